"""GPU: the env kernels (csrc/env.hip) on injected states against the env oracle, bit for bit.

tests/env_cases.py builds the states (wins, lone brick bits, the wrap to the bottom row, done envs that still move,
every column of the paddle's hit window) and runs `oracle.env.BreakoutEnvOracle` on them with four distinct dyadic
rewards; tests/test_cpu_env_cases.py holds the floor of envs per class. Here the compact step, the planes step, the
compact step at forced envs-per-block, a lockstep run with the history ring, both sink addressings and the f32 / bf16
representation input, the builder's grid-stride pass, and the brick masks of reset and restart are compared with it
at six brick-word geometries. Every failure names the classes of the envs that differ.
"""
import numpy as np
import pytest
import torch

import env_cases as EC
from oracle.acting import prepare_mcts_input
from oracle.env import convert_to_grayscale

pytestmark = pytest.mark.gpu

STATE = ("paddle", "bx", "by", "dx", "dy", "done", "bricks", "reward", "valid", "hist_frames", "hist_actions",
         "hist_len", "cur_frame", "cur_src")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).cuda()
    return t.to(dtype) if dtype is not None else t


def host(t):
    return t.cpu().numpy()


def rows_equal(got, exp, what, lab):
    """got == exp (as values: -0.0 == 0.0) env by env; the message lists the first envs that differ and their classes."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, f"{what}: shape {got.shape} vs {exp.shape}"
    B = got.shape[0]
    bad = np.flatnonzero((got != exp).reshape(B, -1).any(1))
    if bad.size:
        def show(v):
            return v.tolist() if v.size <= 8 else f"{int((v != 0).sum())} nonzero of {v.size}"
        first = "; ".join(f"env {b} [{lab[b]}] got {show(got[b])} want {show(exp[b])}" for b in bad[:6])
        raise AssertionError(f"{what}: {bad.size} of {B} envs differ: {first}")


def make_env(geom, batch, L=4, single_write=True, rec_flags=0):
    """A compact env reset with explicit legal draws, then overwritten in place with the batch (the ABI struct holds
    the tensors' addresses). Returns the env and the reset draws (the ring's pad frames come from them)."""
    from mzba.env import CompactBreakout
    H, W, rows = EC.GEOMETRIES[geom]
    B = len(batch["paddle"])
    env = CompactBreakout(EC.REWARDS, B, L, H, W, paddle_width=EC.PW, brick_rows=rows, single_write=single_write,
                          rec_flags=rec_flags)
    assert env.nw == EC.nwords(geom)
    params = EC.reset_params(geom, B)
    env.reset(0, params=params)
    for k in ("paddle", "bx", "by", "dx", "dy", "done"):
        getattr(env, k).copy_(dev(batch[k]))
    env.bricks.copy_(dev(EC.words(batch, geom).view(np.int64).reshape(-1)))
    return env, params


def check_step(env, exp, lab, tag):
    """The env after a step against the oracle's outputs of that step."""
    from mzba.env import gray_lut
    B, H, W = env.B, env.H, env.W
    rows_equal(host(env.to_planes()), exp["next_state"], f"{tag} planes", lab)
    rows_equal(host(env.reward), exp["reward"], f"{tag} reward", lab)
    rows_equal(host(env.done) != 0, exp["done"], f"{tag} done", lab)
    rows_equal(host(env.valid), exp["valid"], f"{tag} valid", lab)
    rows_equal(host(env.dx).astype(np.int64), exp["dx"], f"{tag} dx", lab)
    rows_equal(host(env.dy), exp["dy"], f"{tag} dy", lab)
    cur = host(env.current_frame()).reshape(B, H * W)
    assert cur.max() < 8
    rows_equal(gray_lut()[cur], convert_to_grayscale(exp["next_state"]).reshape(B, H * W), f"{tag} current frame", lab)
    rows_equal(cur, EC.codes_of(exp["next_state"]), f"{tag} current frame codes", lab)


def case(geom, seed, n=None):
    """(batch, oracle outputs, class labels) of a generated batch, or of its first n envs."""
    batch, out = EC.make_batch(geom, seed), EC.oracle_step(geom, seed)
    lab = EC.labels(EC.classify(batch, out, geom))
    if n is not None:
        batch, out, lab = EC.take(batch, slice(0, n)), {k: v[:n] for k, v in out.items()}, lab[:n]
    return batch, out, lab


# ------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("seed", EC.SEEDS)
@pytest.mark.parametrize("geom", list(EC.GEOMETRIES))
def test_compact_step_injected_states(geom, seed):
    """One compact step of every injected batch: planes, reward (each of the four terms visible), done, valid, dx, dy
    and the rendered frame equal the oracle's (0.3 s for the slowest case on the MI355X)."""
    batch, out, lab = case(geom, seed)
    env, _ = make_env(geom, batch)
    # the injected state itself round-trips through the compact form
    rows_equal(host(env.to_planes()), out["state"], f"{geom} injected planes", lab)
    env.step(dev(batch["action"]), True)
    check_step(env, out, lab, f"{geom} seed {seed}")
    # record rule at the first step (prev_done aliases done): exactly the envs still live are recorded
    rows_equal(host(env.hist_len), (~out["done"]).astype(np.int32), f"{geom} hist_len", lab)
    rows_equal(host(env.cur_src), (~out["done"]).astype(np.uint8), f"{geom} cur_src", lab)


@pytest.mark.parametrize("seed", EC.SEEDS)
@pytest.mark.parametrize("geom", ["16x20", "84x84"])
def test_planes_step_same_states(geom, seed):
    """The planes kernel on the same planes with the same rewards: its paddle-hit term is visible too."""
    from mzba.env import BreakoutEnvironment
    H, W, rows = EC.GEOMETRIES[geom]
    batch, out, lab = case(geom, seed)
    B = len(batch["paddle"])
    e = BreakoutEnvironment({**EC.REWARDS, "n_parallel": B}, paddle_width=EC.PW)
    e.height, e.width = H, W
    e.ball_dx, e.ball_dy = dev(batch["dx"], torch.int64), dev(batch["dy"])
    done = dev(batch["done"] != 0)
    ns, r, dn, v = e.step(dev(out["state"]), dev(batch["action"]), done)
    assert dn is done
    tag = f"planes kernel {geom} seed {seed}"
    rows_equal(host(ns), out["next_state"], f"{tag} planes", lab)
    rows_equal(host(r), out["reward"], f"{tag} reward", lab)
    rows_equal(host(dn), out["done"], f"{tag} done", lab)
    rows_equal(host(v), out["valid"], f"{tag} valid", lab)
    rows_equal(host(e.ball_dx), out["dx"], f"{tag} dx", lab)
    rows_equal(host(e.ball_dy), out["dy"], f"{tag} dy", lab)


# ------------------------------------------------------------------------------ envs per block
def _sink(T, B, HW):
    rec = {"action": torch.empty(T, B, dtype=torch.uint8, device="cuda"),
           "reward": torch.empty(T, B, dtype=torch.float32, device="cuda"),
           "mask": torch.empty(T, B, dtype=torch.uint8, device="cuda"),
           "frame": torch.empty(T, B, HW, dtype=torch.uint8, device="cuda")}
    for v in rec.values():
        v.view(torch.uint8).fill_(0xAB)
    return rec


@pytest.mark.parametrize("geom,n", EC.BLOCK_CASES)
def test_compact_step_envs_per_block(geom, n):
    """mzba_env_set_block_envs(E) for E in {1, 3, 64, 256}: phase 2's indexing over several envs per block (the
    reciprocal division by the chunk count, the env count of a partial last block, the LDS reads by env) gives what
    the automatic choice (E = 1 at these sizes) and the oracle give. n = 668 / 428 leave the last block partial at
    every E > 1; n = 40 is one block with fewer envs than E."""
    from mzba import _lib as L
    H, W, rows = EC.GEOMETRIES[geom]
    batch, out, lab = case(geom, 0, n)
    action = dev(batch["action"])

    def run():
        env, _ = make_env(geom, batch)
        rec = _sink(1, n, H * W)
        env.step(action, True, rec, 0)
        state = {k: host(getattr(env, k)).reshape(n, -1) for k in STATE}
        state.update({f"sink {k}": host(v[0].view(torch.uint8)).reshape(n, -1) for k, v in rec.items()})
        return env, state

    lib = L.lib()
    assert lib.mzba_env_set_block_envs(257) == -1 and lib.mzba_env_set_block_envs(-1) == -1
    _, auto = run()
    try:
        for E in (1, 3, 64, 256):
            assert n % E != 0 or E == 1
            L.call("mzba_env_set_block_envs", E)
            env, got = run()
            check_step(env, out, lab, f"{geom} B={n} E={E}")
            for k in got:
                rows_equal(got[k], auto[k], f"{geom} B={n} E={E} vs automatic: {k}", lab)
        # a refused value leaves the last accepted one in force
        assert lib.mzba_env_set_block_envs(257) == -1
        _, again = run()
        for k in again:
            rows_equal(again[k], auto[k], f"{geom} B={n} after a refused E: {k}", lab)
    finally:
        L.call("mzba_env_set_block_envs", 0)
    rows_equal(auto["sink frame"], EC.codes_of(out["next_state"]), f"{geom} B={n} sink frame", lab)
    rows_equal(auto["sink mask"], (~out["done"]).astype(np.uint8)[:, None], f"{geom} B={n} sink mask", lab)


# ------------------------------------------------------------------------------ lockstep
def lockstep(geom, seed, n, L, single_write, rec_flags, T):
    """env_cases.oracle_run(geom, seed, n, L, rec_flags, T) on the device: two equal envs, one given the sink by row
    t and one through a device step context, compared with the oracle at every step, and their sinks at the end.
    Returns the envs and the oracle run."""
    from mzba import _lib as Lb
    H, W, rows = EC.GEOMETRIES[geom]
    batch, _, lab = case(geom, seed, n)
    run = EC.oracle_run(geom, seed, n, L, rec_flags, T)
    envs = [make_env(geom, batch, L, single_write, rec_flags)[0] for _ in range(2)]
    recs = [_sink(T, n, H * W), _sink(T, n, H * W)]
    ctx = torch.zeros(3, dtype=torch.int32, device="cuda")
    for t, exp in enumerate(run["steps"]):
        a = dev(run["actions"][t])
        envs[0].step(a, t == 0, recs[0], t)
        envs[1].step(a, False, recs[1], 0, ctx=ctx)  # row and first_step from ctx[2]
        Lb.call("mzba_ctx_advance", Lb.ptr(ctx), Lb.stream())
        for env, how in zip(envs, ("row", "ctx")):
            tag = f"{geom} L={L} single_write={single_write} flags={rec_flags} t={t} sink by {how}"
            check_step(env, exp, lab, tag)
            rows_equal(host(env.hist_len), exp["hist_len"], f"{tag} hist_len", lab)
            if single_write:
                rows_equal(host(env.cur_src), exp["rec"].astype(np.uint8), f"{tag} cur_src", lab)
    for rec, how in zip(recs, ("row", "ctx")):
        for k, want in run["sink"].items():
            got = host(rec[k]).reshape(T, n, -1)
            for t in range(T):
                rows_equal(got[t], want[t].reshape(n, -1), f"{geom} L={L} sink by {how}: {k}[{t}]", lab)
    return envs, run, lab


def check_rep_input(env, trajs, cur_gray, L, lab, tag, Cs=64):
    """build_rep_input in f32 against prepare_mcts_input over the oracle Trajectories, and in bf16 bit-equal to that
    expectation converted on the CPU (both round to nearest even); channels 2L .. Cs are zero."""
    B, H, W = env.B, env.H, env.W
    ref = np.stack([prepare_mcts_input(cur_gray[b], trajs[b], L) for b in range(B)])  # (B, 2L, H, W)
    ref = np.ascontiguousarray(ref.transpose(0, 2, 3, 1)).reshape(B, H * W * 2 * L)
    ref16 = host(torch.from_numpy(ref).to(torch.bfloat16).view(torch.int16))
    for bf16 in (False, True):
        out = torch.full((B, H * W, Cs), -7.0, dtype=torch.bfloat16 if bf16 else torch.float32, device="cuda")
        env.build_rep_input(out, Cs, bf16)
        bits = host(out.view(torch.int16 if bf16 else torch.int32))
        assert not bits[:, :, 2 * L:].any(), f"{tag} bf16={bf16}: pad channels not zero"
        got = bits[:, :, :2 * L].reshape(B, -1)
        rows_equal(got, ref16 if bf16 else ref.view(np.int32), f"{tag} rep input bf16={bf16}", lab)


@pytest.mark.parametrize("single_write", [True, False])
@pytest.mark.parametrize("L", EC.LOCKSTEP_L)
@pytest.mark.parametrize("geom", EC.LOCKSTEP_GEOMETRIES)
def test_compact_lockstep_from_injected_states(geom, L, single_write):
    """T = 3L steps (the ring wraps three times for an env that lives; an env done at the start never records) at the
    headline geometry and at nw = 2, with a ring of one frame (L = 2) and of three, in both frame-storage modes."""
    envs, run, lab = lockstep(geom, EC.LOCKSTEP_SEED, EC.LOCKSTEP_N, L, single_write, 0, 3 * L)
    for i, env in enumerate(envs):
        check_rep_input(env, run["trajs"], run["gray"], L, lab, f"{geom} L={L} single_write={single_write} env {i}")


def test_compact_lockstep_records_every_env_with_env0_action():
    """rec_flags = 3 (the test simulation's rule): every env is recorded at every step, done or not, with env 0's
    action."""
    L = 4
    envs, run, lab = lockstep("16x20", EC.LOCKSTEP_SEED, EC.LOCKSTEP_N, L, True, 3, 3 * L)
    assert all(tr.length == 3 * L for tr in run["trajs"])
    check_rep_input(envs[0], run["trajs"], run["gray"], L, lab, "16x20 flags=3")


def test_rep_input_grid_stride_pass():
    """B = 75 at 84x84 with L = 4, Cs = 64 is the smallest batch whose B*H*W*(Cs/8) threads exceed the builder's grid
    cap of 16384 blocks of 256, so the last envs are written by the grid-stride loop's second pass."""
    geom, L, Cs, B = "84x84", 4, 64, 75
    H, W, _ = EC.GEOMETRIES[geom]
    assert B * H * W * (Cs // 8) > 16384 * 256 >= (B - 1) * H * W * (Cs // 8)
    envs, run, lab = lockstep(geom, 0, B, L, True, 0, 3)
    check_rep_input(envs[0], run["trajs"], run["gray"], L, lab, "84x84 B=75", Cs)


# ------------------------------------------------------------------------------ reset / restart brick masks
@pytest.mark.parametrize("geom", list(EC.GEOMETRIES))
def test_reset_and_restart_brick_masks(geom):
    """reset's per-bit loop mask and restart's nbits formula at 60, 64, 120, 128, 192 and 252 brick bits: the words
    are exactly the low brick_rows * W bits, and the planes, ball direction and frame are the oracle reset's."""
    from mzba.env import CompactBreakout
    H, W, rows = EC.GEOMETRIES[geom]
    B, nw, nbits = 70, EC.nwords(geom), rows * W  # restart: two blocks of 64 envs, the second partial
    full = np.array([((1 << min(max(nbits - 64 * w, 0), 64)) - 1) for w in range(nw)], np.uint64)
    lab = ["reset"] * B
    env = CompactBreakout(EC.REWARDS, B, 4, H, W, paddle_width=EC.PW, brick_rows=rows)
    o = EC.make_oracle(geom, B)

    def check(params, tag):
        so, _ = o.reset(params)
        assert so[:, 2].sum() == B * nbits
        rows_equal(host(env.bricks).view(np.uint64).reshape(B, nw), np.tile(full, (B, 1)), f"{tag} brick words", lab)
        rows_equal(host(env.to_planes()), so, f"{tag} planes", lab)
        rows_equal(host(env.dx).astype(np.int64), o.ball_dx, f"{tag} dx", lab)
        rows_equal(host(env.dy), o.ball_dy, f"{tag} dy", lab)
        assert not host(env.done).any() and not host(env.hist_len).any()
        rows_equal(host(env.current_frame()).reshape(B, H * W), EC.codes_of(so), f"{tag} frame", lab)

    p0 = EC.reset_params(geom, B, seed=1)
    env.bricks.fill_(0x5555555555555555)
    env.reset(0, params=p0)
    check(p0, f"{geom} reset")
    # restart, driven as the streaming stage drives it: row ctx[2] = 2, every env done
    p1 = EC.reset_params(geom, B, seed=2)
    env.done.fill_(1)
    env.bricks.fill_(0x5555555555555555)
    start = torch.zeros(4, B, dtype=torch.int32, device="cuda")
    ctx = torch.tensor([2, 2, 2], dtype=torch.int32, device="cuda")
    blk = torch.tensor([40, 100], dtype=torch.int32, device="cuda")
    env.restart(start, ctx, blk, dev(np.asarray(p1, np.int32)))
    check(p1, f"{geom} restart")
    off, col, row, _ = p1
    word = 0x80000000 | (W // 2 - EC.PW // 2 + off) | (col << 10) | ((H + row) % H << 20)  # include/mzba.h start word
    words = host(start).view(np.uint32)
    rows_equal(words[2], word.astype(np.uint32), f"{geom} start words", lab)
    assert not words[[0, 1, 3]].any()
