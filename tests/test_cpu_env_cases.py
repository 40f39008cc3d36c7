"""The injected env states do what the GPU tests need them to (numpy and the oracle alone, no GPU): every batch that
tests/test_gpu_env_cases.py steps holds at least FLOOR envs of every class, so no comparison there can pass on a
batch that never reaches a rule; the states are ones the compact form can hold; and the generator's two forms of a
state describe the same state."""
import numpy as np
import pytest

import env_cases as EC

CASES = [(g, s) for g in EC.GEOMETRIES for s in EC.SEEDS]


@pytest.mark.parametrize("geom,seed", CASES)
def test_every_class_reaches_the_floor(geom, seed):
    batch, out = EC.make_batch(geom, seed), EC.oracle_step(geom, seed)
    counts = {k: int(m.sum()) for k, m in EC.classify(batch, out, geom).items()}
    print(geom, seed, "B", len(batch["paddle"]), counts)
    assert tuple(counts) == EC.CLASSES
    short = {k: n for k, n in counts.items() if n < EC.FLOOR}
    assert not short, f"{geom} seed {seed}: classes under the floor of {EC.FLOOR}: {short}"


@pytest.mark.parametrize("geom,seed", CASES)
def test_states_are_compact_representable(geom, seed):
    H, W, rows = EC.GEOMETRIES[geom]
    b = EC.make_batch(geom, seed)
    B = len(b["paddle"])
    assert B <= 700 and H * W % 16 == 0 and W % 2 == 0 and W > EC.PW
    assert EC.nwords(geom) == {"16x20": 1, "84x84": 4, "8x40": 2, "16x64": 3, "8x16": 1, "8x32": 2}[geom]
    assert b["bricks"].shape == (B, rows, W)
    assert ((b["paddle"] >= 0) & (b["paddle"] <= W - EC.PW)).all()
    assert ((b["bx"] >= 0) & (b["bx"] < W) & (b["by"] >= 0) & (b["by"] < H)).all()
    done = b["done"] != 0
    assert set(np.unique(b["done"])) == {0, 1} and set(np.unique(b["action"])) == {0, 1, 2}
    assert (np.abs(b["dx"][~done]) == 1).all() and (np.abs(b["dy"][~done]) == 1).all()
    assert not b["bricks"][done].any()
    assert ((b["dx"][done] == 0) == (b["dy"][done] == 0)).all()
    # paddle columns next to both walls, the ball in both edge columns and on the top and bottom rows
    for p in (0, 1, W - EC.PW - 1, W - EC.PW):
        assert (b["paddle"][~done] == p).sum() >= EC.FLOOR
    for col in (0, W - 1):
        assert (b["bx"] == col).sum() >= EC.FLOOR
    for row in (0, H - 1):
        assert (b["by"] == row).sum() >= EC.FLOOR
    # brick masks: full, empty while live, a lone bit, and (nw > 1) bricks in the last word alone
    flat = b["bricks"].reshape(B, -1)
    n = flat.sum(1)
    assert (n == rows * W).sum() >= EC.FLOOR and ((n == 0) & ~done).sum() >= EC.FLOOR and (n == 1).sum() >= EC.FLOOR
    if EC.nwords(geom) > 1:
        assert ((n > 0) & ~flat[:, :64].any(1)).sum() >= EC.FLOOR, "no env's bricks lie outside word 0 alone"
    again = EC.make_batch.__wrapped__(geom, seed)
    assert all(np.array_equal(b[k], again[k]) for k in b)


@pytest.mark.parametrize("geom,seed", CASES)
def test_planes_and_compact_forms_agree(geom, seed):
    H, W, rows = EC.GEOMETRIES[geom]
    b = EC.make_batch(geom, seed)
    w = EC.words(b, geom)
    assert w.dtype == np.uint64 and w.shape == (len(b["paddle"]), EC.nwords(geom))
    s = EC.planes(b, geom)
    np.testing.assert_array_equal(EC.compact_to_planes(b["paddle"], b["bx"], b["by"], b["done"], w, geom), s)
    # the planes the oracle steps: one ball, a contiguous paddle of pw on the last row or none, bricks in the brick rows
    assert (s[:, 1].sum((1, 2)) == 1).all()
    assert (s[:, 0].sum((1, 2)) == np.where(b["done"] != 0, 0, EC.PW)).all() and not s[:, 0, :H - 1].any()
    assert not s[:, 2, rows:].any()
    if rows * W % 64 == 0:  # bit 63 of the last word is a brick of the field
        assert (w[:, -1] >> np.uint64(63)).any()
    else:
        assert not (w[:, -1] >> np.uint64(rows * W % 64)).any()


@pytest.mark.parametrize("geom,n", EC.BLOCK_CASES)
def test_envs_per_block_batches_keep_the_classes(geom, n):
    """The first n envs that the envs-per-block test steps: the large batches still hold the floor of every class and
    end in a partial block at every forced E > 1; the one-block batches (n < E) hold what the render tells apart: envs
    that stay live (paddle and bricks drawn, frame recorded) and envs that end or were done (neither)."""
    batch, out = EC.make_batch(geom, 0), EC.oracle_step(geom, 0)
    counts = {k: int(m[:n].sum()) for k, m in EC.classify(batch, out, geom).items()}
    assert n <= len(batch["paddle"])
    if n > 256:
        assert all(n % E for E in (3, 64, 256))
        short = {k: c for k, c in counts.items() if c < EC.FLOOR}
        assert not short, f"{geom} first {n}: classes under the floor of {EC.FLOOR}: {short}"
    else:
        assert n < 64
        assert all(counts[k] for k in ("won_live", "done_still", "done_velocity", "brick_up", "valid0_zero")), counts
        assert (~out["done"][:n]).sum() >= EC.FLOOR


def test_reward_names_its_terms():
    v = list(EC.REWARDS.values())
    sums = {sum(x for i, x in enumerate(v) if m >> i & 1) for m in range(16)}
    assert len(sums) == 16 and all(np.float32(x) == x for x in sums)


def test_reset_params_are_legal():
    for geom, (H, W, rows) in EC.GEOMETRIES.items():
        off, col, row, dx = EC.reset_params(geom, 300)
        p = W // 2 - EC.PW // 2 + off
        assert p.min() == 0 and p.max() == W - EC.PW and col.min() >= 0 and col.max() < W
        assert set(row) == {-3, -2} and set(dx) == {-1, 1}


@pytest.mark.parametrize("L", EC.LOCKSTEP_L)
@pytest.mark.parametrize("geom", EC.LOCKSTEP_GEOMETRIES)
def test_lockstep_runs_reach_the_ring_and_the_record_rule(geom, L):
    """The lockstep runs the GPU test follows: some env is never recorded (done when injected), some env is recorded
    at all 3L steps (the ring of L - 1 frames wraps three times), envs finish at different steps in between (won and
    lost), an env is recorded at the step that ends it, and the sink rows follow rec = ~prev_done."""
    T, n = 3 * L, EC.LOCKSTEP_N
    run = EC.oracle_run(geom, EC.LOCKSTEP_SEED, n, L, 0, T)
    lens = run["steps"][-1]["hist_len"]
    print(geom, L, "records per env:", np.bincount(lens, minlength=T + 1))
    assert (lens == 0).sum() >= EC.FLOOR and (lens == T).sum() >= EC.FLOOR and len(np.unique(lens)) >= L + 2
    assert lens.tolist() == [tr.length for tr in run["trajs"]] == run["sink"]["mask"].sum(0).tolist()
    done = np.stack([s["done"] for s in run["steps"]])
    rec = run["sink"]["mask"].astype(bool)
    np.testing.assert_array_equal(rec[0], ~done[0])
    np.testing.assert_array_equal(rec[1:], ~done[:-1])
    assert (rec[1:] & done[1:]).any()  # recorded at the step that ends it
    r = run["sink"]["reward"]
    assert (r[rec] == -1.5).any() and (r[rec] == 0.25).any() and (r[rec] == 1.0).any()
    assert (r[~rec] >= 3.0).any()  # the win term: a win at step 0 is not recorded, and a done env "wins" every step
    assert (run["sink"]["action"] == run["actions"]).all()
    # every env recorded with env 0's action
    run3 = EC.oracle_run("16x20", EC.LOCKSTEP_SEED, n, 4, 3, 12)
    assert run3["sink"]["mask"].all() and (run3["sink"]["action"] == run3["actions"][:, :1]).all()
    assert (run3["actions"] != run3["actions"][:, :1]).any()
