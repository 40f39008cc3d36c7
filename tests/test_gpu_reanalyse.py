"""Reanalyse on the GPU, every comparison exact: the representation input rebuilt from the sink
(csrc/reanalyse.hip) against the acting loop's own and against the oracle; a refresh with the recording agent
reproducing the sink bit for bit; a refresh with another net against the existing pieces run row by row; the
ring rewrite (csrc/replay.hip, DeviceReplayBuffer.reingest_records) against a fresh ingest; and the whole chain."""
import ctypes

import numpy as np
import pytest
import torch

import stream_cases as SC
import test_gpu_replay_batch as RB
from oracle.acting import Trajectory, prepare_mcts_input
from mzba.config import small_model_cfg
from mzba.env import gray_lut
from mzba.weights import init_state_dict

pytestmark = pytest.mark.gpu

S = 8


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def _cfg(B, Lh=4, latent=(4, 5), kind="puct"):
    cfg = SC.default_config()
    cfg["model"] = small_model_cfg(cfg)
    cfg["model"]["state_history_length"] = Lh
    cfg["model"]["latent_resolution"] = list(latent)
    cfg["num_simulations"] = S
    cfg["n_parallel"] = B
    cfg["num_episodes"] = 1
    if kind != "puct":
        cfg["search"]["kind"] = kind
    return cfg


def _agent(cfg, sd_seed, dtype="f32"):
    from mzba.agent import MuZeroAgent
    ag = MuZeroAgent(cfg["model"], dtype=dtype)
    ag.load_state_dict(init_state_dict(cfg["model"], sd_seed))
    return ag


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _same(a, b):
    """Byte equality (NaN-proof) of two tensors of one dtype and shape."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bytes(a), _bytes(b))


def _rep_input(rec, frame0, T, HW, Lh, pad, t, out, cs, ctx=None):
    from mzba import _lib as L
    return L.lib().mzba_sink_rep_input(ctypes.byref(L.sink(rec, T, HW)), L.ptr(frame0), Lh, pad, t, L.ptr(ctx), L.ptr(out),
                                       1 if out.dtype == torch.bfloat16 else 0, cs, L.stream())


# ------------------------------------------------------------------------------ 1. the rep input from the sink
def _scripted_loop(cfg, ag, B, H, W, pad, T):
    """An eager ActingLoop over random-init nets that searches as usual but plays a scripted action: most envs keep
    the paddle under the ball and live past the pad boundary, every third one (b % 3 == 1) plays at random and ends
    at a row of its own."""
    from mzba.acting import ActingLoop

    class Scripted(ActingLoop):
        def _sample(self, counts):
            e = self.env
            track = 1 + (e.bx > e.paddle + 3).long() - (e.bx < e.paddle + 2).long()
            rnd = torch.randint(0, 3, (self.B,), generator=self._gen).cuda()
            self.action.copy_(torch.where(self._random, rnd, track))

    loop = Scripted(cfg, ag, B, seed=B + H, height=H, width=W, max_steps=T, pad_action=pad)
    loop._gen = torch.Generator().manual_seed(B)
    loop._random = (torch.arange(B) % 3 == 1).cuda()
    loop.reset(0)
    ins = []
    while loop.t < T:  # past the end of some envs' episodes: their rows are unmasked
        loop._sync_noise_weight()
        loop._noise_in = None
        loop._act_body()
        ins.append(loop.rep_in.clone())
        loop.search_id += 1; loop.step_index += 1; loop.t += 1
    return loop, ins


def _oracle_input(h, f0, b, t, Lh, H, W, pad):
    """prepare_mcts_input on env b's trajectory truncated to t records (host sink h, g(s0) codes f0)."""
    lut = gray_lut()
    g = lambda codes: lut[codes & 7].reshape(1, H, W)  # noqa: E731
    tr = Trajectory(Lh, g(f0[b]), pad)
    for r in range(t):
        tr.add_observation(h["action"][r, b], g(h["frame"][r, b]), h["reward"][r, b], h["counts"][r, b], h["values"][r, b])
    return prepare_mcts_input(g(h["frame"][t - 1, b] if t else f0[b]), tr, Lh)


@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("H,W,Lh,T", [(16, 20, 32, 36), (84, 84, 4, 8)])
def test_rep_input_from_the_sink(H, W, Lh, T, B, dtype, pad):
    """Every row's input, all Cs channels, equals what the acting loop built at that step on the envs it recorded
    there: rows 0, 1, L - 2, L - 1, L and T - 1 among them, B = 1 (one workgroup run per block row), 5, 257; 16x20 is
    two full 128-pixel runs and one of 64, 84x84 ends in a run of 16. One f32 case also against the oracle."""
    cfg = _cfg(B, Lh, (H // 4, W // 4))
    loop, ins = _scripted_loop(cfg, _agent(cfg, 3, dtype), B, H, W, pad, T)
    rec, frame0, HW, cs = loop.rec, loop.frame0, H * W, loop.cs
    assert cs == 64 and len(ins) == T > Lh
    mask = rec["mask"][:T].bool()
    assert mask[Lh].any() and mask[T - 1].any(), "no env lived past the pad boundary"
    if H == 16 and B > 1:
        assert not mask[T - 1].all(), "no env ended inside the episode"
    out = torch.empty_like(loop.rep_in)
    ctx = torch.zeros(3, dtype=torch.int32, device="cuda")
    for t in range(T):
        out.fill_(7)
        assert _rep_input(rec, frame0, T, HW, Lh, pad, t, out, cs) == 0
        got, exp = out.view(B, HW * cs), ins[t].view(B, HW * cs)
        assert torch.isfinite(got.float()).all()
        assert torch.equal(got[mask[t]], exp[mask[t]]), f"row {t}"
        if t in (0, 1, Lh, T - 1):  # the device row in place of the argument
            via = torch.full_like(out, 7)
            ctx.copy_(torch.tensor([99, 5, t], dtype=torch.int32))
            assert _rep_input(rec, frame0, T, HW, Lh, pad, T + 3, via, cs, ctx) == 0
            assert torch.equal(via, out)
    if (H, B, dtype, pad) == (16, 5, "f32", 1):
        h = {k: v[:T].cpu().numpy() for k, v in rec.items() if v is not None}
        f0 = frame0.view(B, HW).cpu().numpy()
        for t in (0, 1, Lh - 2, Lh - 1, Lh, T - 1):
            assert _rep_input(rec, frame0, T, HW, Lh, pad, t, out, cs) == 0
            x = out.view(B, HW, cs).cpu().numpy()
            for b in np.flatnonzero(h["mask"][t]):
                np.testing.assert_array_equal(x[b, :, :2 * Lh].T.reshape(2 * Lh, H, W), _oracle_input(h, f0, b, t, Lh, H, W, pad))
                assert not x[b, :, 2 * Lh:].any()


def test_rep_input_bad_arguments_launch_nothing():
    rec, frame0 = RB.to_device(*RB.make_records([6, 9, 4], 9))
    T, HW, Lh, cs = 9, 320, 4, 64
    out = torch.full((3 * HW * cs,), 7.0, device="cuda")
    calls = {"t = -1": dict(t=-1), "t = T": dict(t=T), "Cs < 2L": dict(cs=4), "Cs % 8": dict(cs=12), "L < 2": dict(Lh=1),
             "pad": dict(pad=3), "HW % 16": dict(HW=328)}
    for name, kw in calls.items():
        a = dict(rec=rec, frame0=frame0, T=T, HW=HW, Lh=Lh, pad=0, t=0, out=out, cs=cs)
        a.update(kw)
        assert _rep_input(**a) < 0, name
    assert _rep_input({**rec, "frame": None}, frame0, T, HW, Lh, 0, 0, out, cs) < 0
    torch.cuda.synchronize()
    assert (out == 7).all()
    # a device row outside the sink: the launch reads and writes nothing
    ctx = torch.tensor([0, 0, T], dtype=torch.int32, device="cuda")
    assert _rep_input(rec, frame0, T, HW, Lh, 0, 0, out, cs, ctx) == 0
    assert (out == 7).all()


# ------------------------------------------------------------------------------ 2. identity
def _episode(cfg, ag, B, seed, env_offset=0, T=24, search_id0=0):
    """One eager episode of the acting loop -> (loop, rows used); its searches run under ids search_id0 + t."""
    from mzba.acting import ActingLoop
    loop = ActingLoop(cfg, ag, B, seed=seed, env_offset=env_offset, max_steps=T)
    loop.search_id = search_id0
    loop.reset(0)
    while not loop.all_done() and loop.t < T:
        loop.act(eager=True)
    return loop, loop.t


def _poisoned(rec, frame0, T):
    """A snapshot whose counts and values hold nothing of the recording: what a refresh must restore on the masked
    rows and must leave on the others."""
    from mzba.reanalyse import Reanalyser
    snap, f0 = Reanalyser.snapshot(rec, frame0, T)
    snap["counts"].fill_(-7)
    snap["values"].fill_(float("nan"))
    return snap, f0


def _check_refreshed(snap, before, rec, T, what):
    m = rec["mask"][:T].bool()
    assert torch.equal(snap["counts"][m], rec["counts"][:T][m]), what
    assert _same(snap["values"][m], rec["values"][:T][m]), what
    assert _same(snap["counts"][~m], before["counts"][~m]) and _same(snap["values"][~m], before["values"][~m]), what
    for k in ("action", "reward", "mask", "frame"):
        assert _same(snap[k], rec[k][:T]), (what, k)


@pytest.mark.parametrize("dtype,kind,B", [("f32", "puct", 5), ("f32", "puct", 257), ("bf16", "puct", 5),
                                          ("bf16", "puct", 257), ("f32", "gumbel", 5), ("bf16", "gumbel", 257)])
def test_refresh_with_the_recording_agent_is_the_identity(dtype, kind, B):
    from mzba.reanalyse import Reanalyser
    cfg = _cfg(B, kind=kind)
    ag = _agent(cfg, 5, dtype)
    seed, off, sid0 = 2024 + B, 3, 11
    loop, T = _episode(cfg, ag, B, seed, off, search_id0=sid0)
    rec, frame0 = loop.rec, loop.frame0
    lens = rec["mask"][:T].sum(0)
    assert len(torch.unique(lens)) > 1 and T > 8, "the envs must finish at different rows"
    rean = Reanalyser(cfg, ag, B, seed=seed, env_offset=off)
    runs = {"eager": [dict(use_graph=False)], "graph": [dict()],
            "halves": [dict(rows=range(1, T, 2)), dict(rows=range(0, T, 2))]}
    for what, calls in runs.items():
        snap, f0 = _poisoned(rec, frame0, T)
        before = {k: v.clone() for k, v in snap.items() if v is not None}
        for kw in calls:
            rean.refresh(snap, f0, T, sid0, **kw)
        _check_refreshed(snap, before, rec, T, what)
        assert torch.equal(f0, frame0)


# ------------------------------------------------------------------------------ 3. a different net
def test_refresh_with_another_net_equals_the_pieces_row_by_row():
    from mzba.reanalyse import Reanalyser
    from mzba.search import MCTSSearchVec, SearchWorkspace
    B, seed, sid0, H, W = 5, 77, 4, 16, 20
    cfg = _cfg(B)
    Lh = cfg["model"]["state_history_length"]
    a, b = _agent(cfg, 5), _agent(cfg, 6)
    loop, T = _episode(cfg, a, B, seed, search_id0=sid0)
    rows = [0, 2, Lh + 3]
    assert T > rows[-1] and loop.rec["mask"][rows[-1]].any()
    snap, f0 = Reanalyser.snapshot(loop.rec, loop.frame0, T)
    assert Reanalyser(cfg, b, B, seed=seed).refresh(snap, f0, T, sid0, rows=rows) == 3
    h = {k: v[:T].cpu().numpy() for k, v in loop.rec.items() if v is not None}
    f0h = f0.view(B, H * W).cpu().numpy()
    ws = SearchWorkspace(MCTSSearchVec(cfg, b, None, seed=seed), B)
    rep = b.runner(B, H, W)
    cs, differs = 64, False
    for t in rows:
        x = np.zeros((B, H * W, cs), np.float32)
        for e in range(B):
            x[e, :, :2 * Lh] = _oracle_input(h, f0h, e, t, Lh, H, W, 0).reshape(2 * Lh, H * W).T
        rep.representation(torch.as_tensor(x).cuda().view(-1), ws.cur, pool=ws.pool, pool_env_stride=(ws.S + 1) * ws.n)
        values, counts = ws.run(sid0 + t)
        m = loop.rec["mask"][t].bool()
        assert m.any()
        assert torch.equal(snap["counts"][t][m], counts[m]) and _same(snap["values"][t][m], values[m]), f"row {t}"
        assert _same(snap["counts"][t][~m], loop.rec["counts"][t][~m])
        differs |= bool((snap["counts"][t][m] != loop.rec["counts"][t][m]).any())
    assert differs, "agent B's searches must not all agree with agent A's"
    others = torch.ones(T, dtype=torch.bool)
    others[rows] = False
    assert _same(snap["counts"][others], loop.rec["counts"][:T][others])


# ------------------------------------------------------------------------------ 4. the ring rewrite
RING = ("past_actions", "future_actions", "states", "rewards", "counts", "values", "targets", "reward_sum")
LENS_A = [24, 0, 7, 8, 12, 6, 17, 24, 15, 1, 16, 9]   # 0, 1, 6, 7: no window (length <= K + 1)
LENS_B = [9, 24, 5, 13, 8, 20]


def _buffer(cap, prioritized=False):
    from mzba.replay import DeviceReplayBuffer
    return DeviceReplayBuffer(RB.HIST, RB.K, cap, RB.DISCOUNT, RB.NSUM, prioritized=prioritized, alpha=0.7)


def _windows(lens):
    return int(sum(n - RB.K + 1 for n in lens if n > RB.K + 1))


def _research(rec, seed):
    """New counts and values on the recorded rows, as a refresh leaves them (poison elsewhere stays)."""
    g = torch.Generator().manual_seed(seed)
    m = rec["mask"].bool()
    rec["counts"][m] = torch.randint(0, 51, (int(m.sum()), 3), generator=g).cuda()
    rec["values"][m] = (torch.randn(int(m.sum()), generator=g) * 2).cuda()


def _ring(buf):
    return {k: buf._ring[k].clone() for k in RING}


def _assert_ring(got, exp, rows=None, what=""):
    for k in RING:
        a, b = (got[k], exp[k]) if rows is None else (got[k][rows], exp[k][rows])
        assert _same(a, b), (what, k)


@pytest.mark.parametrize("prioritized", [False, True])
def test_reingest_equals_a_fresh_ingest(prioritized):
    T = 24
    rec, frame0 = RB.to_device(*RB.make_records(LENS_A, T, seed=1))
    n = _windows(LENS_A)
    x, y = _buffer(n + 5, prioritized), _buffer(n + 5, prioritized)
    assert x.ingest_records(rec, frame0, T) == n and x.last_ingest.n == n
    h, before = x.last_ingest, _ring(x)
    q0 = x._q.clone() if prioritized else None
    assert x.reingest_records(h, rec, frame0, T) == n  # nothing changed: byte-identical
    _assert_ring(_ring(x), before, what="unmodified sink")
    assert not prioritized or _same(x._q, q0)
    _research(rec, 2)
    assert x.reingest_records(h, rec, frame0, T) == n
    assert y.ingest_records(rec, frame0, T) == n
    _assert_ring(_ring(x), _ring(y), what="modified sink")
    assert not _same(x._ring["targets"], before["targets"]) and not _same(x._ring["counts"], before["counts"])
    for k in ("past_actions", "future_actions", "states", "rewards", "reward_sum"):
        assert _same(x._ring[k], before[k]), k
    assert (x.start, x.length) == (y.start, y.length) == (0, n)
    if prioritized:
        assert _same(x.priorities(), y.priorities()) and not _same(x._q, q0)
        assert (x._q[n:] == 0).all() and _same(x._q, y._q)


@pytest.mark.parametrize("prioritized", [False, True])
def test_reingest_after_eviction_leaves_newer_windows_alone(prioritized):
    T = 24
    ra, fa = RB.to_device(*RB.make_records(LENS_A, T, seed=3))
    rb, fb = RB.to_device(*RB.make_records(LENS_B, T, seed=4))
    na, nb = _windows(LENS_A), _windows(LENS_B)
    cap = na + nb - 30  # smaller than the two batches: B's ingest evicts A's 30 oldest windows
    assert nb < cap < na + nb and na > 30
    x = _buffer(cap, prioritized)
    x.ingest_records(ra, fa, T)
    ha = x.last_ingest
    x.ingest_records(rb, fb, T)
    hb = x.last_ingest
    state, before = (x.start, x.length), _ring(x)
    q0 = x._q.clone() if prioritized else None
    _research(ra, 5)
    assert x.reingest_records(ha, ra, fa, T) == na - 30
    assert (x.start, x.length) == state
    slots_b = (hb.head + torch.arange(nb)) % cap
    slots_a = (ha.head + torch.arange(30, na)) % cap
    assert len(set(slots_a.tolist()) | set(slots_b.tolist())) == cap
    _assert_ring(_ring(x), before, slots_b.cuda(), "slots of the newer batch")
    # the reference: the modified A, then B, ingested afresh
    y = _buffer(cap, prioritized)
    y.ingest_records(ra, fa, T)
    y.ingest_records(rb, fb, T)
    _assert_ring(_ring(x), _ring(y), what="against a fresh ingest of the modified batch")
    assert not _same(x._ring["targets"][slots_a.cuda()], before["targets"][slots_a.cuda()])
    if prioritized:
        assert _same(x._q, y._q) and _same(x._q[slots_b.cuda()], q0[slots_b.cuda()])
    # a fully evicted handle, and a handle from before empty_buffer: 0, nothing written
    x.ingest_records(rb, fb, T)
    x.ingest_records(rb, fb, T)
    before = _ring(x)
    q0 = x._q.clone() if prioritized else None
    _research(ra, 6)
    assert x.reingest_records(ha, ra, fa, T) == 0
    x.empty_buffer()
    x.ingest_records(rb, fb, T)
    after_empty = _ring(x)
    assert x.reingest_records(hb, rb, fb, T) == 0 and x.reingest_records(ha, ra, fa, T) == 0
    _assert_ring(_ring(x), after_empty, what="handles from before empty_buffer")
    for k in RING:  # the third ingest of B changed only B's slots: A's reingest wrote nothing in between
        assert _same(after_empty[k][nb:], before[k][nb:]), k
    if prioritized:
        assert (x._q[nb:] == 0).all()  # empty slots stay exactly 0


# ------------------------------------------------------------------------------ 5. end to end
def test_act_ingest_refresh_reingest():
    from mzba.acting import ActingStage
    from mzba.reanalyse import Reanalyser
    from mzba.replay import DeviceReplayBuffer
    B, seed = 5, 2024
    cfg = _cfg(B)
    Lh, K = cfg["model"]["state_history_length"], cfg["num_unroll_steps"]
    a, b = _agent(cfg, 5), _agent(cfg, 6)
    mk = lambda: DeviceReplayBuffer(Lh, K, 200, cfg["discount_factor"], 16, prioritized=True)  # noqa: E731
    x, y = mk(), mk()
    stage = ActingStage(cfg, a, seed=seed, max_steps=24)
    stage.run_episode(x, trajectories=False)
    loop = stage.loop
    T, handle = loop.t, x.last_ingest
    assert handle.n == len(x) > 0
    rec, f0 = Reanalyser.snapshot(loop.rec, loop.frame0, T)
    Reanalyser(cfg, b, B, seed=seed).refresh(rec, f0, T, 0)
    m = rec["mask"].bool()
    assert (rec["counts"][m] != loop.rec["counts"][:T][m]).any()
    assert x.reingest_records(handle, rec, f0.view(B, -1), T) == handle.n
    assert y.ingest_records(rec, f0.view(B, -1), T) == handle.n
    _assert_ring(_ring(x), _ring(y))
    assert _same(x._q, y._q) and (x.start, x.length) == (y.start, y.length)
