"""Reanalyse on streamed sinks on the GPU, every comparison exact: the segment-aware gather
(mzba_sink_rep_input_stream, csrc/reanalyse.hip) against the numpy statement of tests/reanalyse_stream_cases.py, against
the lockstep gather and against the streamed acting loop's own inputs; refresh_stream with the recording agent
reproducing a streamed stage's sink bit for bit; with another net against the pieces run row by row; the ring rewrite
through the segment table (mzba_replay_stream_rewrite, DeviceReplayBuffer.reingest_stream) against a fresh ingest; and
the whole chain."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import reanalyse_stream_cases as RC
import stream_cases as SC
from stream_cases import K, HIST, DISCOUNT
from mzba.config import small_model_cfg
from mzba.weights import init_state_dict

pytestmark = pytest.mark.gpu

POISON = 7
RING = ("past_actions", "future_actions", "states", "rewards", "counts", "values", "targets", "reward_sum")
REWRITTEN = ("counts", "values", "targets")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def _cfg(B, S=20, kind="puct"):
    cfg = SC.default_config()
    cfg["model"] = small_model_cfg(cfg)  # L = 4
    cfg["num_simulations"] = S
    cfg["n_parallel"] = B
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


def _to_device(rec):
    return {k: torch.as_tensor(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in rec.items()}


def _origin(rec, T):
    """The sink's origin table (mzba_sink_origin): i32 (T, B)."""
    from mzba import _lib as L
    origin = torch.full((T, rec["action"].shape[1]), -99, dtype=torch.int32, device="cuda")
    assert L.lib().mzba_sink_origin(ctypes.byref(L.sink(rec, T, 16)), L.ptr(origin), L.stream()) == 0
    return origin


def _gather(rec, T, H, W, Lh, pad, t, out, cs, ctx=None, HW=None, pw=SC.PW, brick_rows=SC.BRICK_ROWS, origin="fill"):
    from mzba import _lib as L
    sink = L.sink(rec, T, H * W if HW is None else HW)
    origin = _origin(rec, T) if isinstance(origin, str) else origin
    return L.lib().mzba_sink_rep_input_stream(ctypes.byref(sink), L.ptr(origin), H, W, pw, brick_rows, Lh, pad, t,
                                              L.ptr(ctx), L.ptr(out), 1 if out.dtype == torch.bfloat16 else 0, cs,
                                              L.stream())


def _expected(host, t, B, Lh, H, W, pad, dtype):
    """The helper's row t for every env as the kernel lays it out: [B][HW][2L] in the output's dtype."""
    x = np.stack([RC.stream_rep_input(host, t, b, Lh, H, W, pad) for b in range(B)]).reshape(B, 2 * Lh, H * W)
    return torch.from_numpy(x).cuda().to(dtype).permute(0, 2, 1)


# ------------------------------------------------------------------------------ 1. the gather on synthetic sinks
@functools.lru_cache(maxsize=1)
def _gather_case(H, W, Lh, T, B):
    """The synthetic sink of one shape, host and device, and its origin table, shared by its dtype and pad cases and
    never written."""
    host = RC.make_gather_sink(RC.gather_spec(B, T, Lh, seed=Lh + B), T, H, W, seed=B)
    rec = _to_device(host)
    return host, rec, _origin(rec, T)


@pytest.mark.parametrize("pad", [0, 2])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("H,W,Lh,T", [(16, 20, 32, 80), (84, 84, 4, 16), (16, 20, 6, 24)])
def test_gather_equals_the_definition(H, W, Lh, T, B, dtype, pad):
    """Every row, every env, all Cs channels, against the numpy statement. Segment lengths 1, L - 1, L, L + 1 and
    2L + 3, start words at consecutive rows; L = 6 puts action planes into the tail of the last frame chunk; 16x20 ends
    in a run of 64 pixels, 84x84 in one of 16; B = 257 is more than one row of workgroups per start row's line."""
    host, rec, origin = _gather_case(H, W, Lh, T, B)
    assert host["mask"].all() and host["start"][0].all() and (host["start"][1:] != 0).any()
    assert np.array_equal(origin.cpu().numpy(), np.arange(T)[:, None] - RC.ages(host["start"])), "the origin table"
    HW, cs = H * W, (2 * Lh + 63) // 64 * 64
    out = torch.empty(B, HW, cs, dtype=dtype, device="cuda")
    ctx = torch.zeros(3, dtype=torch.int32, device="cuda")
    for t in range(T):
        out.fill_(POISON)
        assert _gather(rec, T, H, W, Lh, pad, t, out, cs, origin=origin) == 0
        assert torch.equal(out[:, :, :2 * Lh], _expected(host, t, B, Lh, H, W, pad, dtype)), f"row {t}"
        assert not out[:, :, 2 * Lh:].any(), f"row {t}: the padding channels"
        if t in (0, 1, Lh, T - 1):  # the device row in place of the argument
            via = torch.full_like(out, POISON)
            ctx.copy_(torch.tensor([99, 5, t], dtype=torch.int32))
            assert _gather(rec, T, H, W, Lh, pad, T + 3, via, cs, ctx, origin=origin) == 0
            assert torch.equal(via, out), f"row {t} through ctx"


# ------------------------------------------------------------------------------ 2. against the lockstep gather
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("H,W,Lh,T,B", [(16, 20, 32, 40, 5), (84, 84, 4, 8, 3)])
def test_one_segment_per_env_equals_the_lockstep_gather(H, W, Lh, T, B, dtype):
    from mzba import _lib as L
    host = RC.make_gather_sink(RC.lockstep_like_spec(B, T), T, H, W, seed=3)
    assert host["start"][0].all() and not host["start"][1:].any()
    frame0 = torch.from_numpy(np.stack([SC.render_s0(*SC.unpack_start(w), H, W) for w in host["start"][0]])).cuda()
    rec = _to_device(host)
    HW, cs = H * W, 64
    a, b = (torch.empty(B, HW, cs, dtype=dtype, device="cuda") for _ in range(2))
    for t in range(T):
        a.fill_(POISON); b.fill_(POISON)
        assert _gather(rec, T, H, W, Lh, 1, t, a, cs) == 0
        assert L.lib().mzba_sink_rep_input(ctypes.byref(L.sink(rec, T, HW)), L.ptr(frame0), Lh, 1, t, None, L.ptr(b),
                                           1 if dtype == torch.bfloat16 else 0, cs, L.stream()) == 0
        assert _same(a, b), f"row {t}"


# ------------------------------------------------------------------------------ 3. against the streamed acting loop
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_gather_equals_the_streamed_acting_loop(dtype):
    """An eager streamed stage (B = 8, T = 40, episode_cap = 7, L = 4, S = 20): the input the loop built from its
    history ring at every step, restarts included, rebuilt from the finished sink."""
    from mzba.stream import StreamingStage
    B, T, cap = 8, 40, 7
    cfg = _cfg(B)
    st = StreamingStage(cfg, _agent(cfg, 5, dtype), steps=T, episode_cap=cap, seed=SC.STAGE_SEED, use_graph=False)
    loop, ins = st.loop, []
    act = loop.act

    def act_and_keep(*a, **kw):
        act(*a, **kw)
        ins.append(loop.rep_in.clone())

    loop.act = act_and_keep
    st.run()
    assert len(ins) == T and loop.graph is None
    start = loop.rec["start"].cpu().numpy().view(np.uint32)
    age = RC.ages(start)
    assert (start[1:] != 0).sum() >= B and age.max() == cap - 1 > loop.Lh and loop.rec["mask"][:T].all()
    out = torch.empty_like(loop.rep_in)
    for t in range(T):
        out.fill_(POISON)
        assert _gather(loop.rec, T, loop.H, loop.W, loop.Lh, loop.env.pad_action, t, out, loop.cs, pw=loop.env.pw,
                       brick_rows=loop.env.brick_rows) == 0
        assert _same(out, ins[t]), f"row {t}"


# ------------------------------------------------------------------------------ 4. bad arguments
def test_bad_arguments_launch_nothing():
    T, H, W, Lh, cs, B = 9, 16, 20, 4, 64, 3
    rec = _to_device(RC.make_gather_sink(RC.gather_spec(B, T, Lh, seed=1), T, H, W, seed=2))
    buf = torch.full((B * H * W * cs + 4,), float(POISON), device="cuda")
    out = buf[:B * H * W * cs]
    origin = _origin(rec, T)
    ok = dict(rec=rec, T=T, H=H, W=W, Lh=Lh, pad=0, t=0, out=out, cs=cs, origin=origin)
    calls = {"NULL start": dict(rec={**rec, "start": None}), "NULL origin": dict(origin=None), "H * W != HW": dict(HW=336), "H * W != HW (H)": dict(H=17),
             "W = 257": dict(W=257, H=1, HW=257), "W = 257, HW % 16": dict(W=257, H=16, HW=257 * 16),
             "pad_action = 3": dict(pad=3), "unaligned out": dict(out=buf[1:1 + B * H * W * cs]), "t = T": dict(t=T),
             "t = -1": dict(t=-1), "no frames": dict(rec={**rec, "frame": None}), "Cs < 2L": dict(cs=4),
             "Cs % 8": dict(cs=12), "L < 2": dict(Lh=1), "paddle_width = 0": dict(pw=0), "paddle_width > W": dict(pw=21),
             "brick_rows = 0": dict(brick_rows=0), "brick_rows > H": dict(brick_rows=17)}
    for name, kw in calls.items():
        assert _gather(**{**ok, **kw}) == -1, name
    torch.cuda.synchronize()
    assert (buf == POISON).all()
    # a device row outside the sink: the launch reads and writes nothing
    for row in (-1, T):
        ctx = torch.tensor([0, 0, row], dtype=torch.int32, device="cuda")
        assert _gather(**ok, ctx=ctx) == 0
        assert (buf == POISON).all(), row
    assert _gather(**ok) == 0 and not (out == POISON).any()
    # the origin table: NULL arguments launch nothing; whatever a table holds, the gather clamps it to the sink's rows
    from mzba import _lib as L
    keep = origin.clone()
    assert L.lib().mzba_sink_origin(ctypes.byref(L.sink({**rec, "start": None}, T, H * W)), L.ptr(origin), L.stream()) == -1
    assert L.lib().mzba_sink_origin(ctypes.byref(L.sink(rec, T, H * W)), None, L.stream()) == -1
    assert torch.equal(origin, keep)
    for junk in (-5, T, 2 ** 31 - 1):
        assert _gather(**{**ok, "t": T - 1, "origin": torch.full_like(origin, junk)}) == 0
        assert torch.isfinite(out).all() and not (out == POISON).any(), junk


# ------------------------------------------------------------------------------ 5. identity
def _poisoned(rec, T, done, hlen):
    from mzba.reanalyse import Reanalyser
    snap, d, h = Reanalyser.snapshot_stream(rec, T, done, hlen)
    snap["counts"].fill_(-7)
    snap["values"].fill_(float("nan"))
    return snap


def _check_rows(snap, rec, T, rows, what):
    """The rows `rows` of snap hold the stage's counts and values, the others the poison; nothing else moved."""
    hit = torch.zeros(T, dtype=torch.bool)
    hit[list(rows)] = True
    assert torch.equal(snap["counts"][hit], rec["counts"][:T][hit]), what
    assert _same(snap["values"][hit], rec["values"][:T][hit]), what
    assert (snap["counts"][~hit] == -7).all() and torch.isnan(snap["values"][~hit]).all(), what
    for k in ("action", "reward", "mask", "frame", "start"):
        assert _same(snap[k], rec[k][:T]), (what, k)


@pytest.mark.parametrize("dtype,kind", [("f32", "puct"), ("bf16", "puct"), ("f32", "gumbel"), ("bf16", "gumbel")])
def test_refresh_stream_with_the_recording_agent_is_the_identity(dtype, kind):
    """Two captured streamed stages (B = 8, T = 64, episode_cap = 12, S = 20); after each, refresh_stream under the
    stage's seed and last_search_id0 restores the poisoned counts and values of a snapshot bit for bit: all rows on the
    captured row graph and a subset eagerly after the first stage, all rows eagerly and reversed after the second."""
    from mzba.reanalyse import Reanalyser
    from mzba.stream import StreamingStage
    B, T, cap, seed = SC.STAGE_B, SC.STAGE_T, SC.STAGE_CAP_SHORT, SC.STAGE_SEED
    cfg = _cfg(B, SC.STAGE_S, kind)
    ag = _agent(cfg, SC.STAGE_SD_SEED, dtype)
    st = StreamingStage(cfg, ag, steps=T, episode_cap=cap, seed=seed)
    rean = Reanalyser(cfg, ag, B, seed=seed)
    subset = [5, 0, T - 1, cap, cap + 1, 2 * cap - 1]
    for stage in range(2):
        st.run()
        loop = st.loop
        assert loop.graph is not None and st.last_search_id0 == stage * T
        rec, env = loop.rec, loop.env
        start = rec["start"][:T]
        assert (start[1:] != 0).sum() >= B and (start[0] != 0).all(), "restarts after row 0"
        assert rec["mask"][:T].all()
        # every row on the captured row graph and eagerly (both equal the sink, so each other), one per stage
        runs = [{"graph": dict(), "subset, eager": dict(rows=subset, use_graph=False)},
                {"eager": dict(use_graph=False), "reversed": dict(rows=range(T - 1, -1, -1))}][stage]
        for what, kw in runs.items():
            snap = _poisoned(rec, T, env.done, env.hist_len)
            n = rean.refresh_stream(snap, T, st.last_search_id0, **kw)
            rows = list(kw.get("rows", range(T)))
            assert n == len(rows)
            _check_rows(snap, rec, T, rows, (stage, what))
    assert rean.stream_graph is not None and rean.graph is None  # the lockstep slot was never touched


# ------------------------------------------------------------------------------ 6. a different net
def test_refresh_stream_with_another_net_equals_the_pieces_row_by_row():
    from mzba.reanalyse import Reanalyser
    from mzba.search import MCTSSearchVec, SearchWorkspace
    from mzba.stream import StreamingStage
    B, T, cap, seed, H, W = 8, 24, 7, 77, 16, 20
    cfg = _cfg(B, 8)
    Lh = cfg["model"]["state_history_length"]
    a, b = _agent(cfg, 5), _agent(cfg, 6)
    st = StreamingStage(cfg, a, steps=T, episode_cap=cap, seed=seed, use_graph=False)
    st.loop.search_id = 4
    st.run()
    sid0, loop = st.last_search_id0, st.loop
    assert sid0 == 4
    snap, _, _ = Reanalyser.snapshot_stream(loop.rec, T, loop.env.done, loop.env.hist_len)
    host = {k: v.cpu().numpy() for k, v in snap.items()}
    host["start"] = host["start"].view(np.uint32)
    age = RC.ages(host["start"])
    rows = [0, 2, cap, cap + 1, cap + Lh + 1]
    assert (age[cap] == 0).any() and (age[cap + 1] == 1).any() and (age[cap + Lh + 1] > Lh).any()
    assert Reanalyser(cfg, b, B, seed=seed).refresh_stream(snap, T, sid0, rows=rows) == len(rows)
    ws = SearchWorkspace(MCTSSearchVec(cfg, b, None, seed=seed), B)
    rep = b.runner(B, H, W)
    cs, differs = 64, False
    for t in rows:
        x = np.zeros((B, H * W, cs), np.float32)
        for e in range(B):
            x[e, :, :2 * Lh] = RC.stream_rep_input(host, t, e, Lh, H, W).reshape(2 * Lh, H * W).T
        rep.representation(torch.as_tensor(x).cuda().view(-1), ws.cur, pool=ws.pool, pool_env_stride=(ws.S + 1) * ws.n)
        values, counts = ws.run(sid0 + t)
        assert torch.equal(snap["counts"][t], counts) and _same(snap["values"][t], values), f"row {t}"
        differs |= bool((snap["counts"][t] != loop.rec["counts"][t]).any())
    assert differs, "agent B's searches must not all agree with agent A's"
    others = torch.ones(T, dtype=torch.bool)
    others[rows] = False
    assert _same(snap["counts"][others], loop.rec["counts"][:T][others])
    assert _same(snap["values"][others], loop.rec["values"][:T][others])
    for k in ("action", "reward", "mask", "frame", "start"):
        assert _same(snap[k], loop.rec[k][:T]), k


# ------------------------------------------------------------------------------ 7. the ring rewrite
def _buffer(cap, prioritized=False):
    from mzba.replay import DeviceReplayBuffer
    return DeviceReplayBuffer(HIST, K, cap, DISCOUNT, 64, prioritized=prioritized, alpha=0.7)


def _stream_sink(B, T, seed):
    spec = SC.random_spec(B, T, seed=seed)
    rec, done, hlen = SC.make_stream_sink(spec, T, seed=seed + 1)
    return spec, _to_device(rec), torch.as_tensor(done).cuda(), torch.as_tensor(hlen).cuda()


def _ingest(buf, sink, T, tail):
    _, rec, done, hlen = sink
    return buf.ingest_stream(rec, T, done, hlen, tail=tail, episode_cap=SC.CAP_SYN)


def _reingest(buf, handle, sink, T):
    _, rec, done, hlen = sink
    return buf.reingest_stream(handle, rec, T, done, hlen)


def _research(rec, seed):
    """New counts and values on the recorded rows, as a refresh leaves them (poison elsewhere stays)."""
    g = torch.Generator().manual_seed(seed)
    m = rec["mask"].bool()
    rec["counts"][m] = torch.randint(0, 51, (int(m.sum()), 3), generator=g).cuda()
    rec["values"][m] = (torch.randn(int(m.sum()), generator=g) * 2).cuda()


def _ring(buf):
    return {k: buf._ring[k].clone() for k in RING}


def _assert_ring(got, exp, rows=None, what="", keys=RING):
    for k in keys:
        a, b = (got[k], exp[k]) if rows is None else (got[k][rows], exp[k][rows])
        assert _same(a, b), (what, k)


@pytest.mark.parametrize("tail", ["drop", "keep"])
@pytest.mark.parametrize("prioritized", [False, True])
def test_reingest_stream_equals_a_fresh_ingest(prioritized, tail):
    B, T = 9, 64
    sink = _stream_sink(B, T, seed=21)
    n = sum(L - K + 1 for _, _, L in SC.kept_segments(sink[0], tail))
    assert n > 0 and len(SC.kept_segments(sink[0], "keep")) > len(SC.kept_segments(sink[0], "drop"))
    x, y = _buffer(n + 5, prioritized), _buffer(n + 5, prioritized)
    assert _ingest(x, sink, T, tail) == n
    h, before = x.last_stream_ingest, _ring(x)
    assert (h.head, h.n, h.segments, h.serial, h.epoch, h.tail, h.episode_cap) == \
        (0, n, x.last_stream["segments"], 0, 0, tail, SC.CAP_SYN) and h.min_len == K + 1
    q0 = x._q.clone() if prioritized else None
    assert _reingest(x, h, sink, T) == n  # nothing changed: byte-identical
    _assert_ring(_ring(x), before, what="unmodified sink")
    assert not prioritized or _same(x._q, q0)
    _research(sink[1], 2)
    assert _reingest(x, h, sink, T) == n
    assert _ingest(y, sink, T, tail) == n
    _assert_ring(_ring(x), _ring(y), what="modified sink")
    for k in REWRITTEN:
        assert not _same(x._ring[k], before[k]), k
    _assert_ring(_ring(x), before, what="fields a search does not change", keys=[k for k in RING if k not in REWRITTEN])
    assert (x.start, x.length) == (y.start, y.length) == (0, n)
    if prioritized:
        assert _same(x._q, y._q) and not _same(x._q, q0) and (x._q[n:] == 0).all()
    if tail == "drop":  # a done / hlen that opens the closed tails plans fewer segments than the handle's
        spec, rec, done, hlen = sink
        assert len(SC.kept_segments([(segs, False) for segs, _ in spec], "drop")) < h.segments
        after = _ring(x)
        with pytest.raises(ValueError, match="plans"):
            x.reingest_stream(h, rec, T, torch.zeros_like(done), torch.zeros_like(hlen))
        _assert_ring(_ring(x), after, what="after the refused reingest")


@pytest.mark.parametrize("prioritized", [False, True])
def test_reingest_stream_after_eviction_leaves_newer_windows_alone(prioritized):
    from mzba.replay import live_windows
    B, T, tail, evict = 9, 64, "keep", 30
    sa, sb = _stream_sink(B, T, seed=31), _stream_sink(B, T, seed=41)
    na, nb = (sum(L - K + 1 for _, _, L in SC.kept_segments(s[0], tail)) for s in (sa, sb))
    cap = na + nb - evict  # smaller than the two ingests: B's evicts A's 30 oldest windows
    assert nb < cap and na > evict
    x = _buffer(cap, prioritized)
    _ingest(x, sa, T, tail)
    ha = x.last_stream_ingest
    _ingest(x, sb, T, tail)
    hb = x.last_stream_ingest
    state, before = (x.start, x.length), _ring(x)
    q0 = x._q.clone() if prioritized else None
    _research(sa[1], 5)
    assert live_windows(ha.serial, ha.n, x._written, x.length) == (evict, na - evict)
    assert _reingest(x, ha, sa, T) == na - evict
    assert (x.start, x.length) == state
    slots_b = ((hb.head + torch.arange(nb)) % cap).cuda()
    slots_a = ((ha.head + torch.arange(evict, na)) % cap).cuda()
    assert len(set(slots_a.tolist()) | set(slots_b.tolist())) == cap
    _assert_ring(_ring(x), before, slots_b, "slots of the newer ingest")
    y = _buffer(cap, prioritized)  # the reference: the modified A, then B, ingested afresh
    _ingest(y, sa, T, tail)
    _ingest(y, sb, T, tail)
    _assert_ring(_ring(x), _ring(y), what="against a fresh ingest of the modified sink")
    assert not _same(x._ring["targets"][slots_a], before["targets"][slots_a])
    if prioritized:
        assert _same(x._q, y._q) and _same(x._q[slots_b], q0[slots_b])
    # a fully evicted handle, and handles from before empty_buffer: 0, nothing written
    _ingest(x, sb, T, tail)
    _ingest(x, sb, T, tail)
    before = _ring(x)
    _research(sa[1], 6)
    assert _reingest(x, ha, sa, T) == 0
    _assert_ring(_ring(x), before, what="a fully evicted handle")
    x.empty_buffer()
    _ingest(x, sb, T, tail)
    after_empty = _ring(x)
    assert _reingest(x, hb, sb, T) == 0 and _reingest(x, ha, sa, T) == 0
    _assert_ring(_ring(x), after_empty, what="handles from before empty_buffer")
    if prioritized:
        assert (x._q[nb:] == 0).all()  # empty slots stay exactly 0


def test_rewrite_bad_arguments_launch_nothing():
    from mzba import _lib as L
    B, T = 9, 64
    sink = _stream_sink(B, T, seed=21)
    x = _buffer(400)
    n = _ingest(x, sink, T, "keep")
    _research(sink[1], 3)
    before = _ring(x)
    _, rec, done, hlen = sink
    sk, table, nmax, nseg, n2 = x._plan_stream(rec, T, done, hlen, "keep", K + 1, SC.CAP_SYN)
    assert n2 == n
    ok = dict(sink=ctypes.byref(sk), table=L.ptr(table), nmax=nmax, nseg=nseg, n=n, j_first=0,
              ring=ctypes.byref(x._abi), head=0, dpow=L.ptr(x._powers(T)))
    none = L.sink({**rec, "counts": None}, T, 320)
    calls = {"NULL table": dict(table=None), "j_first < 0": dict(j_first=-1), "segments > nmax": dict(nseg=nmax + 1),
             "segments > windows": dict(nseg=5, n=4), "head = cap": dict(head=400), "NULL dpow": dict(dpow=None),
             "no counts": dict(sink=ctypes.byref(none)), "no segment": dict(nseg=0)}
    for name, kw in calls.items():
        a = {**ok, **kw}
        assert L.lib().mzba_replay_stream_rewrite(a["sink"], a["table"], a["nmax"], a["nseg"], a["n"], a["j_first"],
                                                  a["ring"], a["head"], a["dpow"], L.stream()) == -1, name
    a = {**ok, "j_first": n}  # nothing live: no launch, no error
    assert L.lib().mzba_replay_stream_rewrite(a["sink"], a["table"], a["nmax"], a["nseg"], a["n"], a["j_first"],
                                              a["ring"], a["head"], a["dpow"], L.stream()) == 0
    _assert_ring(_ring(x), before)


# ------------------------------------------------------------------------------ 8. end to end
def test_stage_ingest_refresh_reingest():
    from mzba.reanalyse import Reanalyser
    from mzba.replay import DeviceReplayBuffer
    from mzba.stream import StreamingStage
    B, T, cap, seed = 8, 48, SC.STAGE_CAP_SHORT, 2024
    cfg = _cfg(B, 8)
    Lh = cfg["model"]["state_history_length"]
    ag = _agent(cfg, 5)
    mk = lambda: DeviceReplayBuffer(Lh, K, 400, cfg["discount_factor"], 16, prioritized=True)  # noqa: E731
    x, y = mk(), mk()
    st = StreamingStage(cfg, ag, steps=T, episode_cap=cap, seed=seed)
    st.run()  # not ingested: the next stage's search ids start at T
    st.run(x, tail="keep")
    handle, loop = x.last_stream_ingest, st.loop
    assert handle.n == x.last_stream["windows"] == len(x) > 0 and st.last_search_id0 == T
    rec, done, hlen = Reanalyser.snapshot_stream(loop.rec, T, loop.env.done, loop.env.hist_len)
    ring0 = _ring(x)
    ag.load_state_dict(init_state_dict(cfg["model"], 6))  # the learner's refreshed weights
    assert Reanalyser(cfg, ag, B, seed=seed).refresh_stream(rec, T, st.last_search_id0) == T
    assert (rec["counts"] != loop.rec["counts"][:T]).any()
    assert x.reingest_stream(handle, rec, T, done, hlen) == handle.n
    assert y.ingest_stream(rec, T, done, hlen, tail="keep", episode_cap=cap) == handle.n
    _assert_ring(_ring(x), _ring(y))
    assert _same(x._q, y._q) and (x.start, x.length) == (y.start, y.length)
    assert not _same(x._ring["targets"], ring0["targets"]) and not _same(x._ring["counts"], ring0["counts"])
