"""The sink archive on the GPU (mzba.archive.SinkArchive, mzba_replay_stream_gather).

A gathered window is compared by bytes over all eight ring fields with two independent references: the oracle's
ReplayOracle.save called once per kept segment of the host statement of the archive (archive_cases.HostArchive), and
the parent's ingest_stream of the same stage into a ring large enough to evict nothing. The synthetic sinks are
poisoned outside their records (stream_cases), so a read past a segment's end shows in the comparison."""
import ctypes

import numpy as np
import pytest
import torch

import archive_cases as AC
import stream_cases as SC
from stream_cases import K, HIST, DISCOUNT
from oracle.replay import ReplayOracle
from mzba.env import gray_lut

pytestmark = pytest.mark.gpu

POISON = 0x5A


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def _ring_fields():
    from mzba.archive import RING_FIELDS
    return RING_FIELDS


def _dev(rec, done, hlen):
    d = {k: torch.as_tensor(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in rec.items()}
    return d, torch.as_tensor(done).cuda(), torch.as_tensor(hlen).cuda()


def _i32(x):
    return torch.as_tensor(np.asarray(x, np.int64).astype(np.int32)).cuda()


def _archive(slabs, T, B, H=16, W=20, min_len=None, seq_len=HIST, cap=SC.CAP_SYN):
    from mzba.archive import SinkArchive
    return SinkArchive(slabs, T, B, K, seq_len, DISCOUNT, height=H, width=W, min_len=min_len, episode_cap=cap)


def _ring_of(stage, T, H=16, W=20, min_len=None, seq_len=HIST):
    """The parent's ingest_stream of one stage into a ring that evicts nothing."""
    from mzba.replay import DeviceReplayBuffer
    spec, tail, rec, done, hlen = stage
    n = AC.windows_of(SC.kept_segments(spec, tail, min_len))
    buf = DeviceReplayBuffer(seq_len, K, n + 3, DISCOUNT, 64, height=H, width=W)
    drec, ddone, dhlen = _dev(rec, done, hlen)
    kw = {} if min_len is None else {"min_len": min_len}
    assert buf.ingest_stream(drec, T, ddone, dhlen, tail=tail, episode_cap=SC.CAP_SYN, **kw) == n
    assert (buf.start, len(buf)) == (0, n)
    return buf


def _bytes(t):
    return t.contiguous().view(torch.uint8)


def _poison(staged):
    for t in staged._ring.values():
        _bytes(t).fill_(POISON)


def _is_poison(staged, rows):
    return all(bool((_bytes(t[rows]) == POISON).all()) for t in staged._ring.values())


def _check_oracle(staged, slots, o, widx, H=16, W=20):
    """Rows `slots` of the holder against the oracle's windows `widx`, f32 by bit pattern."""
    lut = gray_lut()
    g = {k: v[torch.as_tensor(np.asarray(slots)).long().cuda()].cpu().numpy() for k, v in staged._ring.items()}
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    n = len(widx)
    np.testing.assert_array_equal(g["past_actions"], o.batched("past_actions", widx))
    np.testing.assert_array_equal(g["future_actions"], o.batched("future_actions", widx))
    assert g["states"].max() < 8
    np.testing.assert_array_equal(bits(lut[g["states"]]), bits(o.batched("states", widx).reshape(n, -1, H * W)))
    for mine, theirs in (("rewards", "rewards"), ("counts", "visit_counts"), ("values", "values"), ("targets", "targets")):
        np.testing.assert_array_equal(bits(g[mine]), bits(o.batched(theirs, widx)), err_msg=mine)
    np.testing.assert_array_equal(bits(g["reward_sum"]), bits(np.array([o.rows[i]["reward_sum"] for i in widx])))


def _check_ring(staged, slots, buf, ring_rows, what=""):
    """Rows `slots` of the holder against rows `ring_rows` of a ring, all eight fields by bytes."""
    a, b = torch.as_tensor(np.asarray(slots)).long().cuda(), torch.as_tensor(np.asarray(ring_rows)).long().cuda()
    for k in _ring_fields():
        assert torch.equal(_bytes(staged._ring[k][a]), _bytes(buf._ring[k][b])), (what, k)


def _by_slab(segs, T):
    """For the archive's kept segments in archive order: per archive window, (slab, window index in that slab's own
    (env, row) order) = where ingest_stream of that slab's stage put it."""
    per_slab, order = {}, []
    for b, t0, L in segs:  # (env, row) order restricted to one slab is that stage's ingest order
        j = t0 // T
        off = per_slab.get(j, 0)
        order.append((j, off, L - K + 1))
        per_slab[j] = off + L - K + 1
    slab = np.concatenate([np.full(n, j) for j, _, n in order]) if order else np.zeros(0, int)
    widx = np.concatenate([off + np.arange(n) for _, off, n in order]) if order else np.zeros(0, int)
    return slab, widx


def _check_all(arc, host, rings, T, H=16, W=20, min_len=None, idx=None):
    """Every window of the archive (or the listed ones), gathered, against both references; rings[j] = the ring of
    the stage now in slab j. -> the number of windows in the archive."""
    segs = host.plan(min_len=min_len)
    N = AC.windows_of(segs)
    assert (arc.segments, arc.windows) == (len(segs), N)
    idx = np.arange(N) if idx is None else np.asarray(idx)
    staged, slots, idx_out = arc.gather(len(idx), idx=_i32(idx))
    assert slots.dtype == torch.int32 and slots.tolist() == list(range(len(idx))) and idx_out.tolist() == idx.tolist()
    assert (staged.start, staged.length, staged.max_length, len(staged)) == (0, len(idx), len(idx), len(idx))
    o = ReplayOracle(arc.hist_seq_len, K, N + 1, DISCOUNT, 64)
    assert AC.oracle_save_segments(o, host.rec, segs, H, W) == N == len(o)
    _check_oracle(staged, np.arange(len(idx)), o, idx, H, W)
    slab, widx = _by_slab(segs, T)
    for j in np.unique(slab[idx]):
        sel = np.flatnonzero(slab[idx] == j)
        _check_ring(staged, sel, rings[j], widx[idx][sel], f"slab {j}")
    return N


def _one_stage(spec, T, tail, seed, H=16, W=20):
    rec, done, hlen = SC.make_stream_sink(spec, T, H, W, seed=seed)
    return spec, tail, rec, done, hlen


def _append(arc, host, stage, T):
    spec, tail, rec, done, hlen = stage
    drec, ddone, dhlen = _dev(rec, done, hlen)
    slab = arc.append(drec, T, ddone, dhlen, tail=tail)
    assert slab == host.append(rec, done, hlen, tail)
    return slab


# ------------------------------------------------------------------------------ 1. the windows
@pytest.mark.parametrize("tail", ["drop", "keep"])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_one_slab_every_window_permuted_with_repeats(B, tail):
    T = 24
    spec = [([(12, 12), (11, 11)], False)] if B == 1 else SC.random_spec(B, T, seed=B, empty_runs=((2, 4),))
    stage = _one_stage(spec, T, tail, seed=B + 1)
    arc, host = _archive(1, T, B), AC.HostArchive(1, T, B)
    _append(arc, host, stage, T)
    N = AC.windows_of(host.plan())
    assert N > 0 and host.plan() == SC.kept_segments(spec, tail)
    g = np.random.default_rng(B)
    idx = np.concatenate([g.permutation(N), g.integers(0, N, 7), [0, N - 1]])
    assert _check_all(arc, host, [_ring_of(stage, T)], T, idx=idx) == N
    print(f"B={B} tail={tail}: {arc.segments} segments, {N} windows, {len(idx)} gathered")


def test_three_slabs_mixed_tails_then_an_overwrite():
    B, T, S = 67, 24, 3
    stages = AC.mixed_stages(B, T, 100, ("keep", "drop", "keep", "drop"))
    arc, host = _archive(S, T, B), AC.HostArchive(S, T, B)
    rings = [None] * S
    for i, stage in enumerate(stages):
        slab = _append(arc, host, stage, T)
        assert slab == i % S
        rings[slab] = _ring_of(stage, T)
        if i >= S - 1:
            segs = host.plan()
            now = [(stages[j][0], stages[j][1]) for j in ((3, 1, 2) if i == 3 else (0, 1, 2))]
            assert segs == AC.expected_segments(now, T) and len({t0 // T for _, t0, _ in segs}) == S
            assert (1, 0, 14) in segs if i == 2 else all(b != 1 or t0 >= T for b, t0, _ in segs)
            N = _check_all(arc, host, rings, T)
            print(f"after append {i}: {arc.segments} segments, {N} windows")
    assert arc.appended == 4 and arc.stored_bytes() == S * T * B * (1 + 4 + 1 + 24 + 4 + 320 + 4)


@pytest.mark.parametrize("tail", ["drop", "keep"])
def test_boot_boundary(tail):
    """test_gpu_stream_ingest's spec: the bootstrap row at L - 1, L and L + 1 for every one of a window's K positions."""
    B, T = 64, 48
    spec = [([(10 + b % 13, 10 + b % 13), (10 + (b + 5) % 13, 10 + (b + 5) % 13)], b % 3 != 0) for b in range(B)]
    seen = SC.boot_offsets(spec, tail)
    assert all({-1, 0, 1} <= seen[i] for i in range(K))
    stage = _one_stage(spec, T, tail, seed=5)
    arc, host = _archive(1, T, B), AC.HostArchive(1, T, B)
    _append(arc, host, stage, T)
    _check_all(arc, host, [_ring_of(stage, T)], T)


def test_frames_84x84():
    H = W = 84
    T = 32
    spec = [([(16, 16), (9, 9)], True), ([], True), ([(7, 7), (12, 12), (8, 8)], False), ([(5, 5), (15, 15)], True),
            ([(24, 24), (8, 8)], False)]
    stage = _one_stage(spec, T, "keep", 10, H, W)
    arc, host = _archive(2, T, 5, H, W), AC.HostArchive(2, T, 5, HW=H * W)
    _append(arc, host, stage, T)
    assert _check_all(arc, host, [_ring_of(stage, T, H, W)], T, H, W) > 0


def test_min_len_minus_one_keeps_length_k():
    T = 24
    spec = [([(L, L), (K + 2 - L % 2, K + 2 - L % 2)], True) for L in range(1, K + 3)]
    stage = _one_stage(spec, T, "drop", 9)
    arc, host = _archive(1, T, len(spec), min_len=-1), AC.HostArchive(1, T, len(spec))
    _append(arc, host, stage, T)
    assert K in {L for _, _, L in host.plan(min_len=-1)}
    _check_all(arc, host, [_ring_of(stage, T, min_len=-1)], T, min_len=-1)


# ------------------------------------------------------------------------------ 2. containment
def _small(slabs=2, B=9, T=24, seed=21, seq_len=HIST):
    spec = SC.random_spec(B, T, seed=seed)
    stage = _one_stage(spec, T, "keep", seed + 1)
    arc, host = _archive(slabs, T, B, seq_len=seq_len), AC.HostArchive(slabs, T, B)
    _append(arc, host, stage, T)
    return arc, host, stage


def test_containment():
    from mzba import _lib as L
    from mzba.archive import StagedWindows
    T = 24
    arc, host, stage = _small()
    ring, N = _ring_of(stage, T), arc.windows
    assert N > 20
    st = StagedWindows(11, HIST, K, 320, arc.device)
    # rows outside [slot0, slot0 + n) keep their bytes
    _poison(st)
    idx = [N - 1, 0, 7, 7, 3]
    out, slots, idx_out = arc.gather(5, idx=_i32(idx), slot0=3, out=st)
    assert out is st and slots.tolist() == [3, 4, 5, 6, 7] and idx_out.tolist() == idx
    _check_ring(st, slots.cpu().numpy(), ring, idx)
    assert _is_poison(st, slice(0, 3)) and _is_poison(st, slice(8, 11))
    # indices outside the archive leave their rows alone
    _poison(st)
    idx = [-1, N, 2 ** 31 - 1, 5, -2 ** 31]
    _, slots, idx_out = arc.gather(5, idx=_i32(idx), slot0=6, out=st)
    assert idx_out.tolist() == [-1, -1, -1, 5, -1]
    _check_ring(st, [9], ring, [5])
    assert _is_poison(st, slice(0, 9)) and _is_poison(st, slice(10, 11))
    # n = 0
    _poison(st)
    _, slots, idx_out = arc.gather(0, idx=torch.empty(0, dtype=torch.int32, device="cuda"), out=st)
    assert slots.numel() == 0 and idx_out.numel() == 0 and _is_poison(st, slice(0, 11))
    # an empty archive: never appended to, and one whose only stage keeps no segment
    empty = _archive(2, T, 9)
    none = _archive(2, T, 4)
    spec = [([(1, 1), (K + 1, K + 1), (3, 3)], True), ([], True), ([(K + 1, K + 1)] * 3, False), ([(12, 12)], False)]
    _, _, rec, done, hlen = _one_stage(spec, T, "drop", 7)
    drec, ddone, dhlen = _dev(rec, done, hlen)
    none.append(drec, T, ddone, dhlen, tail="drop")
    for a in (empty, none):
        assert (a.segments, a.windows, len(a)) == (0, 0, 0)
        _, _, idx_out = a.gather(4, idx=_i32([0, 1, -1, 5]), slot0=2, out=st)
        assert idx_out.tolist() == [-1] * 4 and _is_poison(st, slice(0, 11))
        with pytest.raises(ValueError, match="empty archive"):
            a.gather(4, out=st)
        # the draw itself on an empty table (the raw entry point): skipped, nothing written
        io = torch.zeros(4, dtype=torch.int32, device="cuda")
        assert L.lib().mzba_replay_stream_gather(
            ctypes.byref(a._sink), 16, 20, 6, 3, L.ptr(a._table), a.nmax, L.ptr(a._totals), None, 4, 0, 0, None,
            ctypes.byref(st._abi), 0, L.ptr(a._dpow), L.ptr(io), L.stream()) == 0
        assert io.tolist() == [-1] * 4 and _is_poison(st, slice(0, 11))
    # argument errors: no launch
    gi = _i32([0, 1, 2, 3])
    ok = dict(sink=ctypes.byref(arc._sink), H=16, W=20, table=L.ptr(arc._table), totals=L.ptr(arc._totals), n=4,
              slot0=0, dpow=L.ptr(arc._dpow))
    sink84 = L.sink(arc.rec, arc.T, 84 * 84)
    calls = {"slot0 + n > cap": dict(slot0=8), "slot0 < 0": dict(slot0=-1), "HW mismatch": dict(H=84, W=84),
             "sink HW": dict(sink=ctypes.byref(sink84)), "NULL table": dict(table=None),
             "NULL totals": dict(totals=None), "NULL dpow": dict(dpow=None), "n < 0": dict(n=-1)}
    for name, kw in calls.items():
        a = {**ok, **kw}
        assert L.lib().mzba_replay_stream_gather(
            a["sink"], a["H"], a["W"], 6, 3, a["table"], arc.nmax, a["totals"], L.ptr(gi), a["n"], 0, 0, None,
            ctypes.byref(st._abi), a["slot0"], a["dpow"], None, L.stream()) == -1, name
    with pytest.raises(RuntimeError, match="mzba_replay_stream_gather"):
        arc.gather(4, idx=gi, slot0=8, out=st)
    torch.cuda.synchronize()
    assert _is_poison(st, slice(0, 11))


# ------------------------------------------------------------------------------ 3. device draws
def test_device_draws_and_a_captured_gather():
    from mzba import _lib as L
    from mzba.archive import StagedWindows
    T, n, seed = 24, 33, 77
    arc, host, stage = _small(slabs=2)
    N = arc.windows
    a, b = (StagedWindows(n, HIST, K, 320, arc.device) for _ in range(2))

    def check(idx_out, step, what):
        want = AC.draw(np.arange(n), step, seed, arc.windows)
        assert idx_out.tolist() == want.tolist(), what
        _poison(b)
        arc.gather(n, idx=_i32(want), out=b)
        for k in _ring_fields():
            assert torch.equal(_bytes(a._ring[k]), _bytes(b._ring[k])), (what, k)
        return want

    _poison(a)
    w5 = check(arc.gather(n, step=5, seed=seed, out=a)[2], 5, "host step")
    sd = torch.tensor([9], dtype=torch.int32, device="cuda")
    _poison(a)
    w9 = check(arc.gather(n, step=5, seed=seed, step_dev=sd, out=a)[2], 9, "step_dev")
    assert w5.tolist() != w9.tolist() and len(set(w9.tolist())) > n // 2
    # one captured gather follows the device step and a later append
    res = []
    graph = L.capture(lambda: res.append(arc.gather(n, seed=seed, step_dev=sd, out=a)))
    _poison(a)
    graph.replay()
    check(res[0][2], 9, "replay")
    sd += 1
    _poison(a)
    graph.replay()
    w10 = check(res[0][2], 10, "replay after step_dev += 1")
    assert w10.tolist() != w9.tolist()
    stage2 = _one_stage(SC.random_spec(9, T, seed=31), T, "drop", 32)
    assert _append(arc, host, stage2, T) == 1
    assert arc.windows > N and arc.windows == AC.windows_of(host.plan())
    _poison(a)
    graph.replay()
    w = check(res[0][2], 10, "replay after an append")
    assert w.max() >= N * 2 // 3 and w.tolist() != w10.tolist()


# ------------------------------------------------------------------------------ 4. the learner
def _learner(seed=6):
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    lm = learner_model_cfg()
    assert lm["state_history_length"] == 4
    return Learner(lm, init_state_dict(lm, seed), K=K)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "captured"])
def test_learner_trains_the_same_from_the_staged_windows_and_from_a_ring(captured):
    T, Lh = 24, 4
    arc, host, stage = _small(slabs=1, seq_len=Lh)
    ring = _ring_of(stage, T, seq_len=Lh)
    idx = np.array([3, arc.windows - 1, 0, 11, 12, 5, 17, 8])
    staged, slots, _ = arc.gather(8, idx=_i32(idx))
    _check_ring(staged, np.arange(8), ring, idx)
    x, y = _learner(), _learner()
    ring_slots = _i32(idx)
    if captured:
        x.train_minibatch(staged, slots)
        y.train_minibatch(ring, ring_slots)
        x.capture(staged, 8)
        y.capture(ring, 8)
    for i in range(2):
        lx = x.train_minibatch(staged, slots).clone()
        ly = y.train_minibatch(ring, ring_slots).clone()
        assert lx.shape == (4,) and torch.isfinite(lx).all()
        assert torch.equal(_bytes(lx), _bytes(ly)), i
    assert x.step_count == y.step_count == (3 if captured else 2)
    assert torch.equal(_bytes(x.P), _bytes(y.P))
    assert float(x.P.double().sum()) == float(y.P.double().sum())


# ------------------------------------------------------------------------------ 5. end to end
def test_stages_refresh_and_training_end_to_end():
    from mzba.agent import MuZeroAgent
    from mzba.archive import SinkArchive
    from mzba.config import small_model_cfg
    from mzba.reanalyse import Reanalyser
    from mzba.replay import DeviceReplayBuffer
    from mzba.stream import StreamingStage
    from mzba.weights import init_state_dict
    B, T, cap, seed = SC.STAGE_B, SC.STAGE_T, SC.STAGE_CAP_SHORT, SC.STAGE_SEED
    cfg = SC.default_config()
    cfg["model"] = small_model_cfg(cfg)
    cfg["num_simulations"], cfg["n_parallel"] = SC.STAGE_S, B
    Lh, disc = cfg["model"]["state_history_length"], cfg["discount_factor"]
    ag = MuZeroAgent(cfg["model"], dtype="f32")
    ag.load_state_dict(init_state_dict(cfg["model"], SC.STAGE_SD_SEED))
    mk = lambda: DeviceReplayBuffer(Lh, K, 1000, disc, 16)  # noqa: E731
    st = StreamingStage(cfg, ag, steps=T, episode_cap=cap, seed=seed)
    arc = SinkArchive(2, T, B, K, Lh, disc, episode_cap=cap)
    rings = []
    for s in range(2):
        rings.append(mk())
        st.run(rings[s], tail="drop")
        assert arc.append_stage(st, tail="drop") == s and arc.search_id0[s] == st.last_search_id0
        assert 0 < len(rings[s]) < 1000
    assert arc.windows == len(rings[0]) + len(rings[1])
    assert arc.segments == sum(r.last_stream["segments"] for r in rings)

    host = AC.HostArchive(2, T, B, cap=cap)  # the archive's own rows, downloaded: which window lies in which slab
    for k in ("mask", "start"):
        host.rec[k] = arc.rec[k].cpu().numpy().view(host.rec[k].dtype)
    segs = host.plan()
    N = AC.windows_of(segs)
    assert N == arc.windows
    slab, widx = _by_slab(segs, T)
    in0, in1 = np.flatnonzero(slab == 0), np.flatnonzero(slab == 1)
    assert len(in0) == len(rings[0]) and len(in1) == len(rings[1])
    staged, _, _ = arc.gather(N, idx=_i32(np.arange(N)))
    _check_ring(staged, in0, rings[0], widx[in0], "stage 0")
    _check_ring(staged, in1, rings[1], widx[in1], "stage 1")
    before = {k: v.clone() for k, v in staged._ring.items()}

    # reanalyse slab 1 with another net: nothing follows the refresh
    frozen = {k: arc.rec[k].clone() for k in ("action", "reward", "mask", "frame", "start")}
    ag.load_state_dict(init_state_dict(cfg["model"], 6))
    assert arc.refresh(Reanalyser(cfg, ag, B, seed=seed), 1) == T
    for k, v in frozen.items():
        assert torch.equal(arc.rec[k], v), k
    fresh = mk()  # a fresh ingest of the refreshed slab rows; its tail rule is already in the mask
    ones, zeros = torch.ones(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    assert fresh.ingest_stream(arc.slab_rec(1), T, ones, zeros, tail="keep", episode_cap=cap) == len(in1)
    staged, _, _ = arc.gather(N, idx=_i32(np.arange(N)))
    _check_ring(staged, in1, fresh, widx[in1], "refreshed slab 1")
    a1 = torch.as_tensor(in1).cuda()
    for k in ("past_actions", "future_actions", "states", "rewards", "reward_sum"):
        assert torch.equal(_bytes(staged._ring[k]), _bytes(before[k])), k
    for k in ("counts", "values", "targets"):
        assert not torch.equal(_bytes(staged._ring[k][a1]), _bytes(before[k][a1])), k
    _check_ring(staged, in0, rings[0], widx[in0], "slab 0 after the refresh of slab 1")

    # train from the archive
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    lm = learner_model_cfg()
    lrn = Learner(lm, init_state_dict(lm, 6), K=K)
    step0 = arc.draw_step
    losses = arc.training_stage(lrn, 2, 8, seed=3)
    assert len(losses) == 2 and all(np.isfinite(losses)) and arc.draw_step == step0 + 1 and lrn.step_count == 2
