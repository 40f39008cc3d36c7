"""Episode statistics on the GPU (csrc/episode_stats.hip, mzba.stats.EpisodeStats) against the numpy /
f64 statement of tests/episode_stats_cases.py: integers, extremes, histogram and the per-env lists exactly, the f64
sums within the bound of a reordered sum. The synthetic sinks are poisoned with NaN outside their records
(stream_cases), so a read past a segment's records shows as a NaN in the block."""
import ctypes

import numpy as np
import pytest
import torch

import episode_stats_cases as EC
import stream_cases as SC

pytestmark = pytest.mark.gpu

T = 96
CAP = SC.CAP_SYN
SEEDS = {1: 11, 5: 12, 257: 13}  # tests/test_cpu_episode_stats.py shows what these sinks hold


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def _dev(rec, done, hlen):
    d = {k: torch.as_tensor(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in rec.items()}
    return d, torch.as_tensor(done).cuda(), torch.as_tensor(hlen).cuda()


_SINKS = {}


def _sink(B, seed):
    if (B, seed) not in _SINKS:
        rec, done, hlen = SC.make_stream_sink(SC.random_spec(B, T, seed), T, seed=seed)
        _SINKS[B, seed] = (rec, done, hlen, _dev(rec, done, hlen))
    return _SINKS[B, seed]


def _stats(B, **kw):
    from mzba.stats import EpisodeStats
    return EpisodeStats(B, **kw)


@pytest.mark.parametrize("first_n", [0, 1, 3])
@pytest.mark.parametrize("B", [1, 5, 257])
def test_synthetic_sinks_match_the_oracle(B, first_n):
    rec, done, hlen, (drec, ddone, dhlen) = _sink(B, SEEDS[B])
    st = _stats(B, first_n=first_n, ep_n=4)
    st.add(drec, T, ddone, dhlen, CAP)
    d = st.read()
    o = EC.stats_oracle(rec, T, done, hlen, CAP, first_n=first_n, ep_n=4)
    print({k: (d[k], o[k], EC.f64_bound(o, k)) for k in EC.F64_FIELDS})
    EC.check_block(d, o, (B, first_n))
    EC.check_lists(d, o, (B, first_n))
    if B > 1:
        assert o["episodes"] > 0 and o["verr_rows"] > 0
    assert d["return_mean"] is None or abs(d["return_mean"] - o["ret_sum"] / o["episodes"]) < 1e-9


def test_histogram_arguments_and_edge_bins():
    B = 257
    rec, done, hlen, (drec, ddone, dhlen) = _sink(B, SEEDS[B])
    st = _stats(B, hist_lo=2.0, hist_step=0.25, gamma=0.5)
    st.add(drec, T, ddone, dhlen, CAP)
    d = st.read()
    o = EC.stats_oracle(rec, T, done, hlen, CAP, hist_lo=2.0, hist_step=0.25, gamma=0.5)
    assert o["hist"][0] > 0 and o["hist"][31] > 0
    EC.check_block(d, o, "narrow histogram, gamma 0.5")


def test_accumulation_and_reset():
    B = 5
    r1, d1, h1, (g1, gd1, gh1) = _sink(B, 12)
    r2, d2, h2, (g2, gd2, gh2) = _sink(B, 14)
    st = _stats(B, ep_n=4)
    st.add(g1, T, gd1, gh1, CAP)
    st.add(g2, T, gd2, gh2, CAP)
    o1, o2 = EC.stats_oracle(r1, T, d1, h1, CAP, ep_n=4), EC.stats_oracle(r2, T, d2, h2, CAP, ep_n=4)
    assert o1["episodes"] != o2["episodes"] or o1["rows"] != o2["rows"]
    d = st.read()
    EC.check_block(d, EC.combine(o1, o2), "two sinks")
    EC.check_lists(d, o2, "the lists are the last sink's")
    raw = st.state()
    st.reset()
    assert not st.block.any() and not st.read()["episodes"]
    st.add(g2, T, gd2, gh2, CAP)  # a zeroed block is the empty one: the extremes are this sink's
    EC.check_block(st.read(), o2, "after reset")
    st.load_state(raw)
    EC.check_block(st.read(), EC.combine(o1, o2), "state put back")


def test_archive_slab_equals_the_stage_sink():
    from mzba.archive import SinkArchive
    B = 257
    rec, done, hlen, (drec, ddone, dhlen) = _sink(B, SEEDS[B])
    assert any(not c for _, _, _, c in SC.segments_of(rec["start"], T, done, hlen, CAP))  # tails are dropped
    arc = SinkArchive(2, T, B, SC.K, SC.HIST, SC.DISCOUNT, episode_cap=CAP)
    other = _dev(*SC.make_stream_sink(SC.random_spec(B, T, 3), T, seed=3))
    assert arc.append(other[0], T, other[1], other[2], tail="drop") == 0
    assert arc.append(drec, T, ddone, dhlen, tail="drop") == 1
    a, s = _stats(B, ep_n=4), _stats(B, ep_n=4)
    a.add_slab(arc, 1)
    s.add(drec, T, ddone, dhlen, CAP)
    assert torch.equal(a._buf, s._buf)
    EC.check_block(a.read(), EC.stats_oracle(rec, T, done, hlen, CAP), "slab 1")


def test_graph_capture_accumulates():
    from mzba import _lib as L
    B = 257
    rec, done, hlen, (drec, ddone, dhlen) = _sink(B, SEEDS[B])
    st = _stats(B, ep_n=4)
    st.add(drec, T, ddone, dhlen, CAP)
    eager = st.read()
    graph = L.capture(lambda: st.add(drec, T, ddone, dhlen, CAP))
    st.reset()
    graph.replay()
    graph.replay()
    d = st.read()
    for k in EC.INT_FIELDS:
        assert d[k] == 2 * eager[k], k
    assert d["hist"] == [2 * x for x in eager["hist"]]
    for k in EC.F64_FIELDS:  # x + x is exact
        assert d[k] == 2 * eager[k], k
    for k in ("ret_min", "ret_max", "len_min", "len_max"):
        assert d[k] == eager[k], k
    assert np.array_equal(d["ep_len"], eager["ep_len"])


@pytest.fixture(scope="module")
def acted():
    from mzba.agent import MuZeroAgent
    from mzba.config import small_model_cfg
    from mzba.stream import StreamingStage
    from mzba.weights import init_state_dict
    cfg = SC.default_config()
    cfg["model"] = small_model_cfg(cfg)
    cfg["num_simulations"], cfg["n_parallel"] = SC.STAGE_S, SC.STAGE_B
    ag = MuZeroAgent(cfg["model"], dtype="f32")
    ag.load_state_dict(init_state_dict(cfg["model"], SC.STAGE_SD_SEED))
    st = StreamingStage(cfg, ag, steps=SC.STAGE_T, episode_cap=SC.STAGE_CAP_SHORT, seed=SC.STAGE_SEED)
    st.run()
    return st


def _download(stage):
    env = stage.loop.env
    rec = {k: v[:stage.steps].cpu().numpy() for k, v in stage.loop.rec.items() if v is not None}
    rec["start"] = rec["start"].view(np.uint32)
    return rec, env.done.cpu().numpy(), env.hist_len.cpu().numpy()


def test_a_real_stage(acted):
    B, cap = SC.STAGE_B, SC.STAGE_CAP_SHORT
    st = _stats(B, ep_n=4)
    st.add_stage(acted)
    d = st.read()
    rec, done, hlen = _download(acted)
    o = EC.stats_oracle(rec, SC.STAGE_T, done, hlen, cap, ep_n=4)
    EC.check_block(d, o, "acted stage")
    EC.check_lists(d, o, "acted stage")
    closed = [s for s in SC.segments_of(rec["start"], SC.STAGE_T, done, hlen, cap) if s[3]]
    assert d["episodes"] == len(closed) > B  # every closed segment of an acted stage holds a record
    assert d["capped"] > 0 or d["len_max"] < cap


def test_bad_arguments_return_minus_one_and_leave_the_block():
    from mzba import _lib as L
    B = 5
    _, _, _, (drec, ddone, dhlen) = _sink(B, SEEDS[B])
    lib = L.lib()
    block = torch.full((360,), 0x5A, dtype=torch.uint8, device="cuda")
    ws = torch.empty(int(lib.mzba_stream_episode_stats_ws_bytes(B)), dtype=torch.uint8, device="cuda")
    good = dict(sink=L.sink(drec, T, 320), done=L.ptr(ddone), hlen=L.ptr(dhlen), cap=CAP, first_n=0, gamma=0.985,
                lo=-8.0, step=1.0, block=L.ptr(block), ws=L.ptr(ws), ws_bytes=ws.numel())

    def call(**kw):
        a = {**good, **kw}
        sink = None if a["sink"] is None else ctypes.byref(a["sink"])
        return lib.mzba_stream_episode_stats(sink, a["done"], a["hlen"], a["cap"], a["first_n"], a["gamma"], a["lo"],
                                             a["step"], a["block"], None, None, 0, a["ws"], a["ws_bytes"], L.stream())

    no_start = L.sink({**drec, "start": None}, T, 320)
    bad = [dict(sink=None), dict(sink=no_start), dict(done=None), dict(hlen=None), dict(block=None), dict(ws=None),
           dict(cap=0), dict(first_n=-1), dict(step=0.0), dict(step=-1.0), dict(ws_bytes=ws.numel() - 1)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((block == 0x5A).all())
    block.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    assert int(block[:8].view(torch.int64)) > 0
