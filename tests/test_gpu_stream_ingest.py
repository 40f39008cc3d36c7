"""Segmented replay ingest (DeviceReplayBuffer.ingest_stream, csrc/replay.hip) on synthetic streamed sinks, bit for bit
against oracle.replay.ReplayOracle.save called once per kept segment in (env, start row) order, and against
ingest_records where the two must coincide. The sinks are poisoned outside the recorded rows (stream_cases), so a read
past a segment's end shows up in the comparison."""
import numpy as np
import pytest
import torch

import stream_cases as SC
from stream_cases import K, HIST, DISCOUNT
from test_gpu_replay_batch import check_replay, new_buffer, NSUM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def to_device(rec, done, hlen):
    d = {k: torch.as_tensor(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in rec.items()}
    return d, torch.as_tensor(done).cuda(), torch.as_tensor(hlen).cuda()


def ingest(buf, drec, T, tail, **kw):
    rec, done, hlen = drec
    return buf.ingest_stream(rec, T, done, hlen, tail=tail, episode_cap=SC.CAP_SYN, **kw)


@pytest.mark.parametrize("tail", ["drop", "keep"])
def test_big_batch_no_eviction(tail):
    """More envs than the scan kernel's 1024 threads; runs of envs without a kept segment at both ends and in the
    middle (runs of equal offsets ahead of the fill); open and closed tails."""
    B, T = 1025, 24
    spec = SC.random_spec(B, T, seed=B, empty_runs=((0, 3), (B // 2, B // 2 + 41), (B - 3, B)))
    rec, done, hlen = SC.make_stream_sink(spec, T, seed=B + 1)
    kept = SC.kept_segments(spec, tail)
    total = sum(L - K + 1 for _, _, L in kept)
    buf, o = new_buffer(total + 11)
    n_exp = SC.oracle_save_stream(o, rec, spec, tail)
    n = ingest(buf, to_device(rec, done, hlen), T, tail)
    print(f"B={B} tail={tail}: {len(kept)} segments, {n} windows")
    assert n == n_exp == len(o) == total and buf.last_stream == {"segments": len(kept), "windows": total}
    check_replay(buf, o)


def test_bigger_batch_with_eviction():
    """2500 envs (three per scan thread) into a 97-window ring: only the newest 97 windows are written."""
    B, T, cap = 2500, 24, 97
    spec = SC.random_spec(B, T, seed=B, empty_runs=((0, 3), (B // 2, B // 2 + 41), (B - 3, B)))
    rec, done, hlen = SC.make_stream_sink(spec, T, seed=B + 1)
    buf, o = new_buffer(cap)
    n_exp = SC.oracle_save_stream(o, rec, spec, "drop")
    n = ingest(buf, to_device(rec, done, hlen), T, "drop")
    print(f"B={B} cap={cap}: {n} windows, {n - cap} evicted")
    assert n == n_exp and n > 10 * cap
    check_replay(buf, o)


@pytest.mark.parametrize("tail", ["drop", "keep"])
def test_boot_boundary_and_second_ingest_from_a_moved_head(tail):
    """Two segments per env with lengths 10..22: the bootstrap row lies at L - 1, L and L + 1 for every one of a
    window's K positions, in first and in later segments. Twice into a ring smaller than one ingest."""
    B, T, cap = 64, 48, 301
    spec = [([(10 + b % 13, 10 + b % 13), (10 + (b + 5) % 13, 10 + (b + 5) % 13)], b % 3 != 0) for b in range(B)]
    seen = SC.boot_offsets(spec, tail)
    assert all({-1, 0, 1} <= seen[i] for i in range(K))
    rec, done, hlen = SC.make_stream_sink(spec, T, seed=5)
    buf, o = new_buffer(cap)
    drec = to_device(rec, done, hlen)
    for rnd in range(2):
        n_exp = SC.oracle_save_stream(o, rec, spec, tail)
        n = ingest(buf, drec, T, tail)
        assert n == n_exp and n > cap
        if rnd == 0:
            assert (buf.start + buf.length) % cap != 0
        check_replay(buf, o)
    if tail == "keep":
        assert n > sum(L - K + 1 for _, _, L in SC.kept_segments(spec, "drop"))


def test_batch_without_a_window_changes_nothing():
    T = 24
    spec = SC.random_spec(20, T, seed=6)
    rec, done, hlen = SC.make_stream_sink(spec, T, seed=6)
    buf, o = new_buffer(50)
    SC.oracle_save_stream(o, rec, spec, "keep")
    assert ingest(buf, to_device(rec, done, hlen), T, "keep") > 50
    before = {k: v.clone() for k, v in buf._ring.items()}
    start, length = buf.start, len(buf)
    spec2 = [([(1, 1), (K + 1, K + 1), (3, 3)], True), ([], True), ([(K + 1, K + 1)] * 3, False), ([(K, K)], True)]
    rec2, done2, hlen2 = SC.make_stream_sink(spec2, T, seed=7)
    assert not SC.kept_segments(spec2, "keep")
    assert ingest(buf, to_device(rec2, done2, hlen2), T, "keep") == 0
    assert (buf.start, len(buf)) == (start, length)
    for k, v in before.items():
        assert torch.equal(buf._ring[k].view(torch.uint8), v.view(torch.uint8)), k
    check_replay(buf, o)
    # an open tail that would be the only kept segment, dropped
    spec3 = [([(3, 3), (12, 12)], False)]
    rec3, done3, hlen3 = SC.make_stream_sink(spec3, T, seed=8)
    assert ingest(buf, to_device(rec3, done3, hlen3), T, "drop") == 0 and (buf.start, len(buf)) == (start, length)


def test_min_len_minus_one_keeps_length_k():
    T = 24
    spec = [([(L, L), (K + 2 - L % 2, K + 2 - L % 2)], True) for L in range(1, K + 3)]
    rec, done, hlen = SC.make_stream_sink(spec, T, seed=9)
    buf, o = new_buffer(1000)
    n_exp = SC.oracle_save_stream(o, rec, spec, "drop", min_len=-1)
    n = ingest(buf, to_device(rec, done, hlen), T, "drop", min_len=-1)
    assert n == n_exp == len(o) and K in {L for _, _, L in SC.kept_segments(spec, "drop", -1)}
    check_replay(buf, o)


def test_frames_84x84_with_eviction():
    H = W = 84
    T, cap = 32, 23
    spec = [([(16, 16), (9, 9)], True), ([], True), ([(7, 7), (12, 12), (8, 8)], False), ([(5, 5), (15, 15)], True),
            ([(24, 24), (8, 8)], False)]
    rec, done, hlen = SC.make_stream_sink(spec, T, H, W, seed=10)
    from mzba.replay import DeviceReplayBuffer
    from oracle.replay import ReplayOracle
    buf = DeviceReplayBuffer(HIST, K, cap, DISCOUNT, NSUM, height=H, width=W)
    o = ReplayOracle(HIST, K, cap, DISCOUNT, NSUM)
    drec = to_device(rec, done, hlen)
    for rnd in range(2):
        n_exp = SC.oracle_save_stream(o, rec, spec, "keep", H, W)
        n = ingest(buf, drec, T, "keep")
        assert n == n_exp and n > cap
        check_replay(buf, o)


def lockstep_of(rec, segs, T, H=16, W=20):
    """One lockstep env per listed segment (env, t0, L), its records moved to row 0 -> (rec, frame0) for
    ingest_records: the same trajectories in the same order."""
    n, HW = len(segs), H * W
    out = {"action": np.full((T, n), 255, np.uint8), "reward": np.full((T, n), np.nan, np.float32),
           "mask": np.zeros((T, n), np.uint8), "counts": np.full((T, n, 3), -1, np.int64),
           "values": np.full((T, n), np.nan, np.float32), "frame": np.full((T, n, HW), 7, np.uint8)}
    frame0 = np.zeros((n, HW), np.uint8)
    for i, (b, t0, L) in enumerate(segs):
        for k in out:
            out[k][:L, i] = rec[k][t0:t0 + L, b]
        frame0[i] = SC.render_s0(*SC.unpack_start(rec["start"][t0, b]), H, W)
    return out, frame0


@pytest.mark.parametrize("prioritized", [False, True])
def test_ring_equals_ingest_records(prioritized):
    """(a) A sink with one closed segment per env from row 0 (a stage in which no env restarts; lengths as a lockstep
    episode leaves them, rows past the length unmasked): ingest_stream and ingest_records write the same ring, bit for
    bit. (b) A sink with several segments per env against ingest_records of the same segments as one env each. With
    prioritized=True the priorities are equal too."""
    from mzba.replay import DeviceReplayBuffer
    T, cap = 24, 400
    g = np.random.default_rng(12)
    lens = g.choice(np.array([0, 1, 5, 6, 7, 8, 12, 15, 16, 17, 24]), 70)
    one = [([(int(L), T)], True) for L in lens]
    many = SC.random_spec(60, T, seed=13)
    for spec, tail in ((one, "drop"), (many, "drop"), (many, "keep")):
        rec, done, hlen = SC.make_stream_sink(spec, T, seed=14)
        # (a): the sink as it is, env for env; (b): ingest_records applies its own length rule to the listed segments
        segs = [(b, 0, int(L)) for b, L in enumerate(lens)] if spec is one else SC.kept_segments(spec, tail, min_len=-1)
        if spec is one:
            assert (rec["start"][0] != 0).all() and (rec["start"][1:] == 0).all()
        lrec, frame0 = lockstep_of(rec, segs, T)
        bufs = [DeviceReplayBuffer(HIST, K, cap, DISCOUNT, NSUM, prioritized=prioritized, alpha=0.7, prio_eps=1e-2)
                for _ in range(2)]
        for rnd in range(2):  # the second round wraps the ring
            n0 = ingest(bufs[0], to_device(rec, done, hlen), T, tail)
            n1 = bufs[1].ingest_records({k: torch.as_tensor(v).cuda() for k, v in lrec.items()},
                                        torch.as_tensor(frame0).cuda(), T)
            assert n0 == n1 and 2 * n0 > cap and (bufs[0].start, len(bufs[0])) == (bufs[1].start, len(bufs[1]))
            for k in bufs[0]._ring:
                assert torch.equal(bufs[0]._ring[k].view(torch.uint8), bufs[1]._ring[k].view(torch.uint8)), (k, rnd)
            if prioritized:
                assert torch.equal(bufs[0]._q.view(torch.int32), bufs[1]._q.view(torch.int32))
                assert (bufs[0].priorities() > 0).all()
