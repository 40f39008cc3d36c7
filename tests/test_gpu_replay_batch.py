"""Batched replay ingest (csrc/replay.hip) against oracle.replay.ReplayOracle, bit for bit.

The acting loop's sink is built directly as device tensors, so a batch can hold what an episode of a
random-init agent never does: more envs than the plan kernel has threads, runs of envs that yield no
window at the start, in the middle and at the end of the batch, every position of the n-step target's
bootstrap against the trajectory's end, a batch with no window at all, and 84x84 frames. Everything
past a trajectory's length is poison (NaN reward and value, action 255, counts -1, frame code 7), so a
read past the length shows up in the comparison.
"""
import numpy as np
import pytest
import torch

from oracle.replay import ReplayOracle
from mzba.config import default_config
from mzba.env import gray_lut

pytestmark = pytest.mark.gpu

CFG = default_config()
K, HIST, DISCOUNT = CFG["num_unroll_steps"], CFG["model"]["state_history_length"], CFG["discount_factor"]
NSUM = 64
LENGTHS_POOL = np.array([0, 1, 5, 6, 7, 8, 12, 15, 16, 17, 24])
REWARDS = np.array([-1, 0, 0, 1, 5, 6, 0.3], np.float32)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def make_records(lens, T, H=16, W=20, seed=0):
    """Host arrays in the sink's layouts (include/mzba.h), poisoned at t >= lens[b]."""
    g = np.random.default_rng(seed)
    lens = np.asarray(lens)
    B, HW = len(lens), H * W
    assert lens.max() <= T
    live = np.arange(T)[:, None] < lens[None, :]  # [T][B]
    rec = {
        "action": np.where(live, g.integers(0, 3, (T, B)), 255).astype(np.uint8),
        "reward": np.where(live, g.choice(REWARDS, (T, B)), np.float32(np.nan)).astype(np.float32),
        "mask": live.astype(np.uint8),
        "counts": np.where(live[..., None], g.multinomial(50, [0.3, 0.3, 0.4], (T, B)), -1).astype(np.int64),
        "values": np.where(live, (g.normal(size=(T, B)) * 2).astype(np.float32), np.float32(np.nan)).astype(np.float32),
        "frame": np.where(live[..., None], g.integers(0, 5, (T, B, HW)), 7).astype(np.uint8),
    }
    frame0 = g.integers(0, 5, (B, HW)).astype(np.uint8)
    return rec, frame0


def to_device(rec, frame0):
    return {k: torch.as_tensor(v).cuda() for k, v in rec.items()}, torch.as_tensor(frame0).cuda()


def oracle_save(o, rec, frame0, lens, H=16, W=20, min_len=K + 1):
    """The batch's trajectories in env order into the oracle, under ingest_records' length rule.
    -> the number of windows the batch yields (evicted ones included)."""
    lut = gray_lut()
    n = 0
    for b, L in enumerate(lens):
        if L > min_len and L >= K:
            o.save(rec["action"][:L, b].astype(np.int64), lut[rec["frame"][:L, b]].reshape(L, H, W),
                   lut[frame0[b]].reshape(H, W), rec["reward"][:L, b], rec["counts"][:L, b], rec["values"][:L, b])
            n += L - K + 1  # replay_buffer.py:96: one window per state in range(L - K + 1)
    return n


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def check_replay(buf, o, order=None, chunk=1024):
    """Every getter against the oracle's rows (test_gpu_parity._check_replay, f32 by bit pattern), in
    chunks so that a large buffer's frames are never held twice. order: window indices, default all."""
    assert len(buf) == len(o)
    order = np.arange(len(o)) if order is None else np.asarray(order)
    for i0 in range(0, len(order), chunk):
        idx = torch.as_tensor(order[i0:i0 + chunk])
        np.testing.assert_array_equal(buf.get_batched_past_actions(idx).cpu().numpy(), o.batched("past_actions", idx))
        np.testing.assert_array_equal(buf.get_batched_future_actions(idx).cpu().numpy(), o.batched("future_actions", idx))
        _bits(buf.get_batched_states(idx).cpu().numpy()[:, :, 0], o.batched("states", idx))
        _bits(buf.get_batched_rewards(idx).cpu().numpy(), o.batched("rewards", idx))
        _bits(buf.get_batched_visit_counts(idx).cpu().numpy(), o.batched("visit_counts", idx))
        _bits(buf.get_values(idx).cpu().numpy(), o.batched("values", idx))
        _bits(buf.get_batched_values(idx).cpu().numpy(), o.batched("targets", idx))
    _bits(np.array(buf.get_reward_sums(), np.float32), o.reward_sums())


def new_buffer(max_length, H=16, W=20):
    from mzba.replay import DeviceReplayBuffer
    return (DeviceReplayBuffer(HIST, K, max_length, DISCOUNT, NSUM, height=H, width=W),
            ReplayOracle(HIST, K, max_length, DISCOUNT, NSUM))


def big_batch_lengths(B, seed):
    """Lengths from the pool; the first three envs, the last three and 41 consecutive ones in the middle
    yield no window (length <= K + 1)."""
    g = np.random.default_rng(seed)
    lens = g.choice(LENGTHS_POOL, B)
    none = LENGTHS_POOL[LENGTHS_POOL <= K + 1]
    for lo, hi in ((0, 3), (B - 3, B), (B // 2, B // 2 + 41)):
        lens[lo:hi] = g.choice(none, hi - lo)
    return lens


@pytest.mark.parametrize("B", [1025, 2500])
def test_big_batch_no_eviction(B):
    """More envs than the plan kernel's 1024 threads (2 and 3 envs per thread), windowless runs at both ends
    and in the middle of the batch (runs of equal offsets under the write kernel's binary search)."""
    T = 24
    lens = big_batch_lengths(B, seed=B)
    assert (lens[:3] <= K + 1).all() and (lens[-3:] <= K + 1).all() and (lens[B // 2:B // 2 + 41] <= K + 1).all()
    rec, frame0 = make_records(lens, T, seed=B + 1)
    total = int(np.where(lens > K + 1, lens - K + 1, 0).sum())
    buf, o = new_buffer(total + 11)
    n_exp = oracle_save(o, rec, frame0, lens)
    drec, dframe0 = to_device(rec, frame0)
    n = buf.ingest_records(drec, dframe0, T)
    print(f"B={B}: {n} windows, 0 evicted, {int((lens <= K + 1).sum())} envs without a window")
    assert n == n_exp == len(o) == total
    check_replay(buf, o)


@pytest.mark.parametrize("B", [1025, 2500])
def test_big_batch_with_eviction(B):
    """The same batches into a 97-window ring, twice: far more windows than slots (only the newest 97 are
    written), and the second ingest starts from a non-zero head."""
    T, cap = 24, 97
    lens = big_batch_lengths(B, seed=B)
    rec, frame0 = make_records(lens, T, seed=B + 1)
    buf, o = new_buffer(cap)
    drec, dframe0 = to_device(rec, frame0)
    for rnd in range(2):
        n_exp = oracle_save(o, rec, frame0, lens)
        n = buf.ingest_records(drec, dframe0, T)
        assert n == n_exp and n > 10 * cap
        if rnd == 0:
            assert (buf.start + buf.length) % cap != 0  # where the second ingest starts
        print(f"B={B} cap={cap} ingest {rnd}: {n} windows, {n - cap if rnd == 0 else n} evicted")
        check_replay(buf, o)


def test_boot_boundary_at_every_window_position():
    """The n-step target bootstraps 10 steps ahead while that lies inside the trajectory (boot < L): lengths
    10..22 put boot at L - 1, L and L + 1 for every one of a window's K positions."""
    B, T = 64, 24
    lens = 10 + np.arange(B) % 13
    seen = {i: set() for i in range(K)}
    for L in lens:
        for s in range(L - K + 1):
            for i in range(K):
                seen[i].add(s + 10 + i - L)
    assert all({-1, 0, 1} <= seen[i] for i in range(K))
    rec, frame0 = make_records(lens, T, seed=5)
    buf, o = new_buffer(4096)
    n_exp = oracle_save(o, rec, frame0, lens)
    n = buf.ingest_records(*to_device(rec, frame0), T)
    print(f"boot boundary: {n} windows, 0 evicted")
    assert n == n_exp == len(o)
    check_replay(buf, o)


def test_batch_without_a_window_changes_nothing():
    T = 24
    lens = 10 + np.arange(20) % 13
    rec, frame0 = make_records(lens, T, seed=6)
    buf, o = new_buffer(150)  # the prior ingest evicts: start != 0
    oracle_save(o, rec, frame0, lens)
    n0 = buf.ingest_records(*to_device(rec, frame0), T)
    assert n0 > 150
    before = {k: v.clone() for k, v in buf._ring.items()}
    start, length = buf.start, len(buf)
    lens2 = np.array([0, 1, 5, 6, 2, 3, 4, 6, 0, 6, 5, 1])
    assert lens2.max() <= K + 1
    rec2, frame02 = make_records(lens2, T, seed=7)
    n = buf.ingest_records(*to_device(rec2, frame02), T)
    print(f"no windows: {n} windows after a prior ingest of {n0} ({n0 - 150} evicted)")
    assert n == 0 == oracle_save(o, rec2, frame02, lens2)
    assert (buf.start, len(buf)) == (start, length)
    for k, v in before.items():
        assert torch.equal(buf._ring[k].view(torch.uint8), v.view(torch.uint8)), k
    check_replay(buf, o)
    # and into an empty buffer
    buf, o = new_buffer(150)
    assert buf.ingest_records(*to_device(rec2, frame02), T) == 0 and len(buf) == 0
    assert all(not v.any() for v in buf._ring.values())


def test_min_len_minus_one_keeps_length_k():
    """min_len = -1 (save_observation_trajectory's rule): L == K gives one window, L < K none."""
    B, T = 40, 24
    lens = np.arange(B) % (K + 3)
    rec, frame0 = make_records(lens, T, seed=8)
    buf, o = new_buffer(1000)
    n_exp = oracle_save(o, rec, frame0, lens, min_len=-1)
    n = buf.ingest_records(*to_device(rec, frame0), T, min_len=-1)
    print(f"min_len=-1: {n} windows, 0 evicted")
    assert B % (K + 3) == 0  # whole cycles of 0..K+2: lengths K, K + 1, K + 2 give 1 + 2 + 3 windows a cycle
    assert n == n_exp == len(o) == 6 * (B // (K + 3))
    check_replay(buf, o)


def test_frames_84x84_with_eviction():
    """Config 3's frames (HW = 7056), two ingests into a ring smaller than one batch's windows."""
    H = W = 84
    T, cap = 16, 23
    lens = np.array([16, 0, 7, 12, 16, 5, 8, 15, 6])
    rec, frame0 = make_records(lens, T, H, W, seed=9)
    buf, o = new_buffer(cap, H, W)
    drec, dframe0 = to_device(rec, frame0)
    for rnd in range(2):
        n_exp = oracle_save(o, rec, frame0, lens, H, W)
        n = buf.ingest_records(drec, dframe0, T)
        print(f"84x84 ingest {rnd}: {n} windows, {n - cap if rnd == 0 else n} evicted")
        assert n == n_exp and n > cap
        check_replay(buf, o)


def test_get_batched_states_permuted_across_the_wrap_and_empty():
    """Every getter under a permuted index with repeats over a ring whose windows wrap, and an empty index
    (the regression case: mzba_replay_states used to refuse the storage-less tensors of an empty batch)."""
    T, cap = 24, 97
    lens = 10 + np.arange(30) % 13
    rec, frame0 = make_records(lens, T, seed=10)
    buf, o = new_buffer(cap)
    oracle_save(o, rec, frame0, lens)
    buf.ingest_records(*to_device(rec, frame0), T)
    assert len(buf) == cap and buf.start != 0  # windows start..cap-1 and 0..start-1: the index wraps
    g = np.random.default_rng(11)
    order = np.concatenate([g.permutation(cap), g.integers(0, cap, 40)])  # every window, then repeats
    check_replay(buf, o, order=order, chunk=len(order))
    empty = torch.empty(0, dtype=torch.int64)
    assert tuple(buf.get_batched_states(empty).shape) == (0, HIST, 1, 16, 20)
    assert tuple(buf.get_batched_values(empty).shape) == (0, K)
    assert tuple(buf.get_batched_past_actions(empty).shape) == (0, HIST)
    with pytest.raises(IndexError):
        buf.get_batched_states(torch.tensor([cap]))
