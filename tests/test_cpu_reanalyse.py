"""Reanalyse, host side (no GPU): which windows of an earlier ingest are still in the replay ring
(mzba.replay.live_windows) against a brute-force ring, and the sinks Reanalyser.refresh refuses."""
import numpy as np
import pytest
import torch

from mzba.reanalyse import Reanalyser
from mzba.replay import IngestHandle, live_windows


class _Ring:
    """DeviceReplayBuffer's bookkeeping (ingest_records / _commit) with the slots' contents spelled out: each slot
    holds the serial of the window written there last."""

    def __init__(self, cap):
        self.cap, self.start, self.length, self.written = cap, 0, 0, 0
        self.slot = [None] * cap

    def ingest(self, n):
        head = (self.start + self.length) % self.cap
        handle = IngestHandle(head, n, self.written, 0)
        for j in range(max(0, n - self.cap), n):  # mzba_replay_write's window range
            self.slot[(head + j) % self.cap] = self.written + j
        self.written += n
        total = self.length + n
        self.length = min(total, self.cap)
        self.start = (self.start + total - self.length) % self.cap
        return handle

    def live(self, h):
        """The handle's windows j whose slot still holds them."""
        return [j for j in range(h.n) if self.slot[(h.head + j) % self.cap] == h.serial + j]


@pytest.mark.parametrize("seed", range(8))
def test_live_windows_against_a_ring(seed):
    """Random caps and ingest sizes (empty ones, ones larger than the ring): after every ingest, every earlier handle's
    live windows are exactly the range live_windows gives, and they lie inside the ring's stored windows."""
    g = np.random.default_rng(seed)
    cap = int(g.integers(1, 40))
    ring, handles = _Ring(cap), []
    for _ in range(30):
        n = int(g.choice([0, 1, int(g.integers(1, cap + 1)), int(g.integers(cap, 3 * cap + 2))]))
        handles.append(ring.ingest(n))
        stored = {(ring.start + i) % cap for i in range(ring.length)}
        for h in handles:
            j_first, count = live_windows(h.serial, h.n, ring.written, ring.length)
            assert list(range(j_first, j_first + count)) == ring.live(h), (cap, h)
            assert count == 0 or j_first >= h.n - cap  # the rewrite kernel's own lower bound never binds later
            assert {(h.head + j) % cap for j in range(j_first, j_first + count)} <= stored
    assert sum(live_windows(h.serial, h.n, ring.written, ring.length)[1] for h in handles) == ring.length


def test_live_windows_edges():
    assert live_windows(0, 0, 0, 0) == (0, 0)
    assert live_windows(0, 5, 5, 5) == (0, 5)
    assert live_windows(0, 5, 9, 6) == (3, 2)    # four newer windows pushed three out of a ring of six
    assert live_windows(0, 5, 11, 6) == (5, 0)   # exactly evicted
    assert live_windows(0, 50, 50, 6) == (44, 6)  # larger than the ring: only the newest cap were ever written


def _refresher(B=3, H=16, W=20):
    """A Reanalyser's host state without its device buffers: refresh checks the sink before its first launch."""
    r = object.__new__(Reanalyser)
    r.B, r.H, r.W = B, H, W
    return r


def _sink(T=4, B=3, HW=320):
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt)  # noqa: E731
    rec = {"action": z(T, B), "reward": z(T, B, dt=torch.float32), "mask": z(T, B), "frame": z(T, B, HW),
           "counts": z(T, B, 3, dt=torch.int64), "values": z(T, B, dt=torch.float32)}
    return rec, z(B, HW)


def test_refresh_refuses_what_it_cannot_reanalyse():
    rec, frame0 = _sink()
    with pytest.raises(ValueError, match="streamed"):
        _refresher().refresh({**rec, "start": torch.zeros(4, 3, dtype=torch.int32)}, frame0, 4, 0)
    with pytest.raises(ValueError, match="frames"):
        _refresher().refresh({**rec, "frame": None}, frame0, 4, 0)
    with pytest.raises(ValueError, match="envs"):
        _refresher(B=4).refresh(rec, frame0, 4, 0)
    with pytest.raises(ValueError, match="rows"):
        _refresher().refresh(rec, frame0, 5, 0)
    with pytest.raises(ValueError, match="frame0"):
        _refresher().refresh(rec, frame0[:2], 4, 0)
    with pytest.raises(ValueError, match="rows"):
        _refresher().refresh(rec, frame0, 4, 0, rows=[0, 4])
