"""The sink archive (mzba.archive.SinkArchive) stated in numpy, for tests/test_cpu_archive.py and
tests/test_gpu_archive.py. Plain numpy plus the oracle's Philox; nothing here calls the library.

* `HostArchive`: `slabs` slabs of `steps` rows, zero-initialised. `append` copies a stage's sink into slab
  (appended % slabs) and applies the tail rule there; `plan` lists the kept segments of the whole archive with every
  last segment closed, as mzba_replay_stream_plan orders them: by env, then by archive row.
* `expected_segments`: the same list from the slabs' specs, through stream_cases.kept_segments.
* `draw`: the window a gather draws without an index list.
"""
import numpy as np

import stream_cases as SC
from oracle import rng as R

STREAM_ARCHIVE = 6  # Philox stream of the gather's draws (csrc/replay.hip)
KEYS = ("action", "reward", "mask", "counts", "values", "frame", "start")


def draw(i, step, seed, N):
    """Window of request i: ((u64)x * N) >> 32 with x the first word of Philox (i, stream 6, step, 0) under seed."""
    return window_of_word(R.philox4x32(i, STREAM_ARCHIVE, step, 0, seed)[0], N)


def window_of_word(x, N):
    """((u64)x * N) >> 32 for 32-bit words x and 0 < N < 2^31."""
    return ((np.asarray(x).astype(np.uint64) * np.uint64(N)) >> np.uint64(32)).astype(np.int64)


class HostArchive:
    def __init__(self, slabs, steps, B, HW=320, cap=SC.CAP_SYN):
        self.slabs, self.steps, self.B, self.cap = slabs, steps, B, cap
        T = slabs * steps
        self.rec = {"action": np.zeros((T, B), np.uint8), "reward": np.zeros((T, B), np.float32),
                    "mask": np.zeros((T, B), np.uint8), "counts": np.zeros((T, B, 3), np.int64),
                    "values": np.zeros((T, B), np.float32), "frame": np.zeros((T, B, HW), np.uint8),
                    "start": np.zeros((T, B), np.uint32)}
        self.appended = 0

    def append(self, rec, done, hlen, tail):
        slab = self.appended % self.slabs
        r0, T = slab * self.steps, self.steps
        for k in KEYS:
            self.rec[k][r0:r0 + T] = rec[k][:T]
        if tail == "drop":
            for b in range(self.B):
                rows = np.flatnonzero(rec["start"][:T, b])
                closed = bool(done[b]) or hlen[b] >= self.cap
                if len(rows) and not closed:
                    self.rec["mask"][r0 + rows[-1]:r0 + T, b] = 0
        self.appended += 1
        return slab

    def plan(self, K=SC.K, min_len=None):
        """[(env, t0, L)]: a segment runs from a start word to the row before the env's next one, or to the archive's
        end; L = its masked rows; kept with L > min_len and L >= K. Every last segment counts as closed."""
        min_len = K + 1 if min_len is None else min_len
        T = self.slabs * self.steps
        out = []
        for b in range(self.B):
            rows = np.flatnonzero(self.rec["start"][:, b])
            for i, t0 in enumerate(rows):
                t1 = T if i + 1 == len(rows) else rows[i + 1]
                L = int(self.rec["mask"][t0:t1, b].sum())
                if L > min_len and L >= K:
                    out.append((b, int(t0), L))
        return out


def expected_segments(slab_specs, steps, min_len=None):
    """slab_specs[j] = (spec, tail) of the stage now in slab j, or None for an unfilled slab -> [(env, t0, L)] = the
    union of kept_segments(spec_j, tail_j) with start rows shifted by j * steps, in (env, archive row) order."""
    out = []
    for j, st in enumerate(slab_specs):
        if st is not None:
            out += [(b, t0 + j * steps, L) for b, t0, L in SC.kept_segments(st[0], st[1], min_len)]
    return sorted(out)


def windows_of(segs, K=SC.K):
    return sum(L - K + 1 for _, _, L in segs)


def oracle_save_segments(o, rec, segs, H=16, W=20):
    """ReplayOracle.save once per listed segment (env, t0, L) of the host sink `rec`, in the list's order (the body of
    stream_cases.oracle_save_stream) -> windows."""
    from mzba.env import gray_lut
    lut = gray_lut()
    n = 0
    for b, t0, L in segs:
        s = slice(t0, t0 + L)
        f0 = lut[SC.render_s0(*SC.unpack_start(rec["start"][t0, b]), H, W)].reshape(H, W)
        o.save(rec["action"][s, b].astype(np.int64), lut[rec["frame"][s, b]].reshape(L, H, W), f0, rec["reward"][s, b],
               rec["counts"][s, b], rec["values"][s, b])
        n += L - SC.K + 1
    return n


def mixed_stages(B, T, seed, tails, H=16, W=20):
    """One stage per entry of `tails`: random specs with runs of envs that have no kept segment; env 1 holds one open
    segment of 14 records in the even stages and no segment at all (no start word in that slab) in the odd ones, so a
    tail that "keep" keeps is followed by a slab in which its env has no start word.
    -> [(spec, tail, rec, done, hlen)]."""
    stages = []
    for j, tail in enumerate(tails):
        spec = SC.random_spec(B, T, seed + j, empty_runs=((5 * j, 5 * j + 3), (B - 4 - j, B - j)))
        spec[1] = ([(14, 14)], False) if j % 2 == 0 else ([], True)
        rec, done, hlen = SC.make_stream_sink(spec, T, H, W, seed=seed + 10 + j)
        stages.append((spec, tail, rec, done, hlen))
    return stages
