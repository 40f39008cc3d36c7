"""TEST INFRASTRUCTURE ONLY: prioritized replay over the sink archive (mzba.archive, csrc/archive_prio.hip, DESIGN.md
§19) restated in numpy, for tests/test_cpu_archive_prio.py and tests/test_gpu_archive_prio.py. Plain numpy, the
oracle's Philox, archive_cases and per_reference; nothing here calls the library.

* `plan_arrays` / `lookup`: the row -> window lookup over the plan's table, by binary search per env as the device
  does it; `lookup_brute`: the same map by listing every window's root row.
* `nstep_target` / `init_reference`: the n-step target of a window's position 0 in f32, op by op, and q by the init
  rule over a whole host sink.
* `draws53`, `targets`, `sample_rows`, `live_rank_rows`: the sampler's draw, its targets and its rows, with the
  prefix in longdouble (per_reference.prefix).
"""
import numpy as np

import per_reference as PR
from oracle import rng

STREAM_ARCHIVE_PRIO = 7  # Philox stream of the row sampler's draws (csrc/archive_prio.hip)
TD_STEPS = 10


# ---------------------------------------------------------------------- the lookup
def plan_arrays(segs, B, K):
    """segs [(env, t0, L)] in (env, row) order -> (env, t0, L, woff i64[nseg], offs i64[B + 1]): the table's columns
    0, 1, 2, 5 and the segment column of the plan's exclusive scan over the envs."""
    env = np.array([s[0] for s in segs], np.int64).reshape(-1)
    t0 = np.array([s[1] for s in segs], np.int64).reshape(-1)
    L = np.array([s[2] for s in segs], np.int64).reshape(-1)
    woff = np.concatenate([[0], np.cumsum(L - K + 1)])[:-1].astype(np.int64)
    offs = np.concatenate([[0], np.cumsum(np.bincount(env, minlength=B))]).astype(np.int64)
    return env, t0, L, woff, offs


def lookup(segs, B, K, n_rows, rows):
    """Window whose root record is sink row i = t * B + b, or -1, for every i of `rows`."""
    env, t0, L, woff, offs = plan_arrays(segs, B, K)
    out = np.full(len(rows), -1, np.int64)
    for n, i in enumerate(np.asarray(rows, np.int64)):
        if i < 0 or i >= n_rows or len(segs) == 0:
            continue
        t, b = divmod(int(i), B)
        lo, hi = offs[b], offs[b + 1]
        if lo >= hi or t0[lo] > t:
            continue
        seg = lo + np.searchsorted(t0[lo:hi], t, side="right") - 1  # the last segment with t0 <= t
        s = t - t0[seg]
        if s <= L[seg] - K:
            out[n] = woff[seg] + s
    return out


def root_rows(segs, B, K):
    """Sink row of every window's root record, in archive window order."""
    return np.array([(t0 + s) * B + b for b, t0, L in segs for s in range(L - K + 1)], np.int64).reshape(-1)


def lookup_brute(segs, B, K, n_rows):
    """i64[n_rows]: the window of every row, -1 where the row is no root."""
    out = np.full(n_rows, -1, np.int64)
    r = root_rows(segs, B, K)
    out[r] = np.arange(len(r))
    return out


# ---------------------------------------------------------------------- the init rule
def nstep_target(reward, value, b, t0, cur, L, dpow, dpow_K):
    """replay_buffer.py:137-151 for record `cur` of the segment (b, t0, L), in f32, one operation at a time."""
    boot = cur + TD_STEPS
    if boot < L:
        v = np.float32(value[t0 + boot, b] * dpow_K)
        for k in range(boot - cur):
            v = np.float32(v + np.float32(dpow[k] * reward[t0 + cur + k, b]))
    else:
        v = np.float32(dpow[0] * reward[t0 + cur, b])
        for k in range(1, L - cur):
            v = np.float32(v + np.float32(dpow[k] * reward[t0 + cur + k, b]))
    return v


def init_reference(rec, segs, K, discount, eps, alpha):
    """q f64[T * B] by the init rule (per_reference.priority on the f32 |value - z|), 0 at every non-root, and the
    f32 targets z of the windows in archive order."""
    T, B = rec["reward"].shape
    dpow = np.array([discount ** k for k in range(T + 1)], np.float64).astype(np.float32)
    dpow_K = np.float32(np.float64(discount ** K))
    q = np.zeros(T * B, np.float64)
    zs = []
    for b, t0, L in segs:
        for s in range(L - K + 1):
            z = nstep_target(rec["reward"], rec["values"], b, t0, s, L, dpow, dpow_K)
            td = np.abs(np.float32(rec["values"][t0 + s, b] - z))
            q[(t0 + s) * B + b] = PR.priority(td, eps, alpha)
            zs.append(z)
    return q, np.array(zs, np.float32)


# ---------------------------------------------------------------------- the sampler
def draws53(n, step, seed):
    """u_j f64 = (x0 * 2^21 + (x1 >> 11)) * 2^-53 from the first two words of Philox (j, stream 7, step, 0)."""
    x0, x1, _, _ = rng.philox4x32(np.arange(n), STREAM_ARCHIVE_PRIO, step, 0, seed)
    return u_of_words(x0, x1)


def u_of_words(x0, x1):
    k = (np.asarray(x0).astype(np.uint64) << np.uint64(21)) + (np.asarray(x1).astype(np.uint64) >> np.uint64(11))
    return k.astype(np.float64) * 2.0 ** -53  # k < 2^53: both steps exact


def targets_f64(n, u, S):
    """t_j as the device forms it: (((double)j + u_j) / (double)n) * S, three f64 operations."""
    return ((np.arange(n, dtype=np.float64) + np.asarray(u, np.float64)) / np.float64(n)) * np.float64(S)


def sample_rows(q, n, u):
    """Rows of the n samples against the longdouble prefix (per_reference.sample's rule)."""
    C = PR.prefix(q)
    t = PR.targets(q, n, u)
    rows = np.searchsorted(C, t, side="right")
    last_live = int(np.nonzero(np.asarray(q) > 0)[0][-1])
    return np.where(rows >= len(q), last_live, rows).astype(np.int64)


def live_rank_rows(q, n, u):
    """For q in {0, 1}: every partial sum is an exact integer in f64 whatever the order, so sample j is exactly the
    floor(t_j)-th live row, t_j in the device's f64 operations (the last live row where rounding put t_j at S)."""
    q = np.asarray(q)
    assert set(np.unique(q)) <= {0.0, 1.0}
    live = np.flatnonzero(q > 0)
    t = targets_f64(n, u, len(live))
    return live[np.minimum(np.floor(t).astype(np.int64), len(live) - 1)]
