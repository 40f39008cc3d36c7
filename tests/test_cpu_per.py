"""The prioritized-replay reference sampler (tests/per_reference.py) on its own: the properties the device sampler
is then held to (tests/test_gpu_per.py), checked on the numpy restatement itself."""
import numpy as np

import per_reference as R


def _priorities(cap, seed, dead=0.0):
    g = np.random.default_rng(seed)
    q = np.exp(g.uniform(np.log(1e-3), np.log(1e3), cap)).astype(np.float32)
    if dead:
        q[g.random(cap) < dead] = 0.0
    return q


def test_reference_never_returns_a_dead_slot():
    for cap, n in [(1, 1), (63, 7), (1025, 512), (3000, 512)]:
        q = _priorities(cap, cap, dead=0.4 if cap > 1 else 0.0)
        q[:3] = 0.0 if cap > 8 else q[:3]
        q[-5:] = 0.0 if cap > 8 else q[-5:]
        for u in (None, np.zeros(n, np.float32), np.full(n, 1 - 2.0 ** -24, np.float32)):
            slots, prob, w = R.sample(q, n, 1.0, int((q > 0).sum()), step=3, seed=9, u=u)
            assert (q[slots] > 0).all()
            assert ((w > 0) & (w <= 1)).all() and w.max() == 1.0
            assert np.allclose(prob, q[slots].astype(np.float64) / q.astype(np.float64).sum(), rtol=1e-12)


def test_reference_targets_lie_in_their_strata():
    cap, n = 257, 64
    q = _priorities(cap, 5)
    C = R.prefix(q)
    S = C[-1]
    for step in range(4):
        u = R.draws(n, step, 11)
        assert u.dtype == np.float32 and ((u >= 0) & (u < 1)).all()
        t = R.targets(q, n, u)
        j = np.arange(n, dtype=np.longdouble)
        assert (t >= j / n * S).all() and (t < (j + 1) / n * S).all()
        slots, _, _ = R.sample(q, n, 0.5, cap, step=step, seed=11)
        lo = np.where(slots > 0, C[slots - 1], 0)
        assert (lo <= t).all() and (t < C[slots]).all()


def test_reference_frequencies_follow_the_priorities():
    """200 000 draws at cap = 257: each slot's count within 5 binomial standard deviations of N q_i / S.

    The priorities are log-uniform over one decade (0.3 ... 3), so the rarest slot still expects about 190 draws: a
    bound of 5 standard deviations presumes a count whose distribution is near normal, and a slot expecting 0.01
    draws (sd 0.1) would break it with its first, legitimate, hit. Stratification only lowers the variance."""
    cap, n, calls = 257, 500, 400
    q = np.exp(np.random.default_rng(7).uniform(np.log(0.3), np.log(3.0), cap)).astype(np.float32)
    p = q.astype(np.float64) / q.astype(np.float64).sum()
    counts = np.zeros(cap, np.int64)
    for step in range(calls):
        slots, _, _ = R.sample(q, n, 1.0, cap, step=step, seed=21)
        counts += np.bincount(slots, minlength=cap)
    N = n * calls
    assert N == 200000
    sd = np.sqrt(N * p * (1 - p))
    assert (np.abs(counts - N * p) <= 5 * sd).all(), np.abs((counts - N * p) / sd).max()


def test_reference_weights():
    q = _priorities(300, 8)
    slots, prob, w = R.sample(q, 32, 0.0, 300, step=1)
    assert (w == 1.0).all()
    slots, prob, w = R.sample(q, 32, 1.0, 300, step=1)
    assert np.allclose(w, prob.min() / prob, rtol=1e-12)
