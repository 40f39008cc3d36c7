"""TEST INFRASTRUCTURE ONLY: prioritized replay restated in numpy from its formulae (MuZero, Appendix G).

    P(i) = q_i / S,  q_i = p_i ** alpha,  p_i = |nu_i - z_i| + eps,  S = sum q
    sample j of n:  u_j in [0, 1),  t_j = ((j + u_j) / n) S,  slot i with C[i-1] <= t_j < C[i]  (C: inclusive prefix sum)
    weight_j = (N P(i_j)) ** -beta / max_k (N P(i_k)) ** -beta

Prefix sums are taken in np.longdouble; u_j is the project's keyed Philox draw (oracle.rng.uniform(j, 4, step, 0,
seed)) unless given. Nothing here calls the library.
"""
import numpy as np

from oracle import rng

STREAM_REPLAY = 4


def draws(n, step, seed):
    """u_j f32 of the n samples of one call."""
    return rng.uniform(np.arange(n), STREAM_REPLAY, step, 0, seed)


def prefix(q):
    """Inclusive prefix sum of q (any float array) in longdouble."""
    return np.cumsum(np.asarray(q, dtype=np.longdouble))


def targets(q, n, u):
    """t_j in longdouble."""
    S = prefix(q)[-1]
    return (np.arange(n, dtype=np.longdouble) + np.asarray(u, dtype=np.longdouble)) / np.longdouble(n) * S


def sample(q, n, beta, n_live, step=0, seed=0, u=None):
    """-> slots i64[n], prob f64[n], weight f64[n]. A slot with q == 0 is never returned; a target at or beyond S
    gives the last slot with q > 0."""
    q = np.asarray(q)
    if u is None:
        u = draws(n, step, seed)
    C = prefix(q)
    S = C[-1]
    if not S > 0:
        raise ValueError("sample from an empty buffer")
    t = targets(q, n, u)
    slots = np.searchsorted(C, t, side="right")  # first i with C[i] > t: C[i] > C[i-1], so q[i] > 0
    last_live = int(np.nonzero(q > 0)[0][-1])
    slots = np.where(slots >= len(q), last_live, slots).astype(np.int64)
    prob = (q[slots].astype(np.longdouble) / S).astype(np.float64)
    raw = (np.float64(n_live) * prob) ** (-np.float64(beta))
    return slots, prob, raw / raw.max()


def priority(td, eps, alpha):
    """q = (td + eps) ** alpha in f64 (td, eps: the f32 values the kernels see)."""
    return (np.asarray(td, np.float64) + np.float64(np.float32(eps))) ** np.float64(np.float32(alpha))
