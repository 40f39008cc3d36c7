"""Seeded synthetic net outputs for the tree kernels, and the oracle run that goes with them.

`make_case` builds the recorded outputs `oracle.mcts.ReplayModel` and `mzba.search.replay_search`
take (v_root[B], pi_root[B,3], noise[B,3], r[S,B], v[S,B], pi[S,B,3], all f32). The families are
chosen to reach what random-init nets never do: peaked priors with positive values grow chains
dozens of levels deep (the backup's batched path reads), exact two-way ties, all-tie searches and
large signed returns. `run_oracle` runs `MCTSOracle` on a case and also records, per (sim, env),
the selected leaf action and the path length, and how often the tie-break drew among n candidates.
Results are cached per argument tuple, so the CPU conditions and the GPU comparisons share one run.
"""
import functools

import numpy as np

from oracle import mcts as M
from mzba.config import default_config

FAMILIES = ("peaked", "two_way", "uniform_zero", "signed")
PHILOX_SEED = 17  # the keyed tie-break stream's seed, both sides


def _peaked(g, shape, peak):
    """One random action per row with prior `peak`, the other two (1 - peak) / 2."""
    pi = np.full(shape + (3,), (1.0 - peak) / 2.0, dtype=np.float64)
    a = g.integers(0, 3, shape)
    np.put_along_axis(pi, a[..., None], peak, axis=-1)
    return pi.astype(np.float32)


def make_case(family, S, B, seed=0, peak=0.98):
    g = np.random.default_rng(seed)
    f32 = np.float32
    if family in ("peaked", "signed"):
        pi_root = _peaked(g, (B,), peak)
        noise = g.dirichlet([0.25] * 3, B).astype(f32)
        pi = _peaked(g, (S, B), peak)
        if family == "peaked":
            v_root = g.uniform(0.0, 2.0, B).astype(f32)
            v = g.uniform(0.0, 2.0, (S, B)).astype(f32)
            r = g.choice(np.array([0, 0, 0, 1], f32), (S, B))
        else:
            v_root = g.uniform(-300.0, 300.0, B).astype(f32)
            v = g.uniform(-300.0, 300.0, (S, B)).astype(f32)
            r = g.choice(np.array([-1, 0, 0.3, 6], f32), (S, B))
    elif family in ("two_way", "uniform_zero"):
        row = np.array([0.5, 0.5, 0.0] if family == "two_way" else [1 / 3] * 3, f32)
        pi_root = np.tile(row, (B, 1))
        noise = pi_root.copy()
        pi = np.tile(row, (S, B, 1))
        v_root = np.zeros(B, f32)
        v = np.zeros((S, B), f32)
        r = np.zeros((S, B), f32)
    else:
        raise ValueError(family)
    case = dict(v_root=v_root, pi_root=pi_root, noise=noise, r=r.astype(f32), v=v, pi=pi)
    assert all(x.dtype == np.float32 for x in case.values())
    return case


class _CountingRng:
    """oracle.rng with randbelow's calls counted by their n."""

    def __init__(self, rng, ties):
        self._rng, self._ties = rng, ties

    def __getattr__(self, name):
        return getattr(self._rng, name)

    def randbelow(self, env, stream, step, call, seed, n):
        self._ties[int(n)] = self._ties.get(int(n), 0) + 1
        return self._rng.randbelow(env, stream, step, call, seed, n)


class RecordingOracle(M.MCTSOracle):
    """MCTSOracle that records each (sim, env) path length on entry to `_backup` (`depths`), the
    leaf actions (`leaf`) and the tie-break calls by candidate count (`ties`)."""

    def __init__(self, cfg, model, seed=0):
        super().__init__(cfg, model, seed)
        self.depths, self.ties = [], {}
        self.trace = []

    def _backup(self, trees, last_nodes, trajectories, *rest):
        self.depths.append([len(t) for t in trajectories])
        super()._backup(trees, last_nodes, trajectories, *rest)

    def search(self, *args, **kw):
        rng = M.R
        M.R = _CountingRng(rng, self.ties)
        try:
            return super().search(*args, **kw)
        finally:
            M.R = rng


def search_cfg(S):
    cfg = default_config()
    cfg["num_simulations"] = S
    return cfg


@functools.lru_cache(maxsize=None)
def run_oracle(family, S, B, seed=0, peak=0.98, search_id=3, env_offset=0):
    """-> dict(case, values f32[B], counts i64[B,3], leaf i64[S,B], depth i64[S,B], ties {n: calls}).
    Treat the arrays as read-only: the result is shared between tests."""
    case = make_case(family, S, B, seed, peak)
    model = M.ReplayModel(case["v_root"], case["pi_root"], case["r"], case["v"], case["pi"])
    o = RecordingOracle(search_cfg(S), model, seed=PHILOX_SEED)
    values, counts = o.search(np.zeros((B, 1), np.float32), case["noise"], search_id, env_offset)
    out = dict(case=case, values=values, counts=counts,
               leaf=np.array([[a for _, a in row] for row in o.trace], dtype=np.int64),
               depth=np.array(o.depths, dtype=np.int64), ties=dict(o.ties))
    for k in ("values", "counts", "leaf", "depth"):
        out[k].setflags(write=False)
    return out
