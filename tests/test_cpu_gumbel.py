"""The Gumbel search's definition without a GPU: the visit schedule, the oracle's structure, the
fixed-point packing, and the calibration of the GPU test's comparison (tests/test_gpu_gumbel.py): the f32 restatement
makes the f64 statement's decisions on every unambiguous case of the committed case set, and few cases are ambiguous."""
import ctypes

import numpy as np
import pytest

import gumbel_cases as G


def test_schedule_known_values():
    from mzba.search import gumbel_schedule
    for fn in (G.schedule, gumbel_schedule):
        assert fn(8, 3) == [0, 0, 0, 1, 1, 2, 2, 3]
        assert fn(8, 2) == [0, 0, 1, 1, 2, 2, 3, 3]
        assert fn(4, 3) == [0, 0, 0, 1]
        assert fn(4, 2) == [0, 0, 1, 1]
        assert fn(16, 3)[:12] == [0, 0, 0, 1, 1, 1, 2, 2, 3, 3, 4, 4]
        assert fn(50, 3)[:12] == [0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3]
        for S in (1, 2, 4, 8, 16, 50):
            for m in (2, 3):
                assert len(fn(S, m)) == S and fn(S, m) == G.schedule(S, m)


def _visit_multiset(S, m):
    """Root visit counts the schedule implies, whichever eligible action each simulation takes."""
    n = [0] * m
    for want in G.schedule(S, m):
        n[n.index(want)] += 1
    return sorted(n)


@pytest.mark.parametrize("i", range(len(G.CASE_SETS)))
def test_root_visits_follow_the_schedule(i):
    """Root sum N == S, the considered actions' counts are the schedule's per-phase pattern, an action outside the
    considered set is never visited, and the eligibility assertion of the oracle never fires (it would raise)."""
    B, S, m, _, _ = G.CASE_SETS[i]
    _, o = G.oracle(i)
    assert (o["root_n"].sum(1) == S).all()
    want = _visit_multiset(S, m)
    for b in range(B):
        cons = [a for a in range(3) if (o["considered"][b] >> a) & 1]
        assert len(cons) == m
        assert sorted(o["root_n"][b][cons]) == want
        assert o["root_n"][b].sum() == o["root_n"][b][cons].sum()
        # simulation s's leaf at the root is a considered action, and the first m simulations take each one once
        roots = [o["leaf_action"][s, b] for s in range(S) if o["leaf_parent"][s, b] == 0]
        assert set(roots) <= set(cons)
    assert (o["leaf_parent"][0] == 0).all()


def test_packing_rows_sum_to_2_24():
    for i in range(len(G.CASE_SETS)):
        _, o = G.oracle(i)
        assert (np.abs(o["counts"].sum(1) - (1 << 24)) <= 2).all()
        assert (o["counts"] >= 0).all()
        np.testing.assert_allclose(o["counts"] / G.Q24, o["pi"], atol=2.0 ** -25, rtol=0)


def test_one_level_bandit_picks_argmax_of_g_l_sigma():
    """S = 3, m = 3: every action is visited once, each Q is exactly its (r + gamma v) return, and the chosen action is
    the argmax of g + l + sigma(q) computed here from those exact Q."""
    rng = np.random.default_rng(5)
    gamma = float(np.float32(G.GAMMA))
    for _ in range(50):
        c = G.gen_cases(1, 3, int(rng.integers(1 << 30)))
        o = G.search_one(c["v_root"][0], c["pi_root"][0], c["z"][0], c["r"][:, 0], c["v"][:, 0], c["pi"][:, 0], 3, 3)
        assert o["root_n"] == [1, 1, 1] and [p for p, _ in o["leaves"]] == [0, 0, 0]
        q = np.zeros(3)
        for s, (_, a) in enumerate(o["leaves"]):
            q[a] = float(c["v"][s, 0]) * gamma + float(c["r"][s, 0])
        sigma = (50.0 + 1.0) * 1.0 * (q - q.min()) / max(q.max() - q.min(), 1e-8)
        score = c["z"][0].astype(np.float64) + np.log(c["pi_root"][0].astype(np.float64)) + sigma
        assert o["action"] == int(np.argmax(score))
        e = np.exp(np.log(c["pi_root"][0].astype(np.float64)) + sigma - (np.log(c["pi_root"][0]) + sigma).max())
        np.testing.assert_allclose(o["pi"], e / e.sum(), rtol=1e-12)


def test_scale_zero_ignores_the_variates():
    c = G.gen_cases(8, 8, 77)
    a = G.run_cases(c, 8, 3, scale=0.0)
    c2 = dict(c, z=c["z"][::-1].copy())
    b = G.run_cases(c2, 8, 3, scale=0.0)
    for k in ("leaf_parent", "leaf_action", "root_n", "action", "counts"):
        np.testing.assert_array_equal(a[k], b[k])


def test_ambiguity_cap_and_f32_decisions():
    """A case is ambiguous when its smallest f64 argmax margin is below 1e-3. Scores reach about (c_visit + S) c_scale
    ~ 100, so an f32 operation errs by about 6e-6 and a 1e-3 margin is about 50 times that. Cap: at most 5 % of the
    committed cases with S <= 16 and 10 % of those with S = 50 are ambiguous; on every other case the f32 restatement
    makes the f64 decisions, and its pi' / value stay within 1e-4 on all cases (the GPU test's tolerance)."""
    assert G.ambiguous_share(G.SMALL_S) <= 0.05
    assert G.ambiguous_share(G.LARGE_S) <= 0.10
    worst = 0.0
    for i in range(len(G.CASE_SETS)):
        _, o64 = G.oracle(i)
        _, o32 = G.oracle(i, True)
        ok = o64["margin"] >= G.AMBIGUOUS
        for k in ("leaf_parent", "leaf_action"):
            np.testing.assert_array_equal(o32[k][:, ok], o64[k][:, ok], err_msg=f"set {i} {k}")
        for k in ("root_n", "action", "considered"):
            np.testing.assert_array_equal(o32[k][ok], o64[k][ok], err_msg=f"set {i} {k}")
        worst = max(worst, np.abs(o32["pi"] - o64["pi"]).max(),
                    (np.abs(o32["value"] - o64["value"]) / np.maximum(1, np.abs(o64["value"]))).max())
    print("largest f32 error in pi' / value:", worst)
    assert worst <= 1e-4


def test_gumbel_abi_without_gpu():
    """The mode's struct mirror has the library's size, and the entry points reject a NULL struct, B <= 0 and m
    outside {2, 3} before any HIP call."""
    from mzba import _lib
    L = _lib.lib()
    assert L.mzba_struct_bytes(b"mzba_gumbel") == ctypes.sizeof(_lib.Gumbel)
    a = 4096
    p = ctypes.c_void_p(a)

    def ts(B=3, S=4, sim=0):
        return ctypes.byref(_lib.TreeStep(*[a] * 9, B, S, 0, 0, 1, None, sim, 0.985, a))

    def gm(m=3):
        return ctypes.byref(_lib.Gumbel(a, a, a, m, 50.0, 1.0, 1.0))

    for t, g in ((None, gm()), (ts(), None), (ts(B=0), gm()), (ts(), gm(1)), (ts(), gm(4)), (ts(S=0), gm())):
        assert L.mzba_gumbel_root(t, g, p, p, None, None, None) == -1
        assert L.mzba_gumbel_step(t, g, p, p, None) == -1
        assert L.mzba_gumbel_results(t, g, p, p, p, None, None) == -1
    assert L.mzba_gumbel_step(ts(sim=4), gm(), p, p, None) == -1
    assert L.mzba_gumbel_step(ts(sim=-1), gm(), p, p, None) == -1
    assert L.mzba_gumbel_root(ts(), gm(), None, p, None, None, None) == -1
    assert L.mzba_gumbel_results(ts(), gm(), p, p, None, None, None) == -1


def test_search_config_selects_the_mode():
    from mzba.config import default_config
    from mzba.search import gumbel_params, search_kind
    cfg = default_config()
    assert search_kind(cfg) == "puct"
    cfg["search"]["kind"] = "gumbel"
    assert search_kind(cfg) == "gumbel" and gumbel_params(cfg) == (3, 50.0, 1.0, 1.0)
    cfg["search"]["gumbel"] = {"max_considered": 2, "c_visit": 20, "c_scale": 0.5, "scale": 0.0}
    assert gumbel_params(cfg) == (2, 20.0, 0.5, 0.0)
    cfg["search"]["gumbel"]["max_considered"] = 4
    with pytest.raises(ValueError):
        gumbel_params(cfg)
    cfg["search"]["kind"] = "alphazero"
    with pytest.raises(ValueError):
        search_kind(cfg)
