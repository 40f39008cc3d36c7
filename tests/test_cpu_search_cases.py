"""The synthetic search cases do what the GPU tests need them to (oracle alone, no GPU): the
peaked families reach path lengths well past the backup's batch of 8 edges, and the two-way
family draws tie-breaks among exactly 2 candidates. tests/test_gpu_search_deep.py compares the
tree kernels with these same oracle runs (cached in search_cases.run_oracle)."""
import numpy as np
import pytest

from oracle.mcts import ReplayModel
from search_cases import FAMILIES, PHILOX_SEED, RecordingOracle, make_case, run_oracle, search_cfg


@pytest.mark.parametrize("family", FAMILIES)
def test_case_generator_shapes_and_families(family):
    S, B = 6, 4
    c = make_case(family, S, B, seed=1)
    assert {k: v.shape for k, v in c.items()} == {"v_root": (B,), "pi_root": (B, 3), "noise": (B, 3), "r": (S, B),
                                                  "v": (S, B), "pi": (S, B, 3)}
    assert all(v.dtype == np.float32 for v in c.values())
    again = make_case(family, S, B, seed=1)
    assert all(np.array_equal(c[k], again[k]) for k in c)
    if family in ("peaked", "signed"):
        for p in (c["pi"].reshape(-1, 3), c["pi_root"]):
            np.testing.assert_array_equal(np.sort(p, axis=1), np.tile(np.float32([0.01, 0.01, 0.98]), (len(p), 1)))
        lo, hi, rs = (0, 2, {0, 1}) if family == "peaked" else (-300, 300, {-1, 0, 0.3, 6})
        assert (c["v"] >= lo).all() and (c["v"] <= hi).all()
        assert set(np.unique(c["r"])) <= set(np.float32(sorted(rs)))
        if family == "signed":
            assert (c["v"] < -10).any() and (c["v"] > 10).any()
    else:
        row = [0.5, 0.5, 0] if family == "two_way" else [1 / 3] * 3
        for p in (c["pi"].reshape(-1, 3), c["pi_root"], c["noise"]):
            assert (p == np.float32(row)).all()
        assert not c["r"].any() and not c["v"].any() and not c["v_root"].any()


def test_peaked_s64_b37_covers_every_path_length_to_24():
    o = run_oracle("peaked", 64, 37)
    d = o["depth"]
    print("peaked S=64 B=37: per-env max depth", d.max(0).min(), "to", d.max(0).max(), "ties", o["ties"])
    assert set(range(25)) <= set(np.unique(d))
    assert (d.max(0) >= 9).all()


@pytest.mark.parametrize("S,B", [(200, 13), (255, 5), (256, 5)])
def test_peaked_long_searches_reach_depth_25_in_every_env(S, B):
    o = run_oracle("peaked", S, B)
    d = o["depth"]
    print(f"peaked S={S} B={B}: per-env max depth", d.max(0).min(), "to", d.max(0).max(), "ties", o["ties"])
    assert (d.max(0) >= 25).all()


class _SkipsNinthEdge(RecordingOracle):
    """A backup that loses the first edge of its second batch of 8 (what a wrong batch step would do)."""

    def _backup(self, trees, last_nodes, trajectories, *rest):
        for t in trajectories:
            if len(t) >= 9:
                del t[len(t) - 9]
        super()._backup(trees, last_nodes, trajectories, *rest)


@pytest.mark.parametrize("S,B,visible", [(12, 40, False), (64, 37, True)])
def test_compared_outputs_see_a_backup_error_past_the_first_batch(S, B, visible):
    """The outputs the GPU tests compare (leaf actions, counts, values) change when the ninth edge of a path
    misses its update, and only where paths are that long: at S = 12 nothing can show."""
    o = run_oracle("peaked", S, B)
    c = o["case"]
    bad = _SkipsNinthEdge(search_cfg(S), ReplayModel(c["v_root"], c["pi_root"], c["r"], c["v"], c["pi"]), seed=PHILOX_SEED)
    values, counts = bad.search(np.zeros((B, 1), np.float32), c["noise"], 3, 0)
    leaf = np.array([[a for _, a in row] for row in bad.trace])
    same = [np.array_equal(leaf, o["leaf"]), np.array_equal(counts, o["counts"]),
            np.array_equal(values.view(np.uint32), o["values"].view(np.uint32))]
    assert (o["depth"].max() >= 9) == visible
    if visible:
        assert not any(same)
        assert (values.view(np.uint32) != o["values"].view(np.uint32)).all()  # every env's tree is deep enough
    else:
        assert all(same)


def test_two_way_draws_among_two_candidates():
    o = run_oracle("two_way", 64, 37)
    print("two_way S=64 B=37: ties", o["ties"], "max depth", o["depth"].max())
    assert o["ties"].get(2, 0) >= 100


def test_uniform_zero_ties_at_visited_nodes_too():
    S, B = 64, 37
    o = run_oracle("uniform_zero", S, B)
    print("uniform_zero S=64 B=37: ties", o["ties"], "max depth", o["depth"].max())
    # a fresh node's first selection is a 3-way tie whatever the inputs, once per node at the most; more
    # 3-way draws than nodes means equally visited nodes (1, 1, 1) tie too, besides the 2-way draws
    assert o["ties"].get(3, 0) > (S + 1) * B and o["ties"].get(2, 0) >= 100
