"""The tree kernels on deep trees, against the oracle, bit for bit.

The recorded-search fixtures and every random-init net keep a tree within 6 levels; the backup reads
the path in batches of 8 edges, so its second batch and the clamped prefetch of a partial batch first
run at path length 9. The synthetic cases of tests/search_cases.py (conditions asserted on the oracle
alone in test_cpu_search_cases.py) walk paths of every length up to 24 and well beyond, tie exactly
two ways, search with one simulation, spill into a second thread block and run with a non-zero
env_offset. The fused tree step is compared with the separate kernels on nets whose value head is
biased so that visited branches dominate, and the tree height is read back from the node pool.
"""
import numpy as np
import pytest
import torch

from search_cases import PHILOX_SEED, run_oracle, search_cfg
from mzba.config import default_config
from mzba.weights import init_state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def _compare(family, S, B, search_id=3, env_offset=0):
    from mzba.search import replay_search
    o = run_oracle(family, S, B, search_id=search_id, env_offset=env_offset)
    c = o["case"]
    values, counts, leaf = replay_search(B, S, search_cfg(S), c["v_root"], c["pi_root"], c["noise"], c["r"], c["v"],
                                         c["pi"], PHILOX_SEED, search_id, env_offset=env_offset)
    print(f"{family} S={S} B={B} env_offset={env_offset}: oracle max depth {o['depth'].max()}, per env "
          f"{o['depth'].max(0).min()}..{o['depth'].max(0).max()}, tie-breaks by candidates {o['ties']}")
    np.testing.assert_array_equal(leaf, o["leaf"])
    np.testing.assert_array_equal(counts, o["counts"])
    np.testing.assert_array_equal(values.view(np.uint32), o["values"].view(np.uint32))
    return o


@pytest.mark.parametrize("family", ["peaked", "two_way", "uniform_zero", "signed"])
def test_tree_kernels_match_oracle_s64(family):
    o = _compare(family, 64, 37)
    if family == "peaked":
        assert (o["depth"].max(0) >= 9).all()  # every env runs the backup's second batch
    if family == "signed":
        assert o["depth"].max() >= 17  # a third batch somewhere, with negative Q on the way
    if family == "two_way":
        assert o["ties"].get(2, 0) >= 100


@pytest.mark.parametrize("S,B", [(200, 13), (255, 5), (256, 5)])
def test_tree_kernels_match_oracle_long_searches(S, B):
    o = _compare("peaked", S, B)
    assert (o["depth"].max(0) >= 25).all()


@pytest.mark.parametrize("S", [1, 2, 3])
def test_tree_kernels_match_oracle_shortest_searches(S):
    _compare("peaked", S, 5)  # S = 1: no select launch at all


def test_tree_kernels_match_oracle_second_thread_block():
    _compare("peaked", 12, 257)  # 256 threads per block: env 256 alone in the second


def test_tree_kernels_match_oracle_env_offset_and_search_id():
    o = _compare("peaked", 64, 37, search_id=1000003, env_offset=4059)
    base = run_oracle("peaked", 64, 37)
    assert not np.array_equal(o["leaf"], base["leaf"])  # the offset and id reach the tie-break stream


def test_select_depth_matches_oracle_path_lengths_per_sim():
    """TreeState.depth after every select == the oracle's path length of that (sim, env): the backup's
    batch loop gets the inputs the oracle's gets, not only the same final counts."""
    from mzba.search import TreeState
    S, B = 64, 37
    o = run_oracle("peaked", S, B)
    c, cfg = o["case"], search_cfg(S)
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a), device="cuda")  # noqa: E731
    t = TreeState(B, S, cfg["search"]["c1"], cfg["search"]["c2"], "cuda")
    ta = t.args(0, 3, PHILOX_SEED)
    t.root(ta, dv(c["v_root"]), dv(c["pi_root"]), dv(c["noise"]), float(np.float32(1 - 0.175)), float(np.float32(0.175)), 0.25)
    gamma = float(np.float32(cfg["search"]["discount_factor"]))
    depth = np.zeros((S, B), dtype=np.int64)
    leaf = np.zeros((S, B), dtype=np.int64)
    for sim in range(S):
        if sim > 0:
            t.select(ta, sim)
        depth[sim] = t.depth.cpu().numpy()
        leaf[sim] = t.leaf_action.cpu().numpy()
        t.backup(ta, sim, dv(c["r"][sim]), dv(c["v"][sim]), dv(c["pi"][sim]), gamma)
    np.testing.assert_array_equal(depth, o["depth"])
    np.testing.assert_array_equal(leaf, o["leaf"])
    assert set(range(25)) <= set(np.unique(depth))


def _tree_heights(nodes, B, S):
    """Longest root-to-node path (edges) of each env's tree, from the node pool's child links (words 12 to
    14 of a 64-byte node). A child's slot is always larger than its parent's, so one backward sweep does."""
    n = nodes.view(torch.int32).view(B, S + 1, 16).cpu().numpy()
    child = n[:, :, 12:15]
    h = np.zeros((B, S + 1), dtype=np.int64)
    for b in range(B):
        for i in range(S, -1, -1):
            for c in child[b, i]:
                if c >= 0:
                    assert i < c <= S
                    h[b, i] = max(h[b, i], 1 + h[b, c])
    return h[:, 0]


VALUE_BIN, VALUE_BUMP = 8, 6.0  # support +3 of the 11 bins over [-5, 5]


@pytest.mark.parametrize("variant,S", [(2, 255), (2, 256), (4, 255), (4, 256), (3, 64), (1, 64)])
def test_tree_step_fused_into_prediction_is_identical_on_deep_trees(variant, S):
    """backup(sim) + select(sim + 1) inside the fused prediction launch == the separate tree kernels, bit
    for bit (bf16 nets), on trees at least 25 levels high: the prediction value head's bias is raised at
    one positive support bin, so every node's value is positive and visited branches dominate. S = 255
    fills the fused step's LDS copy of the two ucb tables to its last float, S = 256 falls back to the
    global tables; variant 3 reads the global tables at any S."""
    from mzba import _lib as L
    from mzba.agent import MuZeroAgent
    from mzba.search import MCTSSearchVec
    cfg = default_config()
    cfg["num_simulations"] = S
    mcfg = cfg["model"]
    sd = init_state_dict(mcfg, 4)
    sd["pred_net.value_head.2.bias"][VALUE_BIN] += VALUE_BUMP
    ag = MuZeroAgent(mcfg, dtype="bf16")
    ag.load_state_dict(sd)
    B = 13
    g = torch.Generator().manual_seed(5)
    h = torch.rand(B, 256, 4, 5, generator=g).cuda()
    out = []
    L.call("mzba_tower_set_variant", variant)
    try:
        for fuse in (False, True):
            ag._runners = {}
            s = MCTSSearchVec(cfg, ag, None, seed=17)
            ws = s.workspace(B)
            ws.use_tree_fusion = fuse
            assert ws.runner.fused_ok() and ws.runner.tower_plan == variant
            v, c = s.search(h)
            out.append((v.numpy(), c.numpy(), _tree_heights(ws.tree.nodes, B, S), ws.tree.nodes.cpu().numpy()))
    finally:
        L.call("mzba_tower_set_variant", 0)
    print(f"variant {variant} S={S}: tree height per env, unfused {out[0][2].tolist()}, fused {out[1][2].tolist()}")
    assert (out[0][2] >= 25).all() and (out[1][2] >= 25).all()
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    np.testing.assert_array_equal(out[0][3], out[1][3])  # the whole node pool: Q, P, R, N, child links
