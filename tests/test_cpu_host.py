"""CPU-only checks of the host side: C-ABI library loads and exports every symbol
declared in include/mzba.h (no compute without a GPU), weight packing/spec logic."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mzba.config import default_config, small_model_cfg
from mzba.weights import init_state_dict, state_dict_spec


def _declared():
    h = open(os.path.join(ROOT, "include", "mzba.h")).read()
    return sorted(set(re.findall(r"\b(mzba_[a-z0-9_]+)\s*\(", h)))


def test_library_exports_every_declared_symbol():
    from mzba import _lib
    L = _lib.lib()
    decl = _declared()
    assert decl, "no declarations parsed"
    for name in decl:
        assert hasattr(L, name), name
    assert sorted(_lib.exported_symbols()) == decl


_CTYPE = {"int": "I", "long long": "LL", "int64_t": "LL", "uint64_t": "U64", "uint32_t": "U32", "float": "F",
          "double": "D"}


def _prototypes():
    """{name: (return type, [parameter type, ...])} of every mzba_* function declared in include/mzba.h."""
    h = open(os.path.join(ROOT, "include", "mzba.h")).read()
    h = re.sub(r"/\*.*?\*/", " ", h, flags=re.S)
    h = re.sub(r"//[^\n]*|^\s*#[^\n]*", " ", h, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w ]*?)\s*\b(mzba_\w+)\s*\(([^()]*)\)\s*;", h):
        assert name not in out, name
        params = [" ".join(p.split()) for p in params.split(",")]
        out[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return out


def _param_code(p):
    if "*" in p or p.startswith("hipStream_t "):
        return "P"
    ctype = p.rsplit(" ", 1)[0]  # without the parameter's name
    assert ctype in _CTYPE, f"parameter type the table's check does not know: {p!r}"
    return _CTYPE[ctype]


def test_signature_table_matches_header_types():
    """Every prototype of include/mzba.h against _lib.SIGNATURES, parameter by parameter (pointers and the stream are
    P), and the non-int return types against _lib.RESTYPES: the table ctypes converts by is the header's."""
    from mzba import _lib
    protos = _prototypes()
    assert sorted(protos) == _declared()
    for name, (ret, params) in protos.items():
        got = [getattr(_lib, _param_code(p)) for p in params]
        assert got == _lib.SIGNATURES[name], (name, params)
        assert _lib.RESTYPES.get(name, _lib.I) is getattr(_lib, _CTYPE[ret]), (name, ret)
    assert set(_lib.RESTYPES) <= set(protos)


def test_struct_sizes_match_the_library():
    import ctypes
    from mzba import _lib
    L = _lib.lib()
    assert sorted(_lib.STRUCTS) == ["mzba_env_state", "mzba_replay_ring", "mzba_sink", "mzba_tower_ext",
                                    "mzba_tree_step"]
    for name, cls in _lib.STRUCTS.items():
        assert L.mzba_struct_bytes(name.encode()) == ctypes.sizeof(cls), name
    assert L.mzba_struct_bytes(b"mzba_guard") == -1
    assert L.mzba_struct_bytes(None) == -1


def test_env_and_replay_entry_points_reject_bad_arguments_without_gpu():
    """The entry points that take the env state, the sink and the ring check them before any HIP call: a NULL
    required struct and an empty batch (B = 0) return -1; the streamed plan keeps its -2 for a short table."""
    from ctypes import byref, c_void_p
    from mzba import _lib
    L = _lib.lib()
    p = c_void_p(4096)
    a = 4096

    def env(B=3):
        return byref(_lib.EnvState(*[a] * 7, 1, *[a] * 5, 4, B, 16, 20, 6, 3))

    def sink(B=3, T=8):
        return byref(_lib.Sink(*[a] * 7, T, B, 320))

    ring = byref(_lib.ReplayRing(*[a] * 8, 64, 5, 4))
    r4 = (_lib.F * 4)(1, 1, -1, 1)
    calls = {
        "mzba_env_reset_compact": lambda e, s, g: (e, 0, 0, 0, None, 0, None),
        "mzba_env_restart_compact": lambda e, s, g: (e, p, p, p, 0, 0, None, 0, None),
        "mzba_env_step_compact": lambda e, s, g: (e, p, p, p, None, 1, r4, None, 0, None),
        "mzba_compact_to_planes": lambda e, s, g: (e, p, None),
        "mzba_build_rep_input": lambda e, s, g: (e, p, 1, 64, None),
        "mzba_env_current_frame": lambda e, s, g: (e, p, None),
        "mzba_replay_plan": lambda e, s, g: (s, p, 5, 6, p, p, p, None),
        "mzba_replay_write": lambda e, s, g: (s, p, p, p, p, 4, g, 0, p, None),
        "mzba_replay_stream_plan": lambda e, s, g: (s, p, p, 5, 6, 261, 0, p, p, p, 64, None),
        "mzba_replay_stream_write": lambda e, s, g: (s, 16, 20, 6, 3, p, 64, 1, 4, g, 0, p, None),
    }
    for name, args in calls.items():
        fn = getattr(L, name)
        assert fn(*args(None, None, ring)) == -1, name                 # the NULL env state / sink
        assert fn(*args(env(B=0), sink(B=0), ring)) == -1, name        # B = 0
    for name in ("mzba_replay_write", "mzba_replay_stream_write"):
        assert getattr(L, name)(*calls[name](None, sink(), None)) == -1, name  # the NULL ring
    assert L.mzba_record_results(p, p, None, 0, None, None) == -1
    assert L.mzba_record_results(p, p, sink(B=0), 0, None, None) == -1
    # nmax below B * (T / keep): T = 8, keep = max(min_len + 1, K) = 4 -> 3 * 2 = 6 table rows at least
    plan = lambda nmax: L.mzba_replay_stream_plan(sink(), p, p, 4, 3, 261, 0, p, p, p, nmax, None)  # noqa: E731
    assert plan(5) == -2
    assert plan(-1) == -2


def test_tree_entry_points_reject_bad_arguments_without_gpu():
    """The four PUCT entry points check their mzba_tree_step before any HIP call: a NULL struct, B = 0, S = 0 and a
    NULL nodes return -1, and so do a simulation outside the entry point's range and a backup without rewards."""
    from ctypes import byref, c_void_p
    from mzba import _lib
    L = _lib.lib()
    a = 4096
    p = c_void_p(a)

    def ts(B=3, S=4, sim=1, nodes=a, r=a):
        return byref(_lib.TreeStep(nodes, *[a] * 8, B, S, 0, 0, 1, None, sim, 0.985, r))

    calls = {
        "mzba_mcts_root": lambda t: (t, p, p, None, p, 0.825, 0.175, None, 0.25, None),
        "mzba_mcts_select": lambda t: (t, None),
        "mzba_mcts_backup": lambda t: (t, p, p, None),
        "mzba_mcts_results": lambda t: (t, p, p, None),
    }
    for name, args in calls.items():
        for t in (None, ts(B=0), ts(S=0), ts(nodes=None)):
            assert getattr(L, name)(*args(t)) == -1, name
    assert L.mzba_mcts_select(ts(sim=0), None) == -1
    assert L.mzba_mcts_select(ts(sim=4), None) == -1
    assert L.mzba_mcts_backup(ts(sim=4), p, p, None) == -1
    assert L.mzba_mcts_backup(ts(r=None), p, p, None) == -1


def test_node_layout_is_one_line():
    from mzba import _lib
    assert _lib.lib().mzba_mcts_node_bytes() == 64


def test_bad_arguments_rejected_without_gpu():
    from mzba import _lib
    import ctypes
    rc = _lib.lib().mzba_conv2d(1, None, 0, None, 0, None, None, None, None, 0, None, None, 0, 4, 5, 256, 256, 3,
                                1, None)
    assert rc < 0
    rc = _lib.lib().mzba_conv2d(1, None, 0, None, 0, None, None, None, None, 0, None, None, 2, 4, 5, 100, 256, 3,
                                1, None)
    assert rc == -2
    del ctypes


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from mzba.agent import MuZeroAgent
    with pytest.raises(RuntimeError):
        MuZeroAgent(default_config()["model"])


@pytest.mark.parametrize("small", [False, True])
def test_state_dict_spec_matches_reference_layout(small):
    cfg = default_config()
    m = small_model_cfg(cfg) if small else cfg["model"]
    spec = dict(state_dict_spec(m))
    c1 = m["latent_channels"][1]
    assert spec["dyn_net.conv_block.conv.weight"] == (c1, c1 + 3, 3, 3)
    assert spec["pred_net.value_head.2.weight"] == (11, c1 // 2 * 20)
    sd = init_state_dict(m, 0)
    assert len(sd) == len(spec)
    w = sd["rep_net.blocks.0.weight"]
    assert np.abs(w).max() <= 1 / np.sqrt(np.prod(w.shape[1:]))
    if not small:
        n = sum(int(np.prod(s)) for k, s in spec.items() if not k.endswith("num_batches_tracked"))
        assert n > 40_000_000  # rep 8.05M + dyn 17.26M + pred 16.90M


def test_ucb_tables_double_precision():
    import math
    import torch
    from mzba.search import ucb_tables
    sq, ct = ucb_tables(50, 1.25, 19652.0, "cpu")
    for n in (0, 1, 7, 50):
        assert sq[n].item() == float(np.float32(math.sqrt(n)))
        assert ct[n].item() == float(np.float32(1.25 + math.log((n + 19652.0 + 1) / 19652.0)))
    del torch


def test_torch_custom_ops_registered():
    """libmzba_torch.so registers TORCH_LIBRARY(mz) with the drop-in surface of SURVEY §8(b);
    env_step declares the reference's done_mask aliasing (Tensor(a!) done -> Tensor(a!))."""
    from mzba import _lib
    ops = _lib.ops()
    for name in _lib.TORCH_OPS:
        assert hasattr(ops, name), name
    sch = str(ops.env_step.default._schema)
    assert "Tensor(a!) done" in sch and "Tensor(a!) done_out" in sch, sch
    assert "Tensor(h!) values" in str(ops.mcts_results_.default._schema)


def test_net_ops_schemas_declare_their_writes():
    """The nets as custom ops (csrc/net_ops.cpp): the reference surface takes the weight pack
    (mz.NetPack) and returns new tensors; the NHWC acting forms and the fused prediction + tree step
    declare every buffer they write as Tensor(x!) — the tree buffers of prediction_tree_ included —
    and nothing they only read."""
    import torch
    from mzba import _lib
    ops = _lib.ops()
    assert "__torch__.torch.classes.mz.NetPack nets" in str(ops.representation.default._schema)
    for name, writes, reads in (
            ("dynamics_", ["out", "r_dec", "r_logits", "pool"], ["src", "act", "slot"]),
            ("prediction_", ["pi", "v", "p_logits", "v_logits"], ["h"]),
            ("prediction_tree_", ["pi", "v", "nodes", "root_sum", "calls", "leaf_parent", "leaf_action", "depth",
                                  "path"], ["h", "sqrt_tab", "c_tab", "r", "ctx"]),
            ("representation_", ["out", "pool"], ["x"])):
        args = {a.name: a for a in getattr(ops, name).default._schema.arguments}
        for w in writes:
            assert args[w].alias_info is not None and args[w].alias_info.is_write, (name, w)
        for r in reads:
            assert args[r].alias_info is None, (name, r)
    p = torch.classes.mz.NetPack()
    p.set_int("k", 7)
    assert p.get_int("k") == 7 and not p.fused_ok()


def test_default_checkpoint_optimizer_state_loads_into_reference_adam():
    """Without a learner, save_checkpoint writes a fresh Adam state that the reference's
    `optimizer.load_state_dict` (train_torch.py:646) accepts: one group, every parameter."""
    import torch
    from mzba.checkpoint import fresh_optimizer_state
    from mzba.config import default_config
    from mzba.weights import state_dict_spec
    mcfg = default_config()["model"]
    params = [torch.nn.Parameter(torch.zeros(1)) for k, _ in state_dict_spec(mcfg)
              if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]
    opt = torch.optim.Adam(params, lr=mcfg["learning_rate"], weight_decay=1e-4)
    opt.load_state_dict(fresh_optimizer_state(mcfg))
    assert opt.param_groups[0]["weight_decay"] == 1e-4 and len(opt.param_groups[0]["params"]) == len(params)


def test_scale_division_by_double_reciprocal_is_ieee():
    """towerp.hip's _scale_state divides (h - min) by den = (max - min) + 1e-8 as
    f32((double)(h - min) * f64(1 / den)); that must be the IEEE f32 quotient bit for bit (the
    product is within 2^-52 of the exact quotient, a quotient of two f32 at least 2^-49 from a
    rounding midpoint). Checked on 4M random pairs over the ranges the scale sees plus edge pairs."""
    rng = np.random.default_rng(3)
    a = np.concatenate([rng.random(2_000_000, dtype=np.float32) * np.float32(37.0),
                        rng.random(2_000_000, dtype=np.float32) * np.float32(1e-3),
                        np.array([0.0, 1.0, 3.0, 1e-8, 65504.0], np.float32)])
    d = np.concatenate([rng.random(2_000_000, dtype=np.float32) * np.float32(37.0) + np.float32(1e-8),
                        rng.random(2_000_000, dtype=np.float32) * np.float32(1e-3) + np.float32(1e-8),
                        np.array([1e-8, 3.0, 3.0, 7.0, 3.0], np.float32)]).astype(np.float32)
    q_ieee = a / d
    q_dbl = (a.astype(np.float64) * (1.0 / d.astype(np.float64))).astype(np.float32)
    np.testing.assert_array_equal(q_ieee.view(np.uint32), q_dbl.view(np.uint32))


def test_rep_trunk_rejects_bad_arguments_without_gpu():
    """mzba_rep_trunk checks its arguments before any HIP call: null buffers or pointer tables, negative
    block counts, more convs than its kernel-argument tables hold (2 n0 + 2 + 2 n1 <= 56), in == out."""
    import ctypes
    from mzba import _lib
    L = _lib.lib()
    nc = 2 * 2 + 2 + 2 * 3
    w = (ctypes.c_void_p * nc)(*([1] * nc))
    b = (ctypes.c_void_p * nc)(*([1] * nc))
    x, y = ctypes.c_void_p(16), ctypes.c_void_p(32)
    assert L.mzba_rep_trunk(None, y, w, b, 2, 3, 4, None) == -1
    assert L.mzba_rep_trunk(x, y, None, b, 2, 3, 4, None) == -1
    assert L.mzba_rep_trunk(x, y, w, b, -1, 3, 4, None) == -1
    assert L.mzba_rep_trunk(x, y, w, b, 2, 3, 0, None) == -1
    assert L.mzba_rep_trunk(x, x, w, b, 2, 3, 4, None) == -1
    assert L.mzba_rep_trunk(x, y, w, b, 20, 8, 4, None) == -1  # 58 convs
    wn = (ctypes.c_void_p * nc)(*([1] * (nc - 1) + [0]))
    assert L.mzba_rep_trunk(x, y, wn, b, 2, 3, 4, None) == -1


@pytest.mark.parametrize("tag", ["small", "full"])
def test_agent_random_init_equals_reference_construction(tag):
    """MuZeroAgent(cfg)'s starting weights (networks.py:245-266) are the reference agent's bit for
    bit under the same torch seed: tests/golden/agent_init.npz holds per-tensor checksums of the
    reference's own `MuZeroAgent(cfg)` built twice in a row (RLSystem's learner and target agents,
    train_torch.py:86-88) after torch.manual_seed(42) (train_torch.py set_seed) and (7)."""
    import torch
    from conftest import GOLDEN
    from mzba.weights import torch_init_state_dict
    d = np.load(os.path.join(GOLDEN, "agent_init.npz"))
    mcfg = small_model_cfg() if tag == "small" else default_config()["model"]
    for seed in (42, 7):
        torch.manual_seed(seed)
        for ai in range(2):
            sd = torch_init_state_dict(mcfg)
            assert list(sd) == [k for k, _ in state_dict_spec(mcfg)]
            for k, v in sd.items():
                f = v.numpy().astype(np.float64).reshape(-1)
                got = np.concatenate([[f.sum(), np.abs(f).sum()], f[:4], f[-1:]])
                np.testing.assert_array_equal(got, d[f"{tag}/s{seed}/a{ai}/{k}"], err_msg=f"s{seed} a{ai} {k}")


def test_conv_halo_support_matrix_and_bad_arguments_without_gpu():
    """mzba_conv_halo(_ex)'s support checks and argument checks run before any HIP call: the 21x21 latent
    convs (gathered / action-bias form too), the 84x84 and 42x42 representation convs (two-block staging past
    W = 30 at Cin 256), Cout 128 only with all Cin channels staged at once, no gather past two envs per staged
    range (4x5), no action-bias table with a residual, null buffers."""
    import ctypes
    from mzba import _lib
    L = _lib.lib()
    sup = {(H, W, ci, co): (L.mzba_conv_halo_supported(H, W, ci, co, 3), L.mzba_conv_halo_ex_supported(H, W, ci, co, 3, 1))
           for H, W, ci, co in [(21, 21, 256, 256), (21, 21, 256, 128), (42, 42, 256, 256), (84, 84, 256, 256),
                                (84, 84, 128, 128), (84, 84, 128, 256), (42, 42, 256, 128), (84, 84, 64, 128),
                                (4, 5, 256, 256)]}
    assert sup == {(21, 21, 256, 256): (1, 1), (21, 21, 256, 128): (1, 0), (42, 42, 256, 256): (1, 0),
                   (84, 84, 256, 256): (1, 0), (84, 84, 128, 128): (1, 0), (84, 84, 128, 256): (1, 0),
                   (42, 42, 256, 128): (0, 0), (84, 84, 64, 128): (0, 0), (4, 5, 256, 256): (1, 0)}
    assert L.mzba_conv_halo_supported(21, 21, 256, 256, 1) == 0
    p = ctypes.c_void_p(64)
    n = 21 * 21 * 256
    # null input / weights / bias / output
    assert L.mzba_conv_halo_ex(None, n, None, 0, p, p, None, None, 0, None, p, 4, 21, 21, 256, 256, 1, None) == -1
    assert L.mzba_conv_halo_ex(p, n, None, 0, p, None, None, None, 0, None, p, 4, 21, 21, 256, 256, 1, None) == -1
    # action-bias table without actions, with a residual
    assert L.mzba_conv_halo_ex(p, n, None, 0, p, p, p, None, 3, None, p, 4, 21, 21, 256, 256, 1, None) == -1
    assert L.mzba_conv_halo_ex(p, n, None, 0, p, p, p, p, 3, p, p, 4, 21, 21, 256, 256, 1, None) == -1
    # gather where a staged range spans more than two envs; unsupported widths
    assert L.mzba_conv_halo_ex(p, 2 * 20 * 256, p, 20 * 256, p, p, None, None, 0, None, p, 4, 4, 5, 256, 256, 1,
                               None) == -2
    assert L.mzba_conv_halo_ex(p, 21 * 21 * 64, None, 0, p, p, None, None, 0, None, p, 4, 21, 21, 64, 256, 1, None) == -2
    assert L.mzba_conv_halo(p, p, p, None, p, 4, 42, 42, 256, 128, 1, None) == -2
    # the one-block bounds halo_geometry computes with the 16-row zero block: at Cin 256 one
    # 256-channel block up to W = 23 (so the gathered GA instance, which needs it, up to W = 23; past it the
    # plain conv stages two 128-channel blocks); at Cin 128 one block up to W = 183, and nothing past it
    assert L.mzba_conv_halo_ex_supported(23, 23, 256, 256, 3, 1) == 1
    assert L.mzba_conv_halo_ex_supported(24, 24, 256, 256, 3, 1) == 0
    assert L.mzba_conv_halo_supported(24, 24, 256, 256, 3) == 1
    assert L.mzba_conv_halo_supported(24, 24, 256, 128, 3) == 0  # Cout 128 needs one staged block
    assert L.mzba_conv_halo_supported(8, 183, 128, 128, 3) == 1
    assert L.mzba_conv_halo_supported(8, 184, 128, 128, 3) == 0
    assert L.mzba_conv_halo_supported(8, 183, 256, 256, 3) == 1
    assert L.mzba_conv_halo_supported(8, 184, 256, 256, 3) == 0


def test_learner_optimizer_param_groups_persist_and_lr_writes_reach_the_learner():
    """`for g in opt.param_groups: g["lr"] = x` must act like torch.optim.Adam's — one persistent group
    whose lr the next step() uses; the kernel's fixed hyperparameters refuse a change instead of ignoring it."""
    from mzba.agent import LearnerOptimizer

    class Ln:
        lr = 1e-3

    class Ag:
        _learner = Ln()
        cfg = {"learning_rate": 1e-3}

        def parameters(self):
            return iter([np.zeros(1)])

    opt = LearnerOptimizer(Ag())
    assert opt.param_groups is opt.param_groups
    for g in opt.param_groups:
        g["lr"] = 2.5e-4
    opt._sync_groups(Ag._learner)
    assert Ag._learner.lr == 2.5e-4
    opt.param_groups[0]["betas"] = [0.9, 0.999]  # a list equal to the constant is fine
    opt._sync_groups(Ag._learner)
    opt.param_groups[0]["weight_decay"] = 0.0
    with pytest.raises(NotImplementedError):
        opt._sync_groups(Ag._learner)


def test_learner_entry_points_reject_bad_arguments_without_gpu():
    """Every learner entry point of csrc/learn.hip and csrc/pack.hip that tests/test_gpu_learner_ops.py covers checks
    its arguments before any HIP call: otherwise valid (dummy, non-null) arguments with one violation each return the
    documented code. Runs only where no GPU is visible, so a missing check can never launch a kernel on the dummy pointers."""
    import ctypes
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: a missing check would launch on dummy pointers")
    from mzba import _lib
    L = _lib.lib()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(8192)
    eps, mom = 1e-5, 0.1
    # BatchNorm: C % 4, scratch one byte short, empty batch, one running statistic without the other, dtype
    assert L.mzba_bn_stats(0, p, 65, 6, eps, mom, p, p, p, p, p, p, 1 << 20, None) == -1
    assert L.mzba_bn_stats(0, p, 0, 8, eps, mom, p, p, p, p, p, p, 1 << 20, None) == -1
    assert L.mzba_bn_stats(0, p, 65, 8, eps, mom, p, p, p, p, None, p, 1 << 20, None) == -1
    assert L.mzba_bn_stats(0, p, 65, 8, eps, mom, p, p, p, None, p, p, 1 << 20, None) == -1
    assert L.mzba_bn_stats(1, p, 65, 8, eps, mom, p, p, p, p, p, p, 2 * 8 * 8 - 1, None) == -2
    assert L.mzba_bn_stats(2, p, 65, 8, eps, mom, p, p, p, p, p, p, 1 << 20, None) == -9
    assert L.mzba_bn_stats_final(p, 2, 64, 129, 8, eps, mom, p, p, p, p, p, None) == -1
    assert L.mzba_bn_stats_final(p, 3, 64, 128, 8, eps, mom, p, p, p, p, p, None) == -1
    assert L.mzba_bn_stats_final(p, 2, 64, 128, 8, eps, mom, p, p, p, p, None, None) == -1
    assert L.mzba_bn_apply(0, p, p, None, 1, p, 65, 6, None) == -1
    assert L.mzba_bn_apply(1, p, p, None, 1, None, 65, 8, None) == -1
    assert L.mzba_bn_backward(0, p, p, p, p, 65, 6, p, p, p, p, 1 << 20, None) == -1
    assert L.mzba_bn_backward(1, p, None, p, p, 65, 8, p, p, p, p, 2 * 8 * 8 + 12 * 8 - 1, None) == -2
    assert L.mzba_bn_backward_final(0, p, p, p, p, 2, 65, 6, p, p, p, p, 1 << 20, None) == -1
    assert L.mzba_bn_backward_final(1, p, p, p, p, 2, 65, 8, p, p, p, p, 12 * 8 - 1, None) == -2
    assert L.mzba_bn_backward_coef(p, 0, 65, 8, p, p, p, p, None) == -1
    assert L.mzba_bn_backward_coef(p, 2, 65, 8, p, p, p, None, None) == -1
    assert L.mzba_bn_backward_apply(0, p, p, p, p, p, 65, 6, None) == -1
    # avg-pool backward: odd or empty extents; axpy; the min-max scale
    for H, W, C in ((3, 4, 8), (4, 5, 8), (0, 4, 8), (4, 0, 8), (4, 4, 0), (-2, 4, 8)):
        assert L.mzba_avgpool2_backward(0, p, q, 3, H, W, C, None) == -1, (H, W, C)
    assert L.mzba_avgpool2_backward(1, p, q, 0, 4, 4, 8, None) == -1
    assert L.mzba_axpy(0, p, q, -1, None) == -1
    assert L.mzba_axpy(1, p, None, 4, None) == -1
    assert L.mzba_scale_forward(0, p, q, p, p, 5, 0, 4, None) == -1
    assert L.mzba_scale_forward(1, p, q, p, p, 5, 20, 0, None) == -1
    assert L.mzba_scale_backward(0, p, p, p, p, q, 5, 0, 0, None) == -1
    assert L.mzba_scale_backward(1, p, p, p, None, q, 5, 80, 1, None) == -1
    # Linear heads: at most 16 outputs, scratch one byte short
    assert L.mzba_linear_forward(0, p, p, p, q, 4, 100, 17, None) == -1
    assert L.mzba_linear_forward(1, p, p, p, q, 4, 100, 0, None) == -1
    assert L.mzba_linear_backward(0, p, p, p, q, 0, p, p, 64, 100, 17, p, 1 << 20, None) == -1
    need = L.mzba_linear_ws_bytes(64, 100, 3)
    assert need == 16 * (3 * 100 + 3) * 4
    assert L.mzba_linear_backward(1, p, p, p, None, 0, p, p, 64, 100, 3, p, need - 1, None) == -2
    # loss: 2 <= ns <= 16, 1 <= na <= 16, scratch one byte short
    lo, hi = ctypes.c_float(-5.0), ctypes.c_float(5.0)
    for ns, na in ((17, 3), (11, 17), (1, 3), (11, 0)):
        assert L.mzba_learner_loss(p, p, p, p, p, p, None, 4, 5, ns, na, lo, hi, q, q, q, q, None) == -1, (ns, na)
        assert L.mzba_learner_loss_ws(p, p, p, p, p, p, None, 4, 5, ns, na, lo, hi, q, q, q, q, p, 1 << 20,
                                      None) == -1, (ns, na)
    assert L.mzba_learner_loss_ws_bytes(4, 5) == 3 * 4 * 5 * 8
    assert L.mzba_learner_loss_ws(p, p, p, p, p, p, p, 4, 5, 11, 3, lo, hi, q, q, q, q, p, 3 * 4 * 5 * 8 - 1, None) == -2
    # Adam
    sc = [ctypes.c_float(v) for v in (-1e-3, 0.1, 0.999, 1e-3, 1.0, 1e-8, 1e-4)]
    assert L.mzba_adam(p, p, p, p, -1, *sc, None) == -1
    assert L.mzba_adam(p, p, None, p, 8, *sc, None) == -1
    assert L.mzba_adam_dev(p, p, p, p, -1, p, None) == -1
    assert L.mzba_adam_dev(p, p, p, p, 8, None, None) == -1
    # input builders: room for the 2 L planes, an image, an unroll step below K, room for h and the action planes
    assert L.mzba_learner_input(0, p, p, p, p, q, 5, 4, 20, 7, None) == -1
    assert L.mzba_learner_input(1, p, p, p, p, q, 5, 4, 0, 8, None) == -1
    assert L.mzba_learner_input(0, p, p, None, p, q, 5, 4, 20, 8, None) == -1
    assert L.mzba_dyn_input(0, p, p, p, 5, 5, q, 5, 20, 32, 3, 40, None) == -1
    assert L.mzba_dyn_input(1, p, p, p, 5, -1, q, 5, 20, 32, 3, 40, None) == -1
    assert L.mzba_dyn_input(0, p, p, p, 5, 0, q, 5, 0, 32, 3, 40, None) == -1
    assert L.mzba_dyn_input(1, p, p, p, 5, 0, q, 5, 20, 32, 3, 34, None) == -1
    # batched weight pack: job count, output alignment, pad % 8, layout, the layouts' shape rules, the flip rule
    w, o = (ctypes.c_void_p * 1)(4096), (ctypes.c_void_p * 1)(8192)

    def pack(*prm, out=o, njobs=1):
        return L.mzba_conv_pack_bf16_multi(w, out, (ctypes.c_int * 8)(*prm), njobs, None)
    assert pack(32, 9, 32, 32, 32, 0, 1, 8, njobs=0) == -1
    assert pack(32, 9, 32, 32, 32, 0, 1, 8, out=(ctypes.c_void_p * 1)(8200)) == -1
    assert pack(32, 9, 32, 32, 32, 0, 1, 4) == -1
    assert pack(32, 9, 32, 32, 32, 0, 3, 8) == -1
    assert pack(48, 9, 32, 48, 32, 0, 1, 8) == -2
    assert pack(16, 1, 64, 16, 64, 0, 2, 8) == -3
    assert pack(32, 9, 64, 64, 64, 1, 1, 8) == -4
