"""Weight hand-off on the device (csrc/pack.hip, mzba/refresh.py): PackedNets.refresh_from_learner /
MuZeroAgent.refresh_from_learner against the host packer.

The oracle is the host packer itself: for any learner state, PackedNets(learner.state_dict(), cfg, "bf16", device,
dyn_dtype) defines every bit the device path must write, pad regions included, so every comparison below is on the
tensors' integer views and the only accepted count of differing elements is zero.

Configurations (4x5 latent, L = 4): N = small_model_cfg() (plain, pack_lat, action-table and Linear jobs; the band
kernel takes no 64-channel conv, so no band, tower, fused or rep packs), W = channels [128, 256], rep blocks
[1, 1, 1], 1 dynamics and 2 prediction blocks (band packs and every fused pack; unequal block counts), W16 = W with
the fp16 dynamics copies. The learner state is not an init: BatchNorm
gamma ~ N(1, 0.3) with a negative and an exact zero per net, beta ~ N(0, 0.2), running_mean ~ N(0, 0.5), running_var
log-uniform over [1e-6, 1e2], conv biases ~ N(0, 0.1). The pack under test starts as the pack of another random state.
"""
import copy

import numpy as np
import pytest
import torch

from mzba.config import small_model_cfg
from mzba.weights import init_state_dict, state_dict_spec

pytestmark = pytest.mark.gpu


def _cfg(name):
    m = small_model_cfg()
    if name != "N":
        m["latent_channels"] = [128, 256]
        m["dynamics_network"] = {**m["dynamics_network"], "num_res_blocks": 1}
        m["prediction_network"] = {**m["prediction_network"], "num_res_blocks": 2}
    assert tuple(m["latent_resolution"]) == (4, 5) and m["state_history_length"] == 4
    return m, ("fp16" if name == "W16" else None)


def _state(mcfg, seed):
    """The issue's learner state: the init's weights, every BatchNorm and conv bias drawn."""
    sd = init_state_dict(mcfg, seed)
    shapes = dict(state_dict_spec(mcfg))
    g = np.random.default_rng(1000 + seed)
    first_bn = {}
    for key, shape in shapes.items():
        leaf = key.rsplit(".", 1)[1]
        if key[: -len(leaf)] + "running_mean" in shapes:  # a BatchNorm's five entries
            if leaf == "weight":
                v = g.normal(1.0, 0.3, shape)
                first_bn.setdefault(key.split(".")[0], key)
            elif leaf == "bias":
                v = g.normal(0.0, 0.2, shape)
            elif leaf == "running_mean":
                v = g.normal(0.0, 0.5, shape)
            elif leaf == "running_var":
                v = np.exp(g.uniform(np.log(1e-6), np.log(1e2), shape))
            else:
                sd[key] = np.asarray(int(g.integers(0, 1000)), dtype=np.int64)
                continue
            sd[key] = v.astype(np.float32)
        elif leaf == "bias" and len(shapes[key[: -len("bias")] + "weight"]) == 4:
            sd[key] = g.normal(0.0, 0.1, shape).astype(np.float32)
    assert sorted(first_bn) == ["dyn_net", "pred_net", "rep_net"]
    for key in first_bn.values():  # a negative and an exactly zero gamma in every net
        sd[key][0], sd[key][1] = np.float32(-0.7), np.float32(0.0)
    return sd


def _ints(t):
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()])


def _diff(pack, ref, label):
    """Per tensor, the count of elements whose bits differ (pad regions included); prints them, returns the total."""
    from mzba.refresh import named_tensors
    a, b = named_tensors(pack), named_tensors(ref)
    assert list(a) == list(b)
    total = 0
    for path in a:
        assert a[path].shape == b[path].shape and a[path].dtype == b[path].dtype, path
        n = int((_ints(a[path]) != _ints(b[path])).sum())
        print(f"{label} {path}: {n} of {a[path].numel()} differ ({a[path].dtype})")
        total += n
    assert {t.data_ptr() for t in pack.device_tensors()} == {t.data_ptr() for t in a.values()}
    return total


def _pack(sd, name):
    from mzba.agent import PackedNets
    mcfg, dd = _cfg(name)
    return PackedNets(sd, mcfg, "bf16", "cuda", dd)


_WORLD = {}


def _world(name):
    """Per configuration, once: a learner in the issue's state, its host pack (the reference, left unchanged), and
    a pack of another state refreshed from the learner on the device."""
    if name not in _WORLD:
        from mzba.learner import Learner
        mcfg, _ = _cfg(name)
        learner = Learner(mcfg, _state(mcfg, 3), dtype="bf16")
        ref = _pack(learner.state_dict(), name)
        pack = _pack(_state(mcfg, 4), name)
        before = _diff(pack, ref, name + " before")
        pack.refresh_from_learner(learner)
        torch.cuda.synchronize()
        _WORLD[name] = dict(mcfg=mcfg, learner=learner, ref=ref, pack=pack, before=before)
    return _WORLD[name]


@pytest.mark.parametrize("name", ["N", "W", "W16"])
def test_refresh_bit_equal_every_tensor(name):
    """Every tensor of device_tensors() after refresh_from_learner == the host pack of learner.state_dict(), as
    integers, pads included: the index maps, the f64 fold, the f64 -> f32 -> bf16 / fp16 rounding chain and the action
    table's summation order. Zero differing elements everywhere."""
    w = _world(name)
    assert w["before"] > 0  # the starting pack was another state's
    if name != "N":  # W holds what it is there for: every fused pack, several million tower elements
        p = w["pack"]
        assert p.dyn_tower and p.pred_tower and p.fused and p.rep_tail and p.rep_blocks
        assert p.dyn_tower["n"] == 1 and p.pred_tower["n"] == 2 and p.pred_tower["wf"].numel() > 2_000_000
        assert ("wf16" in p.dyn_tower and "dyn16" in p.fused) == (name == "W16")
        assert any("wt" in layer[1][0] for layer in p.rep if layer[0] == "res")  # the band packing (>= 128 channels)
    else:
        p = w["pack"]
        assert p.dyn_tower is None and p.fused is None and p.rep_tail is None and p.rep_blocks is None
        assert "wf" in p.dyn0 and p.dyn0["act_bias"] is not None and "wb" in p.rew_lin
    assert _diff(w["pack"], w["ref"], name) == 0


def test_refresh_captured_in_a_graph():
    """refresh_from_learner inside torch.cuda.graph (a synchronisation or a D2H copy would abort the capture); then
    the learner's weights move in place (one adam_step on a random G, one BN's running statistics overwritten) and the
    replayed graph writes the host pack of the new state."""
    from mzba.learner import Learner
    mcfg, _ = _cfg("W")
    learner = Learner(mcfg, _state(mcfg, 5), dtype="bf16")
    pack = _pack(_state(mcfg, 6), "W")
    pack.refresh_from_learner(learner)  # builds the job table (uploads): before the capture, as any warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pack.refresh_from_learner(learner)
    g = torch.Generator(device="cuda").manual_seed(7)
    learner.G.copy_(torch.randn(learner.G.shape, generator=g, device="cuda") * 0.05)
    old = learner.P.clone()
    learner.adam_step()
    assert int((learner.P != old).sum()) > learner.P.numel() // 2
    rm, rv = learner.run["pred_net.res_blocks.1.bn2"]
    rm.copy_(torch.randn(rm.shape, generator=g, device="cuda"))
    rv.copy_(torch.rand(rv.shape, generator=g, device="cuda") * 3 + 1e-3)
    ref = _pack(learner.state_dict(), "W")
    assert _diff(pack, ref, "W stale") > 0
    graph.replay()
    torch.cuda.synchronize()
    assert _diff(pack, ref, "W replayed") == 0


def test_agent_runs_the_new_weights_and_keeps_its_contract():
    """Agent A refreshed on the device and agent B loaded through the host run the same bits (the three reference
    entry points at B = 4, and a runner created before the refresh: the buffers were written in place); and
    A.state_dict() stays learner.state_dict() as of the refresh after the learner has moved on."""
    from mzba.agent import MuZeroAgent
    w = _world("W")
    mcfg, learner = w["mcfg"], w["learner"]
    torch.manual_seed(11)
    A, B = MuZeroAgent(mcfg, dtype="bf16"), MuZeroAgent(mcfg, dtype="bf16")
    rA, rB = A.runner(4, 16, 20), B.runner(4, 16, 20)  # before the refresh
    ptrs = [t.data_ptr() for t in A.packed.device_tensors()]
    sd0 = learner.state_dict()
    A.refresh_from_learner(learner)
    B.load_state_dict(sd0)
    assert [t.data_ptr() for t in A.packed.device_tensors()] == ptrs
    assert _diff(A.packed, B.packed, "agent") == 0
    g = torch.Generator().manual_seed(12)
    x = torch.rand(4, 8, 16, 20, generator=g).cuda()
    act = torch.nn.functional.one_hot(torch.randint(0, 3, (4, 4, 5), generator=g), 3).permute(0, 3, 1, 2).float().cuda()
    out = []
    for ag, rn in ((A, rA), (B, rB)):
        h = ag.create_hidden_state_root(x)
        h2, rl = ag.hidden_state_transition(h, act)
        pl, vl = ag.evaluate_state(h2)
        lat = torch.rand(4, 20 * 256, generator=torch.Generator().manual_seed(13)).to(torch.bfloat16).cuda()
        pi, v = torch.empty(4, 3, device="cuda"), torch.empty(4, device="cuda")
        plg, vlg = torch.empty(4, 3, device="cuda"), torch.empty(4, 11, device="cuda")
        rn.prediction(lat, pi, v, plg, vlg)
        torch.cuda.synchronize()
        out.append([t.float().cpu() for t in (h, h2, rl, pl, vl, pi, v, plg, vlg)])
    for a, b in zip(*out):
        assert torch.isfinite(a).all() and a.abs().sum() > 0
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the learner moves on in place; A's host copy is the state at the refresh
    keep_P, keep_run = learner.P.clone(), {k: (m.clone(), v.clone()) for k, (m, v) in learner.run.items()}
    keep_nbt = dict(learner.nbt)
    try:
        learner.P.mul_(1.25)
        for k, (m, v) in learner.run.items():
            m.add_(0.5)
            v.mul_(2.0)
            learner.nbt[k] += 1
        got = A.state_dict()
        assert list(got) == list(sd0)
        for k in sd0:
            assert got[k].dtype == sd0[k].dtype and got[k].shape == sd0[k].shape and torch.equal(got[k], sd0[k]), k
        assert all(torch.equal(p.detach(), sd0[k]) for k, p in A.named_parameters())
    finally:  # the shared learner as it was
        learner.P.copy_(keep_P)
        for k, (m, v) in learner.run.items():
            m.copy_(keep_run[k][0])
            v.copy_(keep_run[k][1])
        learner.nbt.update(keep_nbt)


def test_refusals_and_fallback():
    """A learner of another configuration: ValueError, nothing written. An f32 agent: the host path's pack. A pack
    tensor the job table does not know: NotImplementedError naming it."""
    from mzba.agent import MuZeroAgent
    from mzba.learner import Learner
    n, w = _world("N"), _world("W")
    pack = _pack(_state(n["mcfg"], 8), "N")
    was = [t.clone() for t in pack.device_tensors()]
    with pytest.raises(ValueError):
        pack.refresh_from_learner(w["learner"])
    deeper = copy.deepcopy(n["mcfg"])
    deeper["prediction_network"]["num_res_blocks"] = 3
    with pytest.raises(ValueError):
        pack.refresh_from_learner(Learner(deeper, init_state_dict(deeper, 1), dtype="bf16"))
    torch.cuda.synchronize()
    assert all(torch.equal(_ints(a), _ints(b)) for a, b in zip(pack.device_tensors(), was))
    ag = MuZeroAgent(n["mcfg"], dtype="bf16")
    ag.packed
    with pytest.raises(ValueError):
        ag.refresh_from_learner(w["learner"])
    # f32 agent: the fallback is load_state_dict(learner.state_dict())
    A, B = MuZeroAgent(n["mcfg"], dtype="f32"), MuZeroAgent(n["mcfg"], dtype="f32")
    A.packed
    A.refresh_from_learner(n["learner"])
    B.load_state_dict(n["learner"].state_dict())
    assert len(A.packed.device_tensors()) == len(B.packed.device_tensors()) > 0
    assert all(torch.equal(_ints(a), _ints(b)) for a, b in zip(A.packed.device_tensors(), B.packed.device_tensors()))
    with pytest.raises(ValueError):
        A.packed.refresh_from_learner(n["learner"])  # the pack method itself writes bf16 packs only
    # an extra tensor in the pack: refused by name, nothing written
    pack.dyn0["extra_table"] = torch.zeros(64, device="cuda")
    with pytest.raises(NotImplementedError, match="dyn0.extra_table"):
        pack.refresh_from_learner(n["learner"])
    del pack.dyn0["extra_table"]
    torch.cuda.synchronize()
    assert all(torch.equal(_ints(a), _ints(b)) for a, b in zip(pack.device_tensors(), was))
    pack.refresh_from_learner(n["learner"])
    torch.cuda.synchronize()
    assert _diff(pack, n["ref"], "N again") == 0
