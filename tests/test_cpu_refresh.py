"""The device weight hand-off's job-table builder (mzba/refresh.py:plan), shapes only: no device tensor.

The expected tensor list of a bf16 pack is restated here from PackedNets' own rules (agent.py: which packings a layer
gets, and their sizes), so plan() is checked against the pack's structure, not against itself: every tensor written
exactly once over its non-pad extent, no overlap, nothing past the end; anything else refused by name."""
import copy

import pytest
import torch

from mzba.config import default_config, small_model_cfg
from mzba.weights import rep_layout

PAD = 8 * 64 * 8  # agent.LAT_PAD_ELEMS
BF, F32, F16 = torch.bfloat16, torch.float32, torch.float16


def _r64(c):
    return (c + 63) // 64 * 64


def _expected(mcfg, fp16):
    """(tensors, meta) of PackedNets(sd, mcfg, "bf16", ..., "fp16" if fp16 else None) at a 16x20 input."""
    from mzba import _lib as L
    lib = L.lib()
    c0, c1 = mcfg["latent_channels"]
    hw = mcfg["latent_resolution"][0] * mcfg["latent_resolution"][1]
    ns, A = mcfg["num_supports"], mcfg["dynamics_network"]["num_actions"]
    na = mcfg["prediction_network"]["num_actions"]
    nd, npred = mcfg["dynamics_network"]["num_res_blocks"], mcfg["prediction_network"]["num_res_blocks"]
    t = {}

    def conv(path, cin, cout, ks, band=False, act=0):
        cp = _r64(cin)
        t[path + ".w"] = (cout * ks * ks * cp, BF)
        t[path + ".b"] = (cout, F32)
        if act:
            t[path + ".act_bias"] = (hw * act * cout, F32)
        if cout % 32 == 0 and cp in (64, 128, 256):
            t[path + ".wf"] = (cout * ks * ks * cp + PAD, BF)
        if band and ks == 3 and lib.mzba_conv_band_supported(16, 20, cin, cout, 3):
            t[path + ".wt"] = (cout * 9 * cin + PAD, BF)

    def lin(path, c, O):
        t[path + ".w"], t[path + ".b"], t[path + ".wb"] = (O * c * hw, F32), (O, F32), (16 * c * hw, BF)

    lay = rep_layout(mcfg)
    cin, nconv = 2 * mcfg["state_history_length"], 0
    for pos, (kind, _) in enumerate(lay):
        if kind == "conv":
            cout = c0 if nconv == 0 else c1
            conv(f"rep.{pos}.1", cin, cout, 3, band=True)
            cin, nconv = cout, nconv + 1
        elif kind == "res":
            conv(f"rep.{pos}.1.0", cin, cin, 3, band=True)
            conv(f"rep.{pos}.1.1", cin, cin, 3, band=True)
    conv("dyn0", c1, c1, 3, act=A)
    for nm, n in (("dyn", nd), ("pred", npred)):
        for i in range(n):
            conv(f"{nm}.{i}.0", c1, c1, 3)
            conv(f"{nm}.{i}.1", c1, c1, 3)
    conv("rew_conv", c1, c1, 1)
    conv("pol_conv", c1, c1 // 2, 3)
    conv("val_conv", c1, c1 // 2, 1)
    lin("rew_lin", c1, ns)
    lin("pol_lin", c1 // 2, na)
    lin("val_lin", c1 // 2, ns)
    meta = {"rep_tail": None, "rep_blocks": None}
    if c1 == 256 and hw == 20:
        for nm, n in (("dyn_tower", nd), ("pred_tower", npred)):
            t[nm + ".wf"], t[nm + ".b"] = (2 * n * 9 * c1 * c1 + PAD, BF), (2 * n * c1, F32)
        if fp16:
            t["dyn_tower.wf16"] = (2 * nd * 9 * c1 * c1 + PAD, F16)
        for k, co, taps in (("w0", c1, 9), ("rw", c1, 1), ("pw", c1 // 2, 9), ("vw", c1 // 2, 1)):
            t["fused." + k] = (co * taps * c1 + PAD, BF)
            if fp16 and k in ("w0", "rw"):
                t["fused.dyn16." + k] = (co * taps * c1 + PAD, F16)
        t["fused.rb"], t["fused.pb"], t["fused.vb"] = (c1, F32), (c1 // 2, F32), (c1 // 2, F32)
        if fp16:
            t["fused.dyn16.lw"] = (16 * c1 * hw, F16)
        n0, n1, n2 = mcfg["representation_network"]["num_res_blocks"]
        pool1 = 2 + n0 + n1  # rep_layout: conv, n0 res, conv, n1 res, pool, n2 res, pool
        if n2:
            meta["rep_tail"] = (pool1, n2)
            t["rep_tail.wf"], t["rep_tail.b"] = (2 * n2 * 9 * c1 * c1 + PAD, BF), (2 * n2 * c1, F32)
        if n1:
            meta["rep_blocks"] = (pool1 - n1, n1)
            t["rep_blocks.wf"], t["rep_blocks.b"] = (2 * n1 * 9 * c1 * c1 + PAD, BF), (2 * n1 * c1, F32)
    return t, meta


def _wide():
    m = small_model_cfg()
    m["latent_channels"] = [128, 256]
    m["dynamics_network"] = {**m["dynamics_network"], "num_res_blocks": 1}
    return m


CASES = {"N": (small_model_cfg, False), "W": (_wide, False), "W16": (_wide, True),
         "full": (lambda: default_config()["model"], False), "full16": (lambda: default_config()["model"], True)}


@pytest.mark.parametrize("name", list(CASES))
def test_plan_covers_every_tensor_exactly_once(name):
    from mzba.refresh import ACT, BIAS, plan
    mk, fp16 = CASES[name]
    mcfg = mk()
    tensors, meta = _expected(mcfg, fp16)
    jobs, pads = plan(mcfg, tensors, meta)
    assert set(pads) == set(tensors)
    spans = {}
    for j in jobs:
        assert j.off >= 0 and j.n > 0 and j.off + j.n <= tensors[j.path][0] - pads[j.path], j.path
        assert j.kind in (BIAS, ACT) or (j.off % 8 == 0 and j.n % 8 == 0 and j.units() * 8 == j.n)
        assert (j.otype == 0) == (tensors[j.path][1] == F32)
        spans.setdefault(j.path, []).append((j.off, j.off + j.n))
    for path, (numel, _) in tensors.items():
        s = sorted(spans[path])
        assert s[0][0] == 0 and all(a[1] == b[0] for a, b in zip(s, s[1:])), path  # no gap, no overlap
        assert s[-1][1] == sum(b - a for a, b in s) == numel - pads[path], path
        leaf = path.rsplit(".", 1)[1]
        want = PAD if leaf in ("wf", "wt", "wf16", "w0", "rw", "pw", "vw") else 0
        if leaf in ("wb", "lw"):  # 16 rows of K, the first O written
            O = mcfg["prediction_network"]["num_actions"] if path.startswith("pol_lin") else mcfg["num_supports"]
            want = numel // 16 * (16 - O)
        assert pads[path] == want, path
    if name in ("W", "W16"):  # the concatenated towers: slices in block order, conv1 before conv2
        offs = [(j.key, j.off) for j in jobs if j.path == "pred_tower.wf"]
        assert offs == [(f"pred_net.res_blocks.{i}.conv{k}.weight", (2 * i + k - 1) * 9 * 256 * 256)
                        for i in range(2) for k in (1, 2)]
        assert [j.key for j in jobs if j.path == "rep_tail.wf"] == [f"rep_net.blocks.5.conv{k}.weight" for k in (1, 2)]
        assert [j.key for j in jobs if j.path == "rep_blocks.wf"] == [f"rep_net.blocks.3.conv{k}.weight"
                                                                      for k in (1, 2)]


def test_plan_refuses_what_it_does_not_cover():
    from mzba.refresh import check_config, check_coverage, plan
    mcfg = _wide()
    tensors, meta = _expected(mcfg, True)
    extra = dict(tensors)
    extra["dyn0.wx3"] = (1024, BF)
    with pytest.raises(NotImplementedError, match="dyn0.wx3"):
        plan(mcfg, extra, meta)
    longer = dict(tensors)
    longer["pred_tower.wf"] = (tensors["pred_tower.wf"][0] + 9 * 256 * 256 * 2, BF)  # a third block's slice unwritten
    with pytest.raises(NotImplementedError, match="pred_tower.wf"):
        plan(mcfg, longer, meta)
    with pytest.raises(ValueError):
        plan(mcfg, tensors, {**meta, "rep_tail": (1, 2)})  # not residual blocks
    jobs, pads = plan(mcfg, tensors, meta)
    j = next(j for j in jobs if j.path == "dyn_tower.b" and j.off > 0)
    j.off -= 8  # overlaps its neighbour
    with pytest.raises(NotImplementedError, match="dyn_tower.b"):
        check_coverage(tensors, jobs, pads)
    other = copy.deepcopy(mcfg)
    other["state_history_length"] = 8
    with pytest.raises(ValueError, match="state_history_length"):
        check_config(mcfg, other)
    check_config(mcfg, copy.deepcopy(mcfg))
