"""Weight hand-off on the device: the acting nets' packs written from a `Learner`'s master weights.

`PackedNets(sd, ...)` (agent.py) folds every BatchNorm and permutes every conv into its kernel packings on the host, in
f64 numpy. This module states the same packing as a job table for csrc/pack.hip: one job writes one destination
tensor, or one slice of a concatenated one, from the learner's flat f32 buffer (`Learner.P`, already
[Cout][tap][Cin_pad8] / [O][pixel][C]) and its running statistics, with the host packer's bits.

  plan(mcfg, tensors, meta)   shapes only (no device): walks the structure PackedNets.__init__ walks and lists, per
                              destination tensor, the parameter key, the BatchNorm and the layout that feed it; then
                              checks that the jobs tile every tensor's non-pad extent exactly once.
  RefreshTable(learner, pack) binds a plan to device pointers and uploads the two tables; run() is two launches with
                              fixed arguments on the current stream: no host synchronisation, graph-capturable.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import _lib as L
from .weights import LAT_PAD_ELEMS, _pad8, _round64, rep_layout  # LAT_PAD_ELEMS: trailing zeros never written here

PLAIN, LAT, LAT16, BIAS, ACT = range(5)  # csrc/pack.hip PF_*
OTYPE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}

JOB_DT = np.dtype([("w", "<u8"), ("ab", "<u8"), ("dst", "<u8"), ("off", "<i8"), ("kind", "<i4"), ("otype", "<i4"),
                   ("cout", "<i4"), ("taps", "<i4"), ("cin_src", "<i4"), ("c_first", "<i4"), ("c_used", "<i4"),
                   ("cin_dst", "<i4"), ("tperm", "<i4"), ("H", "<i4"), ("W", "<i4"), ("A", "<i4")])
BN_DT = np.dtype([("gamma", "<u8"), ("beta", "<u8"), ("mean", "<u8"), ("var", "<u8"), ("out", "<u8"), ("C", "<i4"),
                  ("pad_", "<i4")])

PACK_ATTRS = ("rep", "dyn0", "dyn", "rew_conv", "rew_lin", "pred", "dyn_tower", "pred_tower", "pol_conv", "pol_lin",
              "val_conv", "val_lin", "fused", "rep_tail", "rep_blocks")  # PackedNets.device_tensors()'s order

CFG_KEYS = (("latent_channels",), ("latent_resolution",), ("state_history_length",), ("num_supports",),
            ("representation_network", "num_res_blocks"), ("dynamics_network", "num_res_blocks"),
            ("dynamics_network", "num_actions"), ("prediction_network", "num_res_blocks"),
            ("prediction_network", "num_actions"))


def named_tensors(pack):
    """path -> tensor for every device tensor of the pack, in device_tensors() order; an alias (fused.b0 is
    dyn0.b) is listed once, under its first path."""
    out, seen = OrderedDict(), set()

    def walk(path, x):
        if isinstance(x, torch.Tensor):
            if id(x) not in seen:
                seen.add(id(x))
                out[path] = x
        elif isinstance(x, dict):
            for k in sorted(x):
                walk(f"{path}.{k}", x[k])
        elif isinstance(x, (list, tuple)):
            for i, y in enumerate(x):
                walk(f"{path}.{i}", y)

    for nm in PACK_ATTRS:
        walk(nm, getattr(pack, nm))
    return out


class Job:
    """One destination tensor (or slice): `n` elements from `off` of tensor `path`, from parameter `key` folded with
    BatchNorm `bn` (None: no BatchNorm)."""
    __slots__ = ("path", "key", "bn", "kind", "otype", "off", "n", "cout", "taps", "cin_src", "c_first", "c_used",
                 "cin_dst", "tperm", "H", "W", "A")

    def __init__(self, path, key, bn, kind, otype, off, cout, taps=1, cin_src=0, c_first=0, c_used=0, cin_dst=0,
                 tperm=0, H=0, W=0, A=0):
        self.path, self.key, self.bn, self.kind, self.otype, self.off = path, key, bn, kind, otype, off
        self.cout, self.taps, self.cin_src, self.c_first, self.c_used = cout, taps, cin_src, c_first, c_used
        self.cin_dst, self.tperm, self.H, self.W, self.A = cin_dst, tperm, H, W, A
        if kind == BIAS:
            self.n = cout
        elif kind == ACT:
            self.n = H * W * A * cout
        else:
            self.n = cout * taps * cin_dst
            ok = cin_dst % 8 == 0 and cin_src % 8 == 0 and c_first % 8 == 0 and off % 8 == 0 and c_used <= cin_dst
            if kind == LAT:
                ok = ok and cout % 32 == 0 and cin_dst % 32 == 0
            if kind == LAT16:
                ok = ok and cout % 16 == 0 and (taps * cin_dst) % 32 == 0 and (not tperm or taps == 9)
            if not ok:
                raise NotImplementedError(f"refresh: {path}: shape ({cout}, {taps}, {cin_dst}) has no device packing")

    def units(self):
        """Threads of pack_fold_kernel: 8 destination elements each for a weight job, one otherwise."""
        return self.n if self.kind in (BIAS, ACT) else self.n // 8


def plan(mcfg, tensors, meta):
    """The job list for a pack whose device tensors are `tensors` (path -> (numel, torch dtype), named_tensors()'s
    paths) of model config `mcfg`; meta: {"rep_tail": (first, n) or None, "rep_blocks": (first, n) or None}, the
    rep_layout positions of the two fused representation packs. Returns (jobs, pads): pads[path] = the trailing
    elements of that tensor no job writes (zero from the pack's construction). Raises NotImplementedError naming a
    tensor no job covers, or one whose jobs do not tile it exactly once."""
    c0, c1 = mcfg["latent_channels"]
    hist = mcfg["state_history_length"]
    lh, lw = mcfg["latent_resolution"]
    ns = mcfg["num_supports"]
    A = mcfg["dynamics_network"]["num_actions"]
    na = mcfg["prediction_network"]["num_actions"]
    hw = lh * lw
    jobs, pads = [], {}

    def add(path, pad, *a, **k):
        if path not in tensors:
            return False
        pads[path] = pad
        jobs.append(Job(path, *a, otype=OTYPE[tensors[path][1]], **k))
        return True

    def conv(path, key_w, key_b, bn, cin, cout, ks, act=0):
        """One conv layer dict of PackedNets._conv: cin real input channels (the action planes not counted)."""
        taps, src, cp = ks * ks, _pad8(cin + act), _round64(cin)
        g = dict(cout=cout, taps=taps, cin_src=src, c_used=cin)
        add(path + ".w", 0, key_w, bn, PLAIN, off=0, cin_dst=cp, **g)
        add(path + ".b", 0, key_b, bn, BIAS, off=0, cout=cout)
        add(path + ".wf", LAT_PAD_ELEMS, key_w, bn, LAT, off=0, cin_dst=cp, **g)
        add(path + ".wh", 0, key_w, bn, LAT16, off=0, cin_dst=cp, **g)
        add(path + ".wt", LAT_PAD_ELEMS, key_w, bn, LAT16, off=0, cin_dst=cin, tperm=1, **g)
        if act:
            add(path + ".act_bias", 0, key_w, bn, ACT, off=0, cout=cout, taps=taps, cin_src=src, c_first=cin, H=lh,
                W=lw, A=act)

    def res(path, pre, c):
        for k in (1, 2):
            conv(f"{path}.{k - 1}", f"{pre}.conv{k}.weight", f"{pre}.conv{k}.bias", f"{pre}.bn{k}", c, c, 3)

    def linear(path, pre, c, O, extra=()):
        K = c * hw
        g = dict(cout=O, taps=1, cin_src=K, c_used=K, cin_dst=K)
        add(path + ".w", 0, pre + ".weight", None, PLAIN, off=0, **g)
        add(path + ".b", 0, pre + ".bias", None, BIAS, off=0, cout=O)
        for p in (path + ".wb",) + tuple(extra):  # 16 rows, rows >= O zero
            add(p, (16 - O) * K, pre + ".weight", None, PLAIN, off=0, **g)

    def tower(path, pres, names=("wf",)):
        """Residual convs back to back in the tower packing, one trailing pad; their folded biases back to back."""
        i = 0
        for pre in pres:
            for k in (1, 2):
                for nm in names:
                    add(f"{path}.{nm}", LAT_PAD_ELEMS, f"{pre}.conv{k}.weight", f"{pre}.bn{k}", LAT16,
                        off=i * 9 * c1 * c1, cout=c1, taps=9, cin_src=c1, c_used=c1, cin_dst=c1, tperm=1)
                add(f"{path}.b", 0, f"{pre}.conv{k}.bias", f"{pre}.bn{k}", BIAS, off=i * c1, cout=c1)
                i += 1

    lay = rep_layout(mcfg)
    cin, nconv = 2 * hist, 0
    for pos, (kind, i) in enumerate(lay):
        pre = f"rep_net.blocks.{i}"
        if kind == "conv":
            cout = c0 if nconv == 0 else c1
            conv(f"rep.{pos}.1", pre + ".weight", pre + ".bias", None, cin, cout, 3)
            cin, nconv = cout, nconv + 1
        elif kind == "res":
            res(f"rep.{pos}.1", pre, cin)
    nd, npred = mcfg["dynamics_network"]["num_res_blocks"], mcfg["prediction_network"]["num_res_blocks"]
    cb = "dyn_net.conv_block"
    conv("dyn0", cb + ".conv.weight", cb + ".conv.bias", cb + ".bn", c1, c1, 3, act=A)
    for i in range(nd):
        res(f"dyn.{i}", f"dyn_net.res_blocks.{i}", c1)
    for i in range(npred):
        res(f"pred.{i}", f"pred_net.res_blocks.{i}", c1)
    heads = (("rew", "dyn_net.reward_head", c1, 1, ns), ("pol", "pred_net.policy_head", c1 // 2, 3, na),
             ("val", "pred_net.value_head", c1 // 2, 1, ns))
    for nm, pre, co, ks, O in heads:
        conv(nm + "_conv", pre + ".0.conv.weight", pre + ".0.conv.bias", pre + ".0.bn", c1, co, ks)
        linear(nm + "_lin", pre + ".2", co, O, extra=("fused.dyn16.lw",) if nm == "rew" else ())
    tower("dyn_tower", [f"dyn_net.res_blocks.{i}" for i in range(nd)], ("wf", "wf16"))
    tower("pred_tower", [f"pred_net.res_blocks.{i}" for i in range(npred)])
    for nm in ("rep_tail", "rep_blocks"):
        if meta.get(nm) is not None:
            first, n = meta[nm]
            first += nm == "rep_tail"  # rep_tail's `first` is the pool in front of its blocks
            if any(lay[p][0] != "res" for p in range(first, first + n)):
                raise ValueError(f"refresh: {nm}: rep_layout positions {first}..{first + n - 1} are not residual blocks")
            tower(nm, [f"rep_net.blocks.{lay[p][1]}" for p in range(first, first + n)])
    # the fused steps' ConvBlock and head convs in the tower packings (PackedNets._fused), bf16 and the fp16 copies
    for pre in ("fused.", "fused.dyn16."):
        g = dict(cin_src=_pad8(c1 + A), c_used=c1, cin_dst=c1)
        add(pre + "w0", LAT_PAD_ELEMS, cb + ".conv.weight", cb + ".bn", LAT16, off=0, cout=c1, taps=9, tperm=1, **g)
        for nm, hp, co, ks, _ in heads:
            add(pre + nm[0] + "w", LAT_PAD_ELEMS, hp + ".0.conv.weight", hp + ".0.bn", LAT16, off=0, cout=co,
                taps=ks * ks, cin_src=c1, c_used=c1, cin_dst=c1, tperm=int(ks == 3))
            if pre == "fused.":
                add(pre + nm[0] + "b", 0, hp + ".0.conv.bias", hp + ".0.bn", BIAS, off=0, cout=co)
    check_coverage(tensors, jobs, pads)
    return jobs, pads


def check_coverage(tensors, jobs, pads):
    """Every tensor is written exactly once over [0, numel - pad): no gap, no overlap, nothing past the end."""
    by = {}
    for j in jobs:
        by.setdefault(j.path, []).append(j)
    for path, (numel, _) in tensors.items():
        if path not in by:
            raise NotImplementedError(f"refresh: no job writes pack tensor {path!r}: it would be left stale")
        end = 0
        for j in sorted(by[path], key=lambda j: j.off):
            if j.off != end:
                raise NotImplementedError(f"refresh: {path!r}: jobs leave a gap or overlap at element {end} "
                                          f"(next job starts at {j.off})")
            end = j.off + j.n
        if end != numel - pads[path]:
            raise NotImplementedError(f"refresh: {path!r}: jobs write {end} elements, the tensor holds "
                                      f"{numel} - {pads[path]} pad")


def check_config(a, b):
    for ks in CFG_KEYS:
        x, y = a, b
        for k in ks:
            x, y = x[k], y[k]
        if (list(x) if isinstance(x, (list, tuple)) else x) != (list(y) if isinstance(y, (list, tuple)) else y):
            raise ValueError(f"refresh: the learner and the pack differ in {'.'.join(ks)}: {x} vs {y}")


def _first_blocks(units):
    """first[i] = the first 256-thread workgroup of record i (+ the total as the last entry)."""
    first = np.zeros(len(units) + 1, np.int64)
    first[1:] = np.cumsum([(u + 255) // 256 for u in units])
    if first[-1] >= 2 ** 31:
        raise ValueError("refresh: too many workgroups for one launch")
    return first.astype(np.int32)


class RefreshTable:
    """The device job table for one (learner, pack) pair. Valid while the learner keeps its flat buffer and its
    running-stat tensors (Learner.load_state_dict replaces the latter: stale() then says so)."""

    def __init__(self, learner, pack):
        if pack.dtype != "bf16":
            raise ValueError("refresh: the device hand-off writes bf16 packs (an f32 pack goes through the host)")
        check_config(learner.m, pack.mcfg)
        dev = pack.device
        named = named_tensors(pack)
        meta = {nm: (getattr(pack, nm)["first"], getattr(pack, nm)["n"]) if getattr(pack, nm) is not None else None
                for nm in ("rep_tail", "rep_blocks")}
        jobs, _ = plan(pack.mcfg, OrderedDict((p, (t.numel(), t.dtype)) for p, t in named.items()), meta)
        self.learner_P, self.learner_run = learner.P, learner.run
        P, nflat = learner.P, learner.P.numel()
        base = P.data_ptr()
        # BatchNorm records: alpha / beta' of each into one f64 scratch buffer
        bn_off, n64 = OrderedDict(), 0
        for j in jobs:
            if j.bn is not None and j.bn not in bn_off:
                bn_off[j.bn] = n64
                n64 += 2 * learner.params[j.bn + ".weight"].n
        self.ab = torch.zeros(max(n64, 1), dtype=torch.float64, device=dev)
        bns = np.zeros(len(bn_off), BN_DT)
        for r, (bn, off) in zip(bns, bn_off.items()):
            g, b = learner.params[bn + ".weight"], learner.params[bn + ".bias"]
            rm, rv = learner.run[bn]
            if not (g.n == b.n == rm.numel() == rv.numel() and rm.dtype == rv.dtype == torch.float32
                    and rm.is_contiguous() and rv.is_contiguous() and g.off + g.n <= nflat and b.off + b.n <= nflat):
                raise ValueError(f"refresh: BatchNorm {bn}: parameter and running-stat sizes differ")
            r["gamma"], r["beta"] = base + 4 * g.off, base + 4 * b.off
            r["mean"], r["var"], r["out"], r["C"] = rm.data_ptr(), rv.data_ptr(), self.ab.data_ptr() + 8 * off, g.n
        # job records, every extent checked against its source parameter and its destination tensor
        recs = np.zeros(len(jobs), JOB_DT)
        self.bytes_read = self.bytes_written = 0
        for r, j in zip(recs, jobs):
            p, t = learner.params[j.key], named[j.path]
            src_n = j.cout if j.kind == BIAS else j.cout * j.taps * j.cin_src
            used = j.A if j.kind == ACT else j.c_used
            if src_n != p.n or p.off + p.n > nflat or (j.kind != BIAS and j.c_first + used > j.cin_src):
                raise ValueError(f"refresh: {j.path}: parameter {j.key} holds {p.n} elements, the job reads {src_n}")
            if j.off < 0 or j.off + j.n > t.numel() or not t.is_contiguous() or OTYPE[t.dtype] != j.otype:
                raise ValueError(f"refresh: {j.path}: job extent {j.off}+{j.n} outside the tensor ({t.numel()})")
            if j.kind in (BIAS, ACT) and t.dtype != torch.float32:
                raise ValueError(f"refresh: {j.path}: bias / action tables are f32")
            if (base + 4 * p.off) % 16 or t.data_ptr() % 16:
                raise ValueError(f"refresh: {j.path}: source or destination is not 16-byte aligned")
            r["w"], r["dst"], r["off"] = base + 4 * p.off, t.data_ptr(), j.off
            r["ab"] = self.ab.data_ptr() + 8 * bn_off[j.bn] if j.bn is not None else 0
            for f in ("kind", "otype", "cout", "taps", "cin_src", "c_first", "c_used", "cin_dst", "tperm", "H", "W", "A"):
                r[f] = getattr(j, f)
            self.bytes_read += 4 * (j.cout * j.taps * used if j.kind != BIAS else j.cout)
            self.bytes_written += j.n * t.element_size()
        self.jobs = jobs
        lib = L.lib()
        assert lib.mzba_pack_fold_job_bytes() == JOB_DT.itemsize and lib.mzba_pack_fold_bn_bytes() == BN_DT.itemsize
        up = lambda a: torch.from_numpy(a.view(np.uint8).copy()).to(dev)  # noqa: E731
        bn_first, job_first = _first_blocks([int(r["C"]) for r in bns]), _first_blocks([j.units() for j in jobs])
        self.nbn, self.njobs = len(bns), len(jobs)
        self.bn_blocks, self.job_blocks = int(bn_first[-1]), int(job_first[-1])
        self.d_bns, self.d_jobs = up(bns) if self.nbn else None, up(recs)
        self.d_bn_first, self.d_job_first = up(bn_first), up(job_first)

    def stale(self, learner):
        return learner.P is not self.learner_P or learner.run is not self.learner_run

    def run(self):
        """The refresh: every BatchNorm's fold terms, then every pack tensor, on the current stream."""
        s = L.stream()
        if self.nbn:
            L.call("mzba_pack_fold_bn", L.ptr(self.d_bns), L.ptr(self.d_bn_first), self.nbn, self.bn_blocks, s)
        L.call("mzba_pack_fold", L.ptr(self.d_jobs), L.ptr(self.d_job_first), self.njobs, self.job_blocks, s)
