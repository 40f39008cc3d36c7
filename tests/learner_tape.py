"""The learner's tape replayed in f64, layer by layer (test infrastructure: plain torch on the CPU).

A tape is what one `Learner.train_minibatch` with `keep_tape` left behind (`host_tape`), or the same layout written by
an f64 CPU forward (`cpu_tape`): every tensor a layer stored, as NHWC rows [B * H * W][C] in the storage type, the BN
`stats` rows (mean, invstd, alpha = gamma invstd, beta' = beta - mean alpha), the min-max scale's `mm` and NHWC `idx`,
the logits, the logit gradients and the gradient checkpoints (`gps[k]`, the prediction part of d h_k; `dh[k]`, d h_k
after the prediction part was added).

Forward audit (`audit_forward`): every stored tensor against the same op evaluated in f64 from the stored inputs of
that op and the parameters as they stood before the step; conv weights rounded to bf16 for a bf16 learner, Linear
weights and BN parameters f32. Bounds in the idiom of ops_bounds._check, e_k <= 4 e_w + c 2^-24 S (+ 2^-8 |ref| for a
bf16 output), e_w the error of a plain torch f32 CPU evaluation of the same op:

    conv t            c = taps Cin + 2 (the f32 accumulation as one serial chain, the bias, the cast) on
                      S = |bias| + sum |w| |x|
    BN stats          test_bn_stats's propagation with the chunk chains of the kernel that ran: mzba_bn_stats, c = 21
                      (mean) / 22 (M2) on max |t| / max (t - mean)^2; conv_lat's epilogue (fuse_bn) sums a chunk column
                      in MR / TPC serial adds, TPC more, a divide and a cast, MR <= 160 rows, TPC >= 2: c = 84 / 86.
                      The fused statistics are taken from the stored (bf16-rounded) t, as the separate passes take them
                      (csrc/conv_lat.hip: "the stored (bf16-rounded) values back into the tile for the column pass"), so
                      the fused rows need and get no allowance for t's rounding.
    running stats     the K uses of a BN folded in order, rm <- rm + 0.1 (mean - rm): the statistic's c S times 0.1, three
                      operations on |rm| per use; the unbiased variance M / (M - 1) var
    BN output y       relu(t alpha + beta' [+ res]) from the learner's own alpha / beta' rows: c = 3 on |t alpha| +
                      |beta'| + |res|
    avg-pool          c = 4 (three adds, the quarter) on the mean of |x|
    scale             mm equals the stored h at the stored idx and is the true min / max (exact); out against
                      (h - min) / (max - min + 1e-8): c = 4, S = 1
    Linear logits     c = 2 ceil(K / 256) + 9 on |bias| + sum |w x|
    input rows, dynamics input    exact (torch.equal): ring frames through the LUT and a / 3 planes; the latent bit for
                      bit, the one-hot planes of future_actions[:, k], zeros in the padding

Backward replay (`replay`): with the forward tape fixed the backward is a fixed linear map of the logit gradients. It is
evaluated in f64 in the order of Learner._minibatch_body from the tape's dlr / dlv / dlp, the stored forward tensors
(masks from stored y > 0, xhat from stored t and stats, scale routing from stored idx) and the same parameters, in
three forms: E (no rounding), R (every gradient tensor the learner stores in its activation type rounded to bf16,
nearest even: the Linear, BN, conv, scale and pool input gradients, the accumulations into `acc` and the axpy; the two
routed elements of a scale backward twice, as the kernel stores them twice) and D_s (the same points rounded
stochastically, seeded). `assert_backward` requires per parameter tensor and per checkpoint, in the 2-norm and in the
max norm, d = |g_kernel - g_E| <= 2 w, w = max(|g_R - g_E|, max_s |g_Ds - g_E|): the reference's own rounding spread,
doubled because a maximum over five samples underestimates its tail. Tensors whose replay crosses no stored bf16
gradient (w = 0: the three Linear heads' weights and biases) and every tensor of an f32 learner use the ops_bounds
idiom against an f32 witness (the f32 replay; for a bf16 learner's heads just their f32 contraction): Linear dw c = K (2 rps + nsplit + 2) on sum_k |dy_k|^T |x_k| (test_linear_
forward_backward's chain per step, the K accumulations), db with one operation per row; for f32 tensors further up the
bound is the witness term alone plus 2^-24 of the tensor's max (c S cannot be written per element through ~100 layers;
the f32 witness runs the same layers). Biases of convs that feed a BN have the exact gradient 0: f32 keeps
test_gpu_learner._check_grads's rule (<= 1e-4 max |dw|); in bf16 the gradient is the sum of the stored dt's roundings,
which is exactly what R and D_s hold, so the same d <= 2 w applies and bounds it at rounding-noise size.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from ops_bounds import _check

EPS32, MOM32 = float(np.float32(1e-5)), float(np.float32(0.1))
P_DITHER = 4


def _pad8(c):
    return (c + 7) // 8 * 8


def _img(rows, B):
    """NHWC rows [B * H * W][C] -> NCHW view; H x W from the row count (16 x 20, 8 x 10 or 4 x 5: all 4 : 5)."""
    hw = rows.shape[0] // B
    H = int(round(math.sqrt(hw * 4 / 5)))
    return rows.view(B, H, hw // H, rows.shape[1]).permute(0, 3, 1, 2)


def _rows(img):
    B, C, H, W = img.shape
    return img.permute(0, 2, 3, 1).reshape(B * H * W, C)


def rne_bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def dither_bf16(seed):
    """Stochastic rounding to bf16: up (away from zero) with probability (x - lo) / (hi - lo). The 16 dropped bits are
    compared with 16 bits of a seeded multiplicative hash of (element index, call number): cheap next to the convs."""
    calls = [0]

    def q(t):
        bits = t.float().contiguous().view(torch.int32)
        calls[0] += 1
        r = torch.arange(bits.numel(), dtype=torch.int64).view(bits.shape) + (seed * 1000003 + calls[0]) * 7919
        r = (r ^ (r >> 15)) * 0x2C1B3C6D
        r = (r ^ (r >> 12)) * 0x297A2D39
        r = ((r ^ (r >> 15)) >> 7) & 0xFFFF
        up = ((bits & 0xFFFF).to(torch.int64) > r).to(torch.int32)
        return ((bits & -65536) + (up << 16)).view(torch.float32).to(t.dtype)
    return q


def random_mb(B, L, K, seed):
    """The minibatch arrays of test_gpu_learner._random_ring (same generator, same draws)."""
    g = np.random.default_rng(seed)
    lut = np.array([0, 0.3, 0.6, 1.0], np.float32)
    return dict(states=lut[g.integers(0, 4, (B, L, 16, 20)) * (g.random((B, L, 16, 20)) < 0.3)],
                past_actions=g.integers(0, 3, (B, L)), future_actions=g.integers(0, 3, (B, K)),
                rewards=g.choice(np.array([-1, 0, 0, 1, 5], np.float32), (B, K)),
                targets=(g.normal(size=(B, K)) * 2).astype(np.float32),
                counts=g.multinomial(50, [0.3, 0.3, 0.4], (B, K)).astype(np.float32))


# ----------------------------------------------------------------------------------------- the nets' names
class Net:
    """Module names and shapes of the three nets of a model config (reference state-dict prefixes)."""

    def __init__(self, mcfg):
        from oracle.learner import rep_layout
        self.m = mcfg
        self.hist = mcfg["state_history_length"]
        self.c0, self.c1 = mcfg["latent_channels"]
        self.A = mcfg["dynamics_network"]["num_actions"]
        self.rep = [(kind, f"rep_net.blocks.{i}") for kind, i in rep_layout(mcfg)]
        self.dyn_res = [f"dyn_net.res_blocks.{i}" for i in range(mcfg["dynamics_network"]["num_res_blocks"])]
        self.pred_res = [f"pred_net.res_blocks.{i}" for i in range(mcfg["prediction_network"]["num_res_blocks"])]


class Params:
    """Parameters of a reference state dict in dtype fdt; 4-D (conv) weights through bf16 for a bf16 learner."""

    def __init__(self, sd, bf16, fdt=torch.float64):
        self.p = {}
        for k, v in sd.items():
            t = torch.as_tensor(np.asarray(v))
            if not t.is_floating_point():
                continue
            if bf16 and t.dim() == 4:
                t = t.float().to(torch.bfloat16)
            self.p[k] = t.to(fdt)

    def __getitem__(self, k):
        return self.p[k]


# ----------------------------------------------------------------------------------------- forward ops
def f_conv(P, pre, x):
    w = P[pre + ".weight"]
    return F.conv2d(x[:, :w.shape[1]], w, P[pre + ".bias"], padding=w.shape[2] // 2)


def f_stats(t, gamma, beta, eps):
    """(mean, invstd, alpha, beta') rows [4][C] and the unbiased variance of t (NCHW)."""
    mean = t.mean((0, 2, 3))
    var = t.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + eps)
    alpha = gamma * invstd
    n = t.numel() // t.shape[1]
    return torch.stack([mean, invstd, alpha, beta - mean * alpha]), var * (n / max(n - 1, 1))


def f_apply(t, s, res=None):
    y = t * s[2].view(1, -1, 1, 1) + s[3].view(1, -1, 1, 1)
    return torch.relu(y if res is None else y + res)


def f_scale(h, idx=None):
    """_scale_state on h (NCHW); idx [B][2] NHWC positions of (min, max) or None (the first in NHWC order).
    -> (out, mm [B][2], idx)."""
    B = h.shape[0]
    f = _rows(h).view(B, -1)
    if idx is None:
        idx = torch.stack([f.argmin(1), f.argmax(1)], 1)
    mm = f.gather(1, idx)
    mn, mx = mm[:, 0].view(B, 1, 1, 1), mm[:, 1].view(B, 1, 1, 1)
    return (h - mn) / (mx - mn + 1e-8), mm, idx


def f_linear(P, pre, x):
    return F.linear(x.flatten(1), P[pre + ".weight"], P[pre + ".bias"])


def f_input(net, mb, fdt):
    """mzba_learner_input's rows (NCHW): frames, past actions / 3, zero padding to a multiple of 8."""
    st = torch.as_tensor(np.asarray(mb["states"], np.float32)).to(fdt)
    B = st.shape[0]
    acts = torch.as_tensor(np.asarray(mb["past_actions"], np.int64)).to(fdt)
    x = torch.zeros(B, _pad8(2 * net.hist), 16, 20, dtype=fdt)
    x[:, :net.hist] = st.view(B, net.hist, 16, 20)
    x[:, net.hist:2 * net.hist] = (acts / 3)[:, :, None, None]
    return x


def f_dyn_input(net, h, a):
    B, _, H, W = h.shape
    x = torch.zeros(B, _pad8(net.c1 + net.A), H, W, dtype=h.dtype)
    x[:, :net.c1] = h
    x[:, net.c1:net.c1 + net.A] = F.one_hot(a, net.A).to(h.dtype).view(B, net.A, 1, 1)
    return x


# ----------------------------------------------------------------------------------------- tapes
def cpu_tape(mcfg, sd, mb, K, bf16=False):
    """One minibatch's forward in f64 on the CPU, recorded in the tape's layout (tensors f64; with bf16 every stored
    activation and the conv weights go through bf16, nearest even), the logit gradients from autograd of loss_fn."""
    from oracle.learner import kl_batchmean, supports_representation
    net, P = Net(mcfg), Params(sd, bf16)
    qa = rne_bf16 if bf16 else (lambda t: t)
    f64 = torch.float64

    def bn(pre, t, res=None):
        s, _ = f_stats(t, P[pre + ".weight"], P[pre + ".bias"], 1e-5)
        return s, qa(f_apply(t, s, res))

    def block(pre, x):
        t = qa(f_conv(P, pre + ".conv", x))
        s, y = bn(pre + ".bn", t)
        return y, dict(x=_rows(x), t=_rows(t), s=s, y=_rows(y))

    def res(pre, x):
        t1 = qa(f_conv(P, pre + ".conv1", x))
        s1, a1 = bn(pre + ".bn1", t1)
        t2 = qa(f_conv(P, pre + ".conv2", a1))
        s2, out = bn(pre + ".bn2", t2, x)
        return out, dict(x=_rows(x), t1=_rows(t1), a1=_rows(a1), s1=s1, t2=_rows(t2), s2=s2, out=_rows(out))

    def scale(h):
        out, mm, idx = f_scale(h)
        out = qa(out)
        return out, dict(h=_rows(h), mm=mm, idx=idx, out=_rows(out))

    x = qa(f_input(net, mb, f64))
    B = x.shape[0]
    T = dict(B=B, K=K, x=_rows(x), rep=[], steps=[])
    h = x
    for kind, pre in net.rep:
        if kind == "conv":
            T["rep"].append(dict(x=_rows(h)))
            h = qa(f_conv(P, pre, h))
        elif kind == "res":
            h, sv = res(pre, h)
            T["rep"].append(sv)
        else:
            T["rep"].append({})
            h = qa(F.avg_pool2d(h, 2, 2))
    h, T["rep_scale"] = scale(h)
    fut = torch.as_tensor(np.asarray(mb["future_actions"], np.int64))
    logits = {"lr": [], "lv": [], "lp": []}
    for k in range(K):
        st = dict(h=_rows(h))
        xp, pr = h, dict(res=[])
        for pre in net.pred_res:
            xp, sv = res(pre, xp)
            pr["res"].append(sv)
        yp, pr["pol"] = block("pred_net.policy_head.0", xp)
        pr["lp"] = f_linear(P, "pred_net.policy_head.2", yp)
        yv, pr["val"] = block("pred_net.value_head.0", xp)
        pr["lv"] = f_linear(P, "pred_net.value_head.2", yv)
        xin = f_dyn_input(net, h, fut[:, k])
        xd, dy = xin, dict(res=[])
        xd, dy["blk"] = block("dyn_net.conv_block", xd)
        for pre in net.dyn_res:
            xd, sv = res(pre, xd)
            dy["res"].append(sv)
        yr, dy["rew"] = block("dyn_net.reward_head.0", xd)
        dy["lr"] = f_linear(P, "dyn_net.reward_head.2", yr)
        h, dy["scale"] = scale(xd)
        st["pred"], st["dyn"] = pr, dy
        T["steps"].append(st)
        logits["lr"].append(dy["lr"]); logits["lv"].append(pr["lv"]); logits["lp"].append(pr["lp"])
    z = [torch.stack(logits[n]).detach().requires_grad_() for n in ("lr", "lv", "lp")]  # [K][B][n]
    s = (mcfg["supports_min"], mcfg["supports_max"], mcfg["num_supports"])
    rl = kl_batchmean(z[0].permute(1, 0, 2), supports_representation(
        torch.as_tensor(np.asarray(mb["rewards"], np.float32)).double(), *s))
    vl = kl_batchmean(z[1].permute(1, 0, 2), supports_representation(
        torch.as_tensor(np.asarray(mb["targets"], np.float32)).double(), *s))
    c = torch.as_tensor(np.asarray(mb["counts"], np.float32)).double()
    pl = kl_batchmean(z[2].permute(1, 0, 2), c / c.sum(-1, keepdim=True))
    ((1 / K) * (rl + vl + pl)).backward()
    T["dlr"], T["dlv"], T["dlp"] = (t.grad for t in z)
    return T


def force_index(T):
    """The tape's scale positions as LearnerOracle.force_index wants them: NCHW flatten indices, representation first."""
    out = []
    for sc in [T["rep_scale"]] + [st["dyn"]["scale"] for st in T["steps"]]:
        C = sc["h"].shape[1]
        hw = sc["h"].shape[0] // T["B"]
        i = sc["idx"].long().numpy()
        out.append((i % C) * hw + i // C)
    return out


def host_tape(ln):
    """`ln.last_tape` (a Learner with keep_tape after a minibatch) as CPU tensors in the tape's layout."""
    torch.cuda.synchronize()
    tp = ln.last_tape

    def c(t):
        return t.detach().cpu()

    def blk(sv):
        x, t, s, y = sv
        return dict(x=c(x.t), t=c(t), s=c(s), y=c(y.t))

    def res(sv):
        x, t1, a1, s1, t2, s2, out = sv
        return dict(x=c(x.t), t1=c(t1), a1=c(a1.t), s1=c(s1), t2=c(t2), s2=c(s2), out=c(out.t))

    def scale(sc, out):
        h, mm, idx = sc
        return dict(h=c(h), mm=c(mm), idx=c(idx).long(), out=c(out))

    rtape, rsc = tp["rep_saved"]
    rep = []
    for kind, mod, sv in rtape:
        rep.append(dict(x=c(sv[0].t)) if kind == "conv" else res(sv[0]) if kind == "res" else {})
    lat = tp["latents"]
    lr_all, lv_all, lp_all = ln.last_logits
    steps = []
    for k, (pu, du) in enumerate(tp["unroll"]):
        pr = dict(res=[res(s) for s in pu["psv"]], pol=blk(pu["spol"]), val=blk(pu["sval"]), lp=c(lp_all[k]),
                  lv=c(lv_all[k]))
        dy = dict(blk=blk(du["sblk"]), res=[res(s) for s in du["dsv"]], rew=blk(du["srew"]), lr=c(lr_all[k]),
                  scale=scale(du["ssc"], lat[k + 1]))
        steps.append(dict(h=c(lat[k]), pred=pr, dyn=dy))
    return dict(B=tp["dlr"].shape[1], K=len(steps), x=c(tp["x"]), rep=rep, rep_scale=scale(rsc, lat[0]), steps=steps,
                dlr=c(tp["dlr"]), dlv=c(tp["dlv"]), dlp=c(tp["dlp"]), gps=[c(t) for t in tp["gps"]],
                dh=[c(t) for t in tp["dh"]])


# ----------------------------------------------------------------------------------------- forward audit
def audit_forward(mcfg, T, sd_before, sd_after, ring, slots, lut, bf16, fused):
    """Every stored forward tensor of tape T against f64 (module docstring). ring: the replay arrays on the CPU
    (states codes, past_actions, future_actions); slots: the windows' rows; lut: the frame LUT; fused(Cin, Cout, ks, H, W) says
    whether that conv's BN statistics came from conv_lat's epilogue. sd_after None: the running statistics are not
    checked (a CPU tape has none). Returns the number of tensors checked."""
    net = Net(mcfg)
    P64, P32 = Params(sd_before, bf16), Params(sd_before, bf16, torch.float32)
    B, K = T["B"], T["K"]
    n = [0]
    run = {}  # bn prefix -> [rm64, rv64, rm32, rv32, cs_rm, cs_rv, uses]

    def chk(name, got, ref, wit, cS, out_bf16=False):
        n[0] += 1
        _check(name, got, ref, wit, cS, out_bf16=out_bf16)

    def im(rows, dt=torch.float64):
        return _img(rows.to(dt), B)

    def conv(name, pre, x, t):
        w64 = P64[pre + ".weight"]
        ref = f_conv(P64, pre, im(x))
        wit = f_conv(P32, pre, im(x, torch.float32))
        S = F.conv2d(im(x)[:, :w64.shape[1]].abs(), w64.abs(), P64[pre + ".bias"].abs(), padding=w64.shape[2] // 2)
        c = w64.shape[1] * w64.shape[2] * w64.shape[3] + 2
        chk(name + " conv", _img(t, B), ref, wit, c * S, out_bf16=bf16)

    def bn(name, pre, cpre, t, s, y, res=None):
        t64 = im(t)
        C = t64.shape[1]
        M = t64.numel() // C
        w = P64[cpre + ".weight"]
        cm, cv = (84, 86) if fused(_pad8(w.shape[1]), C, w.shape[2], t64.shape[2], t64.shape[3]) else (21, 22)
        gamma, beta = P64[pre + ".weight"], P64[pre + ".bias"]
        ref, unb = f_stats(t64, gamma, beta, EPS32)
        wit, unb_w = f_stats(im(t, torch.float32), P32[pre + ".weight"], P32[pre + ".bias"], 1e-5)
        mean, invstd, alpha = ref[0], ref[1], ref[2]
        Sx = t64.abs().amax((0, 2, 3))
        Sv = ((t64 - mean.view(1, -1, 1, 1)) ** 2).amax((0, 2, 3))
        cs_mean = cm * Sx
        cs_var = cv * Sv + 2 * Sv.sqrt() * cs_mean
        cs_invstd = 0.5 * invstd ** 3 * cs_var + 2 * invstd
        cs_alpha = gamma.abs() * cs_invstd + alpha.abs()
        cs_betap = alpha.abs() * cs_mean + mean.abs() * cs_alpha + 2 * (beta.abs() + (mean * alpha).abs())
        for i, (nm, cs) in enumerate((("mean", cs_mean), ("invstd", cs_invstd), ("alpha", cs_alpha), ("beta'", cs_betap))):
            chk(f"{name} stats {nm}", s[i], ref[i], wit[i], cs)
        if pre not in run:
            rm, rv = P64[pre + ".running_mean"], P64[pre + ".running_var"]
            run[pre] = [rm, rv, rm.float(), rv.float(), torch.zeros_like(rm), torch.zeros_like(rv), 0]
        r = run[pre]
        r[0] = MOM32 * ref[0] + (1 - MOM32) * r[0]
        r[1] = MOM32 * unb + (1 - MOM32) * r[1]
        r[2] = 0.1 * wit[0] + (1 - 0.1) * r[2]
        r[3] = 0.1 * unb_w + (1 - 0.1) * r[3]
        r[4] = (1 - MOM32) * r[4] + MOM32 * cs_mean + 3 * r[0].abs()
        r[5] = (1 - MOM32) * r[5] + MOM32 * cs_var * (M / max(M - 1.0, 1.0)) + 3 * r[1].abs()
        r[6] += 1
        # the output from the learner's own alpha / beta' rows
        s64 = s.double()
        rr = None if res is None else im(res)
        ref_y = f_apply(t64, s64, rr)
        wit_y = f_apply(im(t, torch.float32), s.float(), None if res is None else im(res, torch.float32))
        S = (t64 * s64[2].view(1, -1, 1, 1)).abs() + s64[3].abs().view(1, -1, 1, 1) + (0 if rr is None else rr.abs())
        chk(f"{name} y", _img(y, B), ref_y, wit_y, 3 * S, out_bf16=bf16)

    def block(name, pre, sv):
        conv(name, pre + ".conv", sv["x"], sv["t"])
        bn(name, pre + ".bn", pre + ".conv", sv["t"], sv["s"], sv["y"])

    def res(name, pre, sv):
        conv(name + " 1", pre + ".conv1", sv["x"], sv["t1"])
        bn(name + " 1", pre + ".bn1", pre + ".conv1", sv["t1"], sv["s1"], sv["a1"])
        conv(name + " 2", pre + ".conv2", sv["a1"], sv["t2"])
        bn(name + " 2", pre + ".bn2", pre + ".conv2", sv["t2"], sv["s2"], sv["out"], res=sv["x"])

    def scale(name, sc):
        h = sc["h"]
        f = h.view(B, -1)
        mm = f.gather(1, sc["idx"]).float()
        smm = sc["mm"].float()
        assert torch.equal(mm, smm), name + ": mm is not h at idx"
        assert torch.equal(smm[:, 0], f.float().amin(1)) and torch.equal(smm[:, 1], f.float().amax(1)), name
        n[0] += 2
        ref = f_scale(im(h), sc["idx"])[0]
        wit = f_scale(im(h, torch.float32), sc["idx"])[0]
        chk(name + " out", _img(sc["out"], B), ref, wit, 4.0, out_bf16=bf16)

    def linear(name, pre, x, got):
        Kd = x.shape[0] // B * x.shape[1]
        ref = f_linear(P64, pre, im(x))
        wit = f_linear(P32, pre, im(x, torch.float32))
        S = P64[pre + ".bias"].abs() + im(x).flatten(1).abs() @ P64[pre + ".weight"].abs().t()
        chk(name + " logits", got, ref, wit, (2 * math.ceil(Kd / 256) + 9) * S)

    def same(a, b, what):
        n[0] += 1
        assert a.dtype == b.dtype and torch.equal(a, b), what

    sdt = T["x"].dtype

    def store(t):  # through the storage type, in the tape's dtype (a CPU tape holds storage values in f64)
        return (t.to(torch.bfloat16) if bf16 else t.float()).to(sdt)
    sl = slots.long().cpu()
    # input rows: the ring's frames through the LUT, the past actions / 3, padding zero
    hist = net.hist
    exp = torch.zeros(B, 320, _pad8(2 * hist))
    exp[:, :, :hist] = torch.as_tensor(lut)[(ring["states"][sl].long() & 7)].reshape(B, hist, 320).permute(0, 2, 1)
    exp[:, :, hist:2 * hist] = (ring["past_actions"][sl].float() / 3.0)[:, None, :]
    same(T["x"], store(exp.reshape(B * 320, -1)), "input rows")
    # representation: an entry's output is the next entry's input (the scale's h after the last)
    ins = []
    for (kind, pre), sv in zip(net.rep, T["rep"]):
        ins.append(sv["x"] if kind != "pool" else None)
    for i, ((kind, pre), sv) in enumerate(zip(net.rep, T["rep"])):
        nxt = ins[i + 1] if i + 1 < len(ins) else T["rep_scale"]["h"]
        if kind == "conv":
            assert nxt is not None
            conv(pre, pre, sv["x"], nxt)
        elif kind == "res":
            res(pre, pre, sv)
            if nxt is not None:
                same(sv["out"], nxt, pre + ": the block's output feeds the next layer")
        else:
            x = T["rep"][i - 1]["out"]
            assert nxt is not None
            ref, wit = F.avg_pool2d(im(x), 2, 2), F.avg_pool2d(im(x, torch.float32), 2, 2)
            chk(pre + " pool", _img(nxt, B), ref, wit, 4 * F.avg_pool2d(im(x).abs(), 2, 2), out_bf16=bf16)
    scale("rep scale", T["rep_scale"])
    h = T["rep_scale"]["out"]
    fut = ring["future_actions"][sl]
    for k, st in enumerate(T["steps"]):
        tag = f"k{k} "
        same(st["h"], h, tag + "latent")
        pr, dy = st["pred"], st["dyn"]
        xp = h
        for pre, sv in zip(net.pred_res, pr["res"]):
            same(sv["x"], xp, tag + pre + " input")
            res(tag + pre, pre, sv)
            xp = sv["out"]
        for head, key, lin in (("pol", "lp", "pred_net.policy_head"), ("val", "lv", "pred_net.value_head")):
            same(pr[head]["x"], xp, tag + lin + " input")
            block(tag + lin, lin + ".0", pr[head])
            linear(tag + lin, lin + ".2", pr[head]["y"], pr[key])
        xin = store(_rows(f_dyn_input(net, im(h), fut[:, k])))
        same(dy["blk"]["x"], xin, tag + "dynamics input")
        block(tag + "dyn_net.conv_block", "dyn_net.conv_block", dy["blk"])
        xd = dy["blk"]["y"]
        for pre, sv in zip(net.dyn_res, dy["res"]):
            same(sv["x"], xd, tag + pre + " input")
            res(tag + pre, pre, sv)
            xd = sv["out"]
        same(dy["rew"]["x"], xd, tag + "reward head input")
        block(tag + "dyn_net.reward_head", "dyn_net.reward_head.0", dy["rew"])
        linear(tag + "dyn_net.reward_head", "dyn_net.reward_head.2", dy["rew"]["y"], dy["lr"])
        same(dy["scale"]["h"], xd, tag + "scale input")
        scale(tag + "dyn scale", dy["scale"])
        h = dy["scale"]["out"]
    for pre, (rm, rv, rm_w, rv_w, cs_rm, cs_rv, uses) in run.items() if sd_after is not None else ():
        chk(pre + " running_mean", torch.as_tensor(np.asarray(sd_after[pre + ".running_mean"])), rm, rm_w, cs_rm)
        chk(pre + " running_var", torch.as_tensor(np.asarray(sd_after[pre + ".running_var"])), rv, rv_w, cs_rv)
        d = int(np.asarray(sd_after[pre + ".num_batches_tracked"])) - int(np.asarray(sd_before[pre + ".num_batches_tracked"]))
        assert d == uses, (pre, d, uses)
    return n[0]


# ----------------------------------------------------------------------------------------- backward replay
class _Replay:
    def __init__(self, mcfg, T, sd, bf16, q, fdt, mut):
        self.net, self.T, self.P = Net(mcfg), T, Params(sd, bf16, fdt)
        self.q = q if q is not None else (lambda t: t)
        self.fdt, self.mut, self.B = fdt, set(mut), T["B"]
        self.g = {}

    def im(self, rows):
        return _img(rows.to(self.fdt), self.B)

    def acc(self, key, v):
        self.g[key] = self.g[key] + v if key in self.g else v

    def bn_bwd(self, pre, dy, y, t, s, k):
        g = dy * (self.im(y) > 0)
        t, s = self.im(t), s.to(self.fdt)
        v = lambda r: r.view(1, -1, 1, 1)  # noqa: E731
        xhat = (t - v(s[0])) * v(s[1])
        n = g.numel() // g.shape[1]
        sg, sgx = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
        self.acc(pre + ".weight", sgx * (2 if ("dgamma2", pre, k) in self.mut else 1))
        self.acc(pre + ".bias", sg)
        return g, self.q(v(s[2]) * (g - v(sg / n) - xhat * v(sgx / n)))

    def dgrad(self, pre, dt, cu=None):
        w = self.P[pre + ".weight"]
        if cu is not None:
            w = w[:, :cu]
        return F.conv_transpose2d(dt, w, padding=w.shape[2] // 2)

    def wgrad(self, pre, x, dt, k):
        if ("misswg", pre, k) in self.mut:
            return
        w = self.P[pre + ".weight"]
        x = self.im(x)[:, :w.shape[1]]
        self.acc(pre + ".weight", torch.nn.grad.conv2d_weight(x, w.shape, dt, padding=w.shape[2] // 2))
        self.acc(pre + ".bias", dt.sum((0, 2, 3)))

    def res_bwd(self, pre, sv, g, k):
        mask_y = sv["a1"] if ("mask", pre, k) in self.mut else sv["out"]
        g, dt2 = self.bn_bwd(pre + ".bn2", g, mask_y, sv["t2"], sv["s2"], k)
        da1 = self.q(self.dgrad(pre + ".conv2", dt2))
        self.wgrad(pre + ".conv2", sv["a1"], dt2, k)
        _, dt1 = self.bn_bwd(pre + ".bn1", da1, sv["a1"], sv["t1"], sv["s1"], k)
        dx = self.dgrad(pre + ".conv1", dt1)
        g = self.q(dx if ("skip", pre, k) in self.mut else g + dx)
        self.wgrad(pre + ".conv1", sv["x"], dt1, k)
        return g

    def block_bwd(self, pre, sv, g, k, acc=None, cu=None):
        _, dt = self.bn_bwd(pre + ".bn", g, sv["y"], sv["t"], sv["s"], k)
        dx = self.dgrad(pre + ".conv", dt, cu)
        out = self.q(dx if acc is None else acc + dx)
        self.wgrad(pre + ".conv", sv["x"], dt, k)
        return out

    def linear_bwd(self, pre, x, dy):
        x = self.im(x)
        dy = dy.to(self.fdt)
        self.acc(pre + ".weight", dy.t() @ x.flatten(1))
        self.acc(pre + ".bias", dy.sum(0))
        return self.q((dy @ self.P[pre + ".weight"]).view(x.shape))

    def scale_bwd(self, sc, dy, acc=None):
        """d h of (h - min) / (max - min + 1e-8), min / max at the stored idx: dy / den everywhere (stored), then the
        routed terms added to the two stored positions (stored again)."""
        B = self.B
        h = self.im(sc["h"])
        shape = h.shape
        hf, dyf = _rows(h).view(B, -1), _rows(dy).view(B, -1)
        idx = sc["idx"]
        mn, mx = hf.gather(1, idx[:, :1]), hf.gather(1, idx[:, 1:2])
        den = mx - mn + 1e-8
        base = dyf / den
        if acc is not None:
            base = base + _rows(acc).view(B, -1)
        base = self.q(base)
        s1, s2 = dyf.sum(1, keepdim=True), (dyf * (hf - mn)).sum(1, keepdim=True)
        add = torch.zeros_like(base)
        add.scatter_add_(1, idx[:, :1], -s1 / den + s2 / den ** 2)
        add.scatter_add_(1, idx[:, 1:2], -s2 / den ** 2)
        routed = self.q(base.gather(1, idx) + add.gather(1, idx))
        base = base.scatter(1, idx, routed)
        C = shape[1]
        return base.view(B, shape[2], shape[3], C).permute(0, 3, 1, 2)

    def run(self):
        T, net, K = self.T, self.net, self.T["K"]
        gps, dhs = [None] * K, [None] * K
        for k in reversed(range(K)):
            pr = T["steps"][k]["pred"]
            dyv = self.linear_bwd("pred_net.value_head.2", pr["val"]["y"], T["dlv"][k])
            gp = self.block_bwd("pred_net.value_head.0", pr["val"], dyv, k)
            dyp = self.linear_bwd("pred_net.policy_head.2", pr["pol"]["y"], T["dlp"][k])
            gp = self.block_bwd("pred_net.policy_head.0", pr["pol"], dyp, k, acc=gp)
            for pre, sv in reversed(list(zip(net.pred_res, pr["res"]))):
                gp = self.res_bwd(pre, sv, gp, k)
            gps[k] = gp
        gh = None
        for k in reversed(range(K)):
            dy = T["steps"][k]["dyn"]
            gx = self.scale_bwd(dy["scale"], gh) if gh is not None else None
            dyr = self.linear_bwd("dyn_net.reward_head.2", dy["rew"]["y"], T["dlr"][k])
            gx = self.block_bwd("dyn_net.reward_head.0", dy["rew"], dyr, k, acc=gx)
            for pre, sv in reversed(list(zip(net.dyn_res, dy["res"]))):
                gx = self.res_bwd(pre, sv, gx, k)
            gh = self.block_bwd("dyn_net.conv_block", dy["blk"], gx, k, cu=net.c1)
            if ("nopred", k) not in self.mut:
                gh = self.q(gh + gps[k])
            dhs[k] = gh
        gx = self.scale_bwd(T["rep_scale"], gh)
        for i in reversed(range(len(net.rep))):
            (kind, pre), sv = net.rep[i], T["rep"][i]
            if kind == "pool":
                gx = self.q(F.interpolate(gx, scale_factor=2, mode="nearest") / 4)
            elif kind == "res":
                gx = self.res_bwd(pre, sv, gx, None)
            else:
                self.wgrad(pre, sv["x"], gx, None)
                gx = self.q(self.dgrad(pre, gx)) if i > 0 else None
        for tag in self.mut:
            if tag[0] == "dwx2":
                self.g[tag[1]] = 2 * self.g[tag[1]]
        return self.g, [_rows(t) for t in gps], [_rows(t) for t in dhs]


def replay(mcfg, T, sd, bf16, q=None, fdt=torch.float64, mut=()):
    """The backward of tape T as the linear map of its logit gradients -> (reference-layout gradients, gps, dh)."""
    with torch.no_grad():
        return _Replay(mcfg, T, sd, bf16, q, fdt, mut).run()


def witnesses(mcfg, T, sd, bf16):
    """(E, W, wit32), each a `flat` dict: the f64 replay; for a bf16 learner R and P_DITHER dithered replays (else
    none); the f32 witness: the whole replay in f32 for an f32 learner, for a bf16 learner only the tensors that use
    it, the Linear heads' contractions."""
    E = flat(replay(mcfg, T, sd, bf16))
    if not bf16:
        return E, [], flat(replay(mcfg, T, sd, bf16, fdt=torch.float32))
    W = [flat(replay(mcfg, T, sd, bf16, q=rne_bf16))]
    W += [flat(replay(mcfg, T, sd, bf16, q=dither_bf16(1000 + s))) for s in range(P_DITHER)]
    wit32 = {}
    for pre, (dl, net, blk) in _HEAD_IN.items():
        x = [_img(T["steps"][k][net][blk]["y"].float(), T["B"]).flatten(1) for k in range(T["K"])]
        dy = [T[dl][k].float() for k in range(T["K"])]
        wit32[pre + ".weight"] = sum(d.t() @ v for d, v in zip(dy, x)).double()
        wit32[pre + ".bias"] = sum(d.sum(0) for d in dy).double()
    return E, W, wit32


def flat(out):
    """(grads, gps, dh) -> one dict name -> f64 tensor."""
    g, gps, dh = out
    d = {k: v.double() for k, v in g.items()}
    d.update({f"gps[{k}]": v.double() for k, v in enumerate(gps)})
    d.update({f"dh[{k}]": v.double() for k, v in enumerate(dh)})
    return d


def _pre_bn_bias(k):
    return k.endswith((".conv1.bias", ".conv2.bias", ".conv.bias"))


# Linear head -> (its logit gradient, the net and the block whose output it reads)
_HEAD_IN = {"dyn_net.reward_head.2": ("dlr", "dyn", "rew"), "pred_net.policy_head.2": ("dlp", "pred", "pol"),
            "pred_net.value_head.2": ("dlv", "pred", "val")}
HEADS = tuple(_HEAD_IN)


def _head_cs(T, key):
    """c S of a Linear head's accumulated dw / db: test_linear_forward_backward's chain per step plus the accumulate."""
    B, K = T["B"], T["K"]
    pre, leaf = key.rsplit(".", 1)
    dl, net, blk = _HEAD_IN[pre]
    nsplit = 16 if B >= 64 else 1
    rps = (B + nsplit - 1) // nsplit
    S = 0
    for k in range(K):
        dy = T[dl][k].double().abs()
        x = _img(T["steps"][k][net][blk]["y"].double(), B).flatten(1).abs()
        S = S + (dy.t() @ x if leaf == "weight" else dy.sum(0))
    return K * ((2 if leaf == "weight" else 1) * rps + nsplit + 2) * S


def assert_backward(got, E, W, wit32, T, bf16, margin=2.0, label=""):
    """The assertion of the module docstring on every tensor of `got` (a `flat` dict: the learner's gradients and
    checkpoints). Prints d / w per tensor; returns (largest d / w, largest w / |g_E|) over the tensors judged by w."""
    assert set(got) == set(E), sorted(set(got) ^ set(E))
    worst, spread, fails = 0.0, 0.0, []
    for k in sorted(E):
        g, e = got[k].double(), E[k]
        assert g.shape == e.shape and torch.isfinite(g).all(), k
        if bf16:
            d2, dm = (g - e).norm().item(), (g - e).abs().max().item()
            w2 = max((w[k] - e).norm().item() for w in W)
            wm = max((w[k] - e).abs().max().item() for w in W)
        else:
            w2 = wm = 0.0
        if w2 == 0.0:
            if _pre_bn_bias(k):  # f32: exact gradient 0, rounding-noise sized against the weight gradient
                wmax = E[k[:-len("bias")] + "weight"].abs().max().item()
                print(f"{label}{k}: |g| {g.abs().max().item():.3e} vs 1e-4 max|dw| {1e-4 * wmax:.3e}")
                if g.abs().max().item() > 1e-4 * wmax:
                    fails.append((k, g.abs().max().item(), 1e-4 * wmax))
            elif k.rsplit(".", 1)[0] in HEADS:
                _check(label + k, g, e, wit32[k], _head_cs(T, k))
            else:  # f32 learner: the f32 replay of the same layers as witness
                assert not bf16, (k, "w == 0 on a tensor below a stored bf16 gradient")
                _check(label + k, g, e, wit32[k], e.abs().max().item())
            continue
        r2, rm = d2 / w2, dm / wm
        nE = e.norm().item()
        print(f"{label}{k}: d/w {r2:.3f} (2-norm) {rm:.3f} (max)  w/|E| {w2 / nE if nE else float('inf'):.4f}")
        worst = max(worst, r2, rm)
        if not _pre_bn_bias(k) and nE:
            spread = max(spread, w2 / nE)
        if r2 > margin or rm > margin:
            fails.append((k, r2, rm))
    print(f"{label}largest d/w {worst:.3f}, largest w/|g_E| {spread:.4f}")
    assert not fails, fails
    return worst, spread
