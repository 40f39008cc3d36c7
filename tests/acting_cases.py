"""Seeded inputs, f64 references, f32 witnesses and c S terms for the acting side's small kernels (csrc/heads.hip: the
three heads forms and the support decode; csrc/conv.hip: min-max scale, avg-pool forward, the generic conv), shared by
tests/test_gpu_acting_ops.py (the kernels against them) and tests/test_cpu_acting_cases.py (the cases are not vacuous:
reference alone, no GPU). Plain torch on the CPU; nothing here calls the library. Every input is already rounded to
its storage type; the reference is evaluated in f64 from those values, the witness op by op in f32.

c (the f32 operations on the longest dependent chain) is counted from the kernel sources and restated here once per
kernel, so both test files use the same number. An MFMA's internal order is undocumented: every product it sums counts
as one operation."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from ops_bounds import BF, U, _gen

TINY = 2.0 ** -126  # the smallest normal f32: below it a kernel may flush to zero or round on the denormal grid
SMIN, SMAX = -5.0, 5.0
C999 = float(np.float32(1 - 0.001))  # the inverse transform's constant as f32 holds it (kernel and reference alike)


def tdt(dtype):
    return torch.bfloat16 if dtype else torch.float32


# ====================================================================== heads
HEAD_FORMS = ("f32_fma", "f32_mfma", "bf16_fma", "bf16_mfma")
HEAD_B = (1, 8, 9, 16, 17, 37)  # tile edges of the 8-env (FMA) and 16-env (MFMA) workgroups
HEAD_BMAX = 37
# f32 MFMA: 1 / 17 / 320 steps of 16 k; bf16 MFMA: 1 / 9 / 160 steps of 32 k (fewer than the 8 waves; no multiple of 8)
HEAD_K = {"f32_fma": (16, 272, 5120), "f32_mfma": (16, 272, 5120), "bf16_fma": (32, 288, 5120),
          "bf16_mfma": (32, 288, 5120)}
HEAD_K_FALLBACK = 40  # K % 16 != 0: mzba_heads' f32 MFMA form hands over to the FMA form
HEAD_O = (2, 3, 11, 16)
HEAD_REGIMES = ("random", "gaps")
# (heads of a launch as (O, decode, logits written)): two heads and one head per launch, logits null for one head,
# every O both decoded as supports (1) and as a policy (0)
HEAD_LAUNCHES = (((11, 1, True), (3, 0, True)), ((16, 1, True), (2, 0, False)), ((2, 1, True),), ((16, 0, False),),
                 ((3, 1, False), (11, 0, True)))


def heads_c(form, K):
    """heads_kernel (both FMA forms): a thread's ceil(K / 256) multiply-adds, the wave's 6 shuffle adds, 2 for the four
    waves, the bias. heads_mfma_f32_kernel: a wave's ceil(K / 16 / 8) steps put 4 products each into one accumulator,
    (a0 + a1) + (a2 + a3), 5 adds over the eight waves' partials, the bias. heads_mfma_kernel: ceil(K / 32 / 8) MFMAs of
    32 products, 8 adds over the waves, the bias."""
    if form in ("f32_fma", "bf16_fma"):
        return 2 * math.ceil(K / 256) + 9
    if form == "f32_mfma":
        return 4 * math.ceil(K / 16 / 8) + 8
    assert form == "bf16_mfma"
    return 32 * math.ceil(K / 32 / 8) + 9


@functools.lru_cache(maxsize=None)
def head_case(form, K, O, regime, tag=0):
    """x [37][K] in the form's activation type, w [O][K] (bf16 for the bf16 MFMA form, else f32), bias [O].
    "random": weights 0.02 N(0, 1), bias 0.1 N(0, 1) plus a ramp from 0 to 1 over the outputs (at K = 16 the logits are
    nearly uniform without it and the decoded x falls into the jump at 0, see x_gap_ok). "gaps": output o uses the weight row and the bias 150 g of its group
    g = min(o, 2): logits of different groups lie 150 apart (exp underflows to an exact zero), the outputs from 2 on tie
    at the top (their supports' mean is not 0 for any O here, so the decoded x stays clear of the jump at 0)."""
    g = _gen(31, HEAD_FORMS.index(form), K, O, HEAD_REGIMES.index(regime), tag)
    x = torch.randn(HEAD_BMAX, K, generator=g).to(torch.bfloat16 if form.startswith("bf16") else torch.float32)
    w = 0.02 * torch.randn(O, K, generator=g)
    bias = 0.1 * torch.randn(O, generator=g) + torch.linspace(0.0, 1.0, O)
    if regime == "gaps":
        grp = torch.arange(O).clamp(max=2)
        w, bias = w[grp].contiguous(), 150.0 * grp.float()
    if form == "bf16_mfma":
        w = w.bfloat16()
    return x, w, bias


def head_logits_ref(x, w, bias, kmax=None):
    """f64 x . W^T + b, its f32 witness, and S = |b| + sum |x w|; kmax drops the products from k = kmax on."""
    x64, w64 = x.double(), w.double()
    if kmax is not None:
        x64, w64 = x64[:, :kmax], w64[:, :kmax]
    ref = x64 @ w64.t() + bias.double()
    S = x64.abs() @ w64.abs().t() + bias.double().abs()
    wit = x.float() @ w.float().t() + bias
    return ref, wit, S


def _softmax64(l):
    """f64 softmax of f32 logits l with the relative error (in 2^-24) of a kernel's e_i / s: l - max rounds once, |d| of
    which exp amplifies, expf is within 2 ulp: a_i = |d_i| + 2; s carries sum p_j a_j and its n - 1 adds; the quotient
    rounds once. An entry at -inf has p = 0 exactly and no error."""
    l64 = l.double()
    d = l64 - l64.max(-1, keepdim=True)[0]
    e = d.exp()
    p = e / e.sum(-1, keepdim=True)
    a = torch.where(p > 0, d.abs() + 2.0, torch.zeros_like(p))
    rel = a + (p * a).sum(-1, keepdim=True) + (l.shape[-1] - 1) + 1.0
    return p, rel


def softmax_ref(l):
    """The policy softmax of the logits a launch wrote: f64 reference, torch f32 witness, c S = p rel + 2^-126 / 2^-24
    (an entry below the normal range is flushed or lands on the denormal grid)."""
    p, rel = _softmax64(l)
    return p, torch.softmax(l.float(), -1), p * rel + TINY / U


def decode_ref(l, smin=SMIN, smax=SMAX):
    """ScalarTransforms.inverted_softmax_expectation of f32 logits l [..., n] in f64 over the f32 values of
    torch.linspace(smin, smax, n); the reference's own f32 chain as the witness; c S; and x, the expectation.

    decode_support: q_i = e_i / s (rel as in _softmax64), sup_i = smin + i step with step = (smax - smin) / (n - 1): the
    quotient rounds twice, i step once, the add once: |sup_i - linspace_i| <= 2^-24 (3 |i step| + |sup_i|), which also
    covers the one f32 ulp by which smin + i step and torch.linspace's upper half (smax - (n - 1 - i) step) differ at
    n = 12 or 16 (numerics). x = sum q_i sup_i: a product and n adds on top: c S_x = sum p_i |sup_i| (rel_i + 1
    + n) + sum p_i (3 |i step| + |sup_i|) + 2^-126 / 2^-24 sum |sup|. Then t = |x| + 0.999, t t - 1: the error of x is
    amplified by 2 t = 2 (|x| + 0.999); the add rounds (2 t t), the square (t t), the subtraction (|t t - 1|)."""
    n = l.shape[-1]
    sup = torch.linspace(smin, smax, n)
    p, rel = _softmax64(l)
    sup64 = sup.double()
    x = (p * sup64).sum(-1)
    t = x.abs() + C999
    ref = torch.sign(x) * (t * t - 1.0)
    step = (smax - smin) / (n - 1)
    dsup = 3.0 * (torch.arange(n, dtype=torch.float64) * step).abs() + sup64.abs()
    cs_x = (p * sup64.abs() * (rel + 1.0 + n)).sum(-1) + (p * dsup).sum(-1) + TINY / U * sup64.abs().sum()
    cS = 2.0 * t * cs_x + 3.0 * t * t + (t * t - 1.0).abs()
    xw = (torch.softmax(l.float(), -1) * sup).sum(-1)
    wit = torch.sign(xw) * ((xw.abs() + (1 - 0.001)) ** 2 - 1)
    return ref, wit, cS, x


# ====================================================================== support decode rows
DECODE_N = (2, 11, 16)
DECODE_ROWS = (1, 255, 256, 257)  # one row; around the 256-thread block


@functools.lru_cache(maxsize=None)
def decode_rows(n, rows):
    """rows x n f32 logits: 3 N(0, 1) rows, and as the last rows (so at 257 rows the second block decodes one of them)
    the n + 3 special ones: one logit 40 above the rest at each index in turn (x at every support, both ends
    saturated; where that support is 0 the rest is at -inf, not 40 below: x is then exactly 0, not 1e-17, see
    x_gap_ok), all but index n // 2 at -inf, rows offset by +1e4 and by -1e4. With fewer rows than specials the first
    ones (the saturated low end first)."""
    g = _gen(32, n, rows)
    sup = torch.linspace(SMIN, SMAX, n)
    sp = []
    for i in range(n):
        r = torch.randn(n, generator=g)
        if sup[i] == 0:
            r[:] = float("-inf")
            r[i] = 0.5
        else:
            r[i] = -100.0
            r[i] = r.max() + 40.0
        sp.append(r)
    r = torch.full((n,), float("-inf"))
    r[n // 2] = -1.25
    sp.append(r)
    sp.append(3.0 * torch.randn(n, generator=g) + 1e4)
    sp.append(3.0 * torch.randn(n, generator=g) - 1e4)
    sp = torch.stack(sp)
    l = 3.0 * torch.randn(rows, n, generator=g)
    k = min(rows, len(sp))
    l[rows - k:] = sp[:k]
    return l


def x_gap_ok(x):
    """The reference's inverse transform jumps by 0.004 at x = 0; a row with 0 < |x_ref| < 1e-4 would compare the sign of
    rounding noise. A condition on the inputs (asserted on the CPU for every row the GPU tests decode), no tolerance."""
    ax = x.abs()
    return bool(((ax == 0) | (ax >= 1e-4)).all())


# ====================================================================== min-max scale
# (dtype, n, the form it is meant for): register form with one chunk, several, and the last size it takes (64 lanes x
# 20 f32 / 10 bf16 chunks); the two-pass form at the first size past that and at a size that is no multiple of a chunk
SCALE_CASES = ((0, 4, "register"), (0, 20, "register"), (0, 5120, "register"), (0, 5124, "two_pass"), (0, 6, "two_pass"),
               (1, 8, "register"), (1, 5120, "register"), (1, 5128, "two_pass"), (1, 12, "two_pass"))
SCALE_KINDS = ("random", "constant", "ends", "negative", "narrow")
SCALE_B = (1, 4, 5)


def scale_form(dtype, n):
    """mzba_scale_state's dispatch condition, restated."""
    epc, cpl = (8, 10) if dtype else (4, 20)
    return "two_pass" if n % epc != 0 or n // epc > 64 * cpl else "register"


@functools.lru_cache(maxsize=None)
def scale_input(dtype, n):
    """h [5][n] in the storage type, one row per kind: N(0, 1); the constant 0.5 (max == min, den = 1e-8, every output
    exactly 0); the strict minimum at element 0 and the strict maximum at the last element of the last chunk; all
    negative; a range of 1e-6 (the 1e-8 in den is 1 % of it)."""
    g = _gen(33, dtype, n)
    h = torch.randn(len(SCALE_KINDS), n, generator=g)
    h[1] = 0.5
    h[3] = -(torch.rand(n, generator=g) + 0.5)
    h[4] = 1e-6 * torch.rand(n, generator=g)
    h = h.to(tdt(dtype))
    h[2, 0] = (h[2].float().min() - 1.0).to(tdt(dtype))
    h[2, -1] = (h[2].float().max() + 1.0).to(tdt(dtype))
    assert (h[2, 1:] > h[2, 0]).all() and (h[2, :-1] < h[2, -1]).all() and (h[3] < 0).all()
    return h


def scale_ref(h, skip_last=0):
    """(h - min) / ((max - min) + 1e-8) per row: f64 from the stored values with the f32 value of 1e-8, and the op-by-op
    torch f32 chain (common.h: every f32 expression is evaluated op by op; the f32 kernel is compared with it bit for
    bit). Chain: two operations for the denominator, a subtract, a divide: c = 4, S = 1 (outputs lie in [0, 1]).
    skip_last leaves that many trailing elements out of the min / max (the CPU conditions)."""
    x = h.double()
    m = x[:, :x.shape[1] - skip_last]
    mn, mx = m.min(1, keepdim=True)[0], m.max(1, keepdim=True)[0]
    ref = (x - mn) / ((mx - mn) + float(np.float32(1e-8)))
    hf = h.float()
    mnf, mxf = hf.min(1, keepdim=True)[0], hf.max(1, keepdim=True)[0]
    wit = (hf - mnf) / ((mxf - mnf) + 1e-8)
    return ref, wit, 4.0


# ====================================================================== avg-pool forward
POOL_HW = ((2, 2), (16, 20), (5, 7))  # (5, 7): the odd row and column are dropped
POOL_C = (6, 8)
POOL_BIG = (129, 16, 16, 256)  # 129 * 8 * 8 * 256 outputs, more than the 8192 x 256 threads of the capped grid


def pool_ref(x):
    """x [B][H][W][C] storage type -> f64 avg_pool2d(2, 2) in NHWC, the f32 witness, S = the mean of the four |x|.
    avgpool2_kernel: three adds and a division by 4 (exact): c = 3."""
    def pool(t):
        return F.avg_pool2d(t.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).contiguous()
    return pool(x.double()), pool(x.float()), pool(x.double().abs())


# ====================================================================== generic conv edges
CONV_A, CONV_S = 3, 4
CONV_SLOTS = (2, 0, 2, 3, 1, 0, 2)  # non-monotone, repeated


def conv_shapes(dtype):
    """(B, H, W, Cin, Cout, ks) with EPC = 4 f32 / 8 bf16 elements per 16-B chunk: a ragged last K-step with one chunk
    per tap and four valid output columns; only the centre tap in bounds and a second N tile of 4 columns; a one-row
    image; 1x1 with Cin no multiple of BK; M = 140, a second M tile of 12 rows."""
    E = 8 if dtype else 4
    return ((3, 4, 5, E, 4, 3), (1, 1, 1, 3 * E, 132, 3), (2, 1, 7, 16, 8, 3), (5, 4, 5, 40, 132, 1), (7, 4, 5, 72, 128, 3))


def conv_bk(dtype):
    return 64 if dtype else 32


def conv_c(dtype, Cin, ks):
    """conv_igemm_kernel: every K-step sums BK products per output into one accumulator (zero-filled ones included),
    then the action bias, the bias and the residual: c = ceil(Ktot / BK) BK + 3."""
    bk = conv_bk(dtype)
    return math.ceil(ks * ks * Cin / bk) * bk + 3


@functools.lru_cache(maxsize=None)
def conv_case(dtype, idx):
    """pool [B][S][HW][Cin] (the gather reads slot CONV_SLOTS[b] of env b; the plain launches slot 1), w [Cout][taps
    Cin] (k = tap Cin + c), res [B HW][Cout] in the storage type; bias [Cout], tab [HW][A][Cout] f32."""
    B, H, W, Cin, Cout, ks = conv_shapes(dtype)[idx]
    g = _gen(34, dtype, idx)
    t = tdt(dtype)
    Ktot = ks * ks * Cin
    return dict(shape=(B, H, W, Cin, Cout, ks),
                pool=torch.randn(B, CONV_S, H * W, Cin, generator=g).to(t),
                w=(torch.randn(Cout, Ktot, generator=g) / Ktot ** 0.5).to(t),
                bias=0.1 * torch.randn(Cout, generator=g),
                res=torch.randn(B * H * W, Cout, generator=g).to(t),
                tab=0.3 * torch.randn(H * W, CONV_A, Cout, generator=g),
                slots=torch.tensor(CONV_SLOTS[:B], dtype=torch.int32))


def conv_input(c, gather):
    pool = c["pool"]
    if gather:
        return pool[torch.arange(pool.shape[0]), c["slots"].long()].contiguous()
    return pool[:, 1].contiguous()


def conv_ref(c, x, with_res, relu, act=None, kmask=None):
    """f64 conv of the stored operands + action bias + bias + residual (ReLU), the same in f32 in the kernel's epilogue
    order (((acc + act_bias) + bias) + res) as the witness, and S from the conv of the absolute values. kmask [taps Cin]
    zeroes weights (the CPU conditions: a dropped tap, a dropped K-step)."""
    B, H, W, Cin, Cout, ks = c["shape"]
    w = c["w"] if kmask is None else c["w"] * kmask.to(c["w"].dtype)

    def conv(xx, ww):
        xx = xx.view(B, H, W, Cin).permute(0, 3, 1, 2)
        ww = ww.view(Cout, ks, ks, Cin).permute(0, 3, 1, 2)
        return F.conv2d(xx, ww, padding=ks // 2).permute(0, 2, 3, 1).reshape(B * H * W, Cout)

    ref, S, wit = conv(x.double(), w.double()), conv(x.double().abs(), w.double().abs()), conv(x.float(), w.float())
    if act is not None:
        ab = c["tab"][:, act.long()].permute(1, 0, 2).reshape(B * H * W, Cout)  # [b][p] = tab[p][act[b]]
        ref, S, wit = ref + ab.double(), S + ab.double().abs(), wit + ab
    ref, S, wit = ref + c["bias"].double(), S + c["bias"].double().abs(), wit + c["bias"]
    if with_res:
        ref, S, wit = ref + c["res"].double(), S + c["res"].double().abs(), wit + c["res"].float()
    if relu:
        ref, wit = torch.relu(ref), torch.relu(wit)
    return ref, wit, S


def bound(ref, wit, cS, out_bf16=False):
    """ops_bounds._check's bound as a tensor (for the CPU conditions)."""
    e_w = (wit.double() - ref).abs().max().item()
    b = torch.zeros_like(ref) + 4.0 * e_w + U * cS
    return b + BF * ref.abs() if out_bf16 else b
