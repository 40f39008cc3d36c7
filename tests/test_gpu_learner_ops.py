"""The learner's small kernels (csrc/learn.hip: BatchNorm statistics / apply / backward, avg-pool backward, axpy,
min-max scale, the Linear heads, the loss, Adam, the input builders; csrc/pack.hip: the batched weight pack), each
called through the C ABI and compared with a float64 evaluation of the same operation on the CPU (plain torch /
numpy) from the same, already rounded, inputs. No mzba_* entry point serves as a reference for another.

Error bounds (the idiom of test_conv_x6_is_as_close_to_exact_as_f32). e_k is the kernel's error against f64, e_w
the error of a plain torch f32 CPU evaluation of the same operation (the witness, measured in the test) against
the same f64 reference. For an f32 output

    e_k <= 4 e_w + c 2^-24 S

with S the magnitude of the terms that enter the result and c the number of f32 operations on the longest
dependent chain of the kernel (counted from csrc/learn.hip and stated at each test; where an intermediate's error
is amplified on its way to the output — the variance under 1/sqrt, a sum inside a quotient — c S is that
propagation written out). The factor 4 allows a different summation order. A bf16 output adds one bf16 rounding of
the reference, 2^-8 |ref|; the two elements mzba_scale_backward rounds twice get two. Operations that are exact in
the storage type are compared with torch.equal. Every test prints its e_k and e_w (pytest -s).
"""
import ctypes
import functools
import itertools
import math
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ops_bounds import U, _check, _gen

pytestmark = pytest.mark.gpu

BN_EPS, BN_MOMENTUM = 1e-5, 0.1
torch.set_num_threads(min(16, os.cpu_count() or 1))


def _lib():
    from mzba import _lib as L
    return L


def _tdt(dtype):
    return torch.bfloat16 if dtype else torch.float32


def _f32(v):
    return float(np.float32(v))


def _bytes(n):
    return torch.empty(max(int(n), 1), dtype=torch.uint8, device="cuda")


# ====================================================================== BatchNorm
# (M, C): variance 0 with the unbiased divisor guarded; fewer rows than the 16 row lanes and C no multiple of 64; a
# 1-row last chunk; 513 chunks of 64 rows, the first count that enters the finalisers' loop after the 8 x 64 preload
BN_SHAPES = [(1, 4), (15, 36), (65, 64), (64 * 512 + 1, 8)]
BN_STATS_CASES = [(M, C, 0) for M, C in BN_SHAPES] + [(64 * 512 + 1, 8, 1)]


@functools.lru_cache(maxsize=None)
def _bn_data(M, C, dtype, offset):
    g = _gen(11, M, C, dtype, offset)
    x = torch.randn(M, C, generator=g)
    if offset:  # mean 3, std 0.05: the between-chunk term d^2 n nb / tot of the chunk combine carries the variance
        x = 3.0 + 0.05 * x
    if M > 64:  # the last row (alone in the last chunk) four standard deviations out: dropping it moves every statistic
        sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
        x[-1] = x[:-1].mean(0) + 4.0 * x[:-1].std(0) * sign
    x = x.to(_tdt(dtype))
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.5 * torch.randn(C, generator=g)
    run_mean = 0.2 * torch.randn(C, generator=g)
    run_var = 1.0 + 0.5 * torch.rand(C, generator=g)
    return x, gamma, beta, run_mean, run_var


def _bn_ref(x, gamma, beta):
    """f64 batch statistics of x [M][C]: mean, biased variance, invstd, gamma invstd, beta - mean gamma invstd."""
    x64 = x.double()
    mean, var = x64.mean(0), x64.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + _f32(BN_EPS))
    alpha = gamma.double() * invstd
    return mean, var, invstd, alpha, beta.double() - mean * alpha


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("M,C,offset", BN_STATS_CASES)
def test_bn_stats(dtype, M, C, offset):
    """mzba_bn_stats: the four stats rows and the running statistics (momentum 0.1, unbiased variance, divisor guarded
    at M = 1) against f64 mean / var(unbiased=False) / var(unbiased=True); also with run_mean = run_var = NULL.

    Chains (bn_stats_partial_kernel, then the combine in double): a chunk mean is 4 row adds, 15 tree adds, a divide
    and the final cast: c S = 21 max|x|. The chunk M2 is a subtract, a square and the same 19 adds, 22 max (x - mean)^2,
    and inherits the chunk means' error through the between-chunk term, 2 sqrt(max (x - mean)^2) (c S)_mean. invstd
    amplifies the variance's error by invstd^3 / 2 and rounds twice; alpha = gamma invstd adds a multiply; beta' = beta -
    mean alpha a multiply and a subtract; the running statistics one rounding each."""
    L = _lib()
    x, gamma, beta, rm0, rv0 = _bn_data(M, C, dtype, offset)
    mom = _f32(BN_MOMENTUM)
    x64 = x.double()
    mean, var, invstd, alpha, betap = _bn_ref(x, gamma, beta)
    unb = x64.var(0, unbiased=True) if M > 1 else torch.zeros(C, dtype=torch.float64)
    rm1 = mom * mean + (1.0 - mom) * rm0.double()
    rv1 = mom * unb + (1.0 - mom) * rv0.double()
    # the f32 witness
    xf = x.float()
    mean_w, var_w = xf.mean(0), xf.var(0, unbiased=False)
    unb_w = xf.var(0, unbiased=True) if M > 1 else torch.zeros(C)
    invstd_w = 1.0 / torch.sqrt(var_w + BN_EPS)
    alpha_w = gamma * invstd_w
    betap_w = beta - mean_w * alpha_w
    rm_w = BN_MOMENTUM * mean_w + (1 - BN_MOMENTUM) * rm0
    rv_w = BN_MOMENTUM * unb_w + (1 - BN_MOMENTUM) * rv0
    # c S per output
    Sx = x64.abs().max(0)[0]
    Sv = ((x64 - mean) ** 2).max(0)[0]
    cs_mean = 21 * Sx
    cs_var = 22 * Sv + 2 * Sv.sqrt() * cs_mean
    cs_invstd = 0.5 * invstd ** 3 * cs_var + 2 * invstd
    cs_alpha = gamma.double().abs() * cs_invstd + alpha.abs()
    cs_betap = alpha.abs() * cs_mean + mean.abs() * cs_alpha + 2 * (beta.double().abs() + (mean * alpha).abs())
    cs_rm = mom * cs_mean + rm1.abs()
    cs_rv = mom * cs_var * (M / (M - 1.0) if M > 1 else 1.0) + rv1.abs()
    xd, gd, bd = x.cuda(), gamma.cuda(), beta.cuda()
    ws = _bytes((M + 63) // 64 * C * 8)
    tag = f"bn_stats dtype {dtype} M {M} C {C} offset {offset}"
    for with_run in (True, False):
        stats = torch.full((4, C), float("nan"), device="cuda")
        rm, rv = (rm0.cuda(), rv0.cuda()) if with_run else (None, None)
        L.call("mzba_bn_stats", dtype, L.ptr(xd), M, C, BN_EPS, BN_MOMENTUM, L.ptr(gd), L.ptr(bd), L.ptr(stats), L.ptr(rm),
               L.ptr(rv), L.ptr(ws), ws.numel(), L.stream())
        torch.cuda.synchronize()
        t = f"{tag} run {int(with_run)}"
        _check(t + " mean", stats[0], mean, mean_w, cs_mean)
        _check(t + " invstd", stats[1], invstd, invstd_w, cs_invstd)
        _check(t + " alpha", stats[2], alpha, alpha_w, cs_alpha)
        _check(t + " beta'", stats[3], betap, betap_w, cs_betap)
        if with_run:
            _check(t + " running_mean", rm, rm1, rm_w, cs_rm)
            _check(t + " running_var", rv, rv1, rv_w, cs_rv)


def _bn_apply_case(dtype, M, C, with_res, relu, alias):
    L = _lib()
    g = _gen(12, M, C, dtype)
    x = torch.randn(M, C, generator=g).to(_tdt(dtype))
    res = torch.randn(M, C, generator=g).to(_tdt(dtype)) if with_res else None
    stats = torch.randn(4, C, generator=g)
    stats[2] = 1.0 + 0.3 * stats[2]
    xd, rd, sd = x.cuda(), (res.cuda() if with_res else None), stats.cuda()
    out = xd if alias == "x" else rd if alias == "res" else torch.full((M, C), float("nan"), device="cuda").to(_tdt(dtype))
    L.call("mzba_bn_apply", dtype, L.ptr(xd), L.ptr(sd), L.ptr(rd), relu, L.ptr(out), M, C, L.stream())
    torch.cuda.synchronize()
    a, b = stats[2].double(), stats[3].double()
    ref = x.double() * a + b
    S = (x.double() * a).abs() + b.abs()
    wit = x.float() * stats[2] + stats[3]
    if with_res:
        ref, S, wit = ref + res.double(), S + res.double().abs(), wit + res.float()
    if relu:
        ref, wit = torch.relu(ref), torch.relu(wit)
    _check(f"bn_apply dtype {dtype} {M}x{C} res {int(with_res)} relu {relu} alias {alias}", out, ref, wit, 3 * S,
           out_bf16=bool(dtype))


@pytest.mark.parametrize("dtype", [0, 1])
def test_bn_apply(dtype):
    """mzba_bn_apply at (65, 36): with and without the residual, with and without ReLU, out aliasing x and res.
    Chain: a multiply, an add, the residual add: c = 3 on |x alpha| + |beta'| + |res|."""
    for with_res, relu in itertools.product((False, True), (0, 1)):
        for alias in (None, "x") + (("res",) if with_res else ()):
            _bn_apply_case(dtype, 65, 36, with_res, relu, alias)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("with_res,relu,alias", [(True, 1, "res"), (False, 0, "x")])
def test_bn_apply_second_grid_pass(dtype, with_res, relu, alias):
    """(65537, 260): 65537 * 65 float4s, more than the 16384 * 256 threads of the capped grid, so the grid-stride loop
    runs a second pass (C / 4 = 65 is odd, so a pass starts at another channel than the one before)."""
    assert 65537 * 260 // 4 > 16384 * 256
    _bn_apply_case(dtype, 65537, 260, with_res, relu, alias)


@functools.lru_cache(maxsize=None)
def _bn_bwd_data(M, C, dtype):
    """Inputs of the backward and its f64 autograd reference, with and without the ReLU mask."""
    x, gamma, beta = _bn_data(M, C, dtype, 0)[:3]
    g = _gen(13, M, C, dtype)
    mean, var, invstd, alpha, betap = _bn_ref(x, gamma, beta)
    stats = torch.stack([mean, invstd, alpha, betap]).float()
    dy = (torch.randn(M, C, generator=g) + 0.5).to(_tdt(dtype))  # a mean well off zero: the mean(g) term matters
    y64 = torch.relu(x.double() * alpha + betap)
    y = y64.to(_tdt(dtype))
    assert ((y > 0) == (y64 > 0)).all() and (y == 0).any()
    zi = int((y.flatten() == 0).nonzero()[0])
    y.view(-1)[zi] = -0.0  # one negative zero among the exact zeros: masked like them
    assert math.copysign(1.0, y.view(-1)[zi].item()) == -1.0
    dg0, db0 = torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps = _f32(BN_EPS)
    refs = {}
    for with_y in (True, False):
        xg = x.double().requires_grad_()
        gm, bt = gamma.double().requires_grad_(), beta.double().requires_grad_()
        if M > 1:
            z = F.batch_norm(xg, None, None, gm, bt, training=True, momentum=0.0, eps=eps)
        else:  # F.batch_norm refuses one value per channel in training mode: the same function, written out
            z = (xg - xg.mean(0)) / torch.sqrt(xg.var(0, unbiased=False) + eps) * gm + bt
        o = torch.relu(z) if with_y else z
        if with_y:
            assert ((o > 0) == (y > 0)).all()
        o.backward(dy.double())
        refs[with_y] = (xg.grad, dg0.double() + gm.grad, db0.double() + bt.grad)
    return x, stats, dy, y, dg0, db0, refs


def _bn_bwd_bounds(x, stats, g, dg0, db0, M):
    """Witness and c S of dgamma, dbeta, dx from the masked gradient g (storage type).
    bn_bwd_partial_kernel: a chunk's sum g is 4 row adds and 15 tree adds, sum g (x - mean) a subtract and a multiply
    more (21); the finaliser adds in double, casts, and forms dgamma (multiply, add: 24 on |dgamma0| + sum |g| (|x| +
    |mean|) invstd), dbeta (21 on |dbeta0| + sum |g|), k = dot invstd^2 / M (3 more) and mean(g). bn_bwd_apply_kernel:
    5 operations on top of k's 24 and mean(g)'s 21: c = 30 on |alpha| (|g| + (|x| + |mean|) K + MG), K and MG the
    sums of absolute values behind k and mean(g). |x| + |mean| in place of |x - mean| carries the f32 rounding of
    the mean in stats; the roundings of invstd and alpha are relative and inside c."""
    mean, invstd, alpha = stats[0], stats[1], stats[2]
    gf, xm = g.float(), x.float() - mean
    sg, dot = gf.sum(0), (gf * xm).sum(0)
    wit = (((gf - xm * (dot * invstd * invstd / M)) - sg / M) * alpha, dg0 + dot * invstd, db0 + sg)
    g64, ax = g.double().abs(), x.double().abs() + mean.double().abs()
    a_dot, a_sg = (g64 * ax).sum(0), g64.sum(0)
    i64, al64 = invstd.double(), alpha.double().abs()
    cs = (30 * al64 * (g64 + ax * (a_dot * i64 ** 2 / M) + a_sg / M), 24 * (dg0.double().abs() + a_dot * i64),
          21 * (db0.double().abs() + a_sg))
    return wit, cs


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("M,C", BN_SHAPES)
def test_bn_backward(dtype, M, C):
    """mzba_bn_backward against f64 autograd of relu(batch_norm(x)) (y given) and of batch_norm(x) (y = NULL) for the
    upstream gradient dy: the in-place ReLU mask of dy exactly (y holds exact zeros and one -0.0), dgamma and dbeta
    added to non-zero starting values, dx. Then the split path: mzba_bn_backward_coef + mzba_bn_backward_apply, and
    mzba_bn_backward_final, fed per-chunk partials the test computes in f64, against the same reference."""
    L = _lib()
    x, stats, dy, y, dg0, db0, refs = _bn_bwd_data(M, C, dtype)
    xd, sd = x.cuda(), stats.cuda()
    nchunk = (M + 63) // 64
    ws = _bytes(nchunk * C * 8 + 12 * C)
    bf = bool(dtype)
    for with_y in (True, False):
        tag = f"bn_backward dtype {dtype} M {M} C {C} y {int(with_y)}"
        g = torch.where(y > 0, dy, torch.zeros_like(dy)) if with_y else dy
        (wdx, wdg, wdb), (cdx, cdg, cdb) = _bn_bwd_bounds(x, stats, g, dg0, db0, M)
        rdx, rdg, rdb = refs[with_y]
        dyd, yd = dy.cuda(), (y.cuda() if with_y else None)
        dg, db = dg0.cuda(), db0.cuda()
        dx = torch.full((M, C), float("nan"), device="cuda").to(_tdt(dtype))
        L.call("mzba_bn_backward", dtype, L.ptr(dyd), L.ptr(yd), L.ptr(xd), L.ptr(sd), M, C, L.ptr(dg), L.ptr(db),
               L.ptr(dx), L.ptr(ws), ws.numel(), L.stream())
        torch.cuda.synchronize()
        assert torch.equal(dyd.cpu(), g), tag + ": ReLU mask of dy"
        _check(tag + " dx", dx, rdx, wdx, cdx, out_bf16=bf)
        _check(tag + " dgamma", dg, rdg, wdg, cdg)
        _check(tag + " dbeta", db, rdb, wdb, cdb)
        # the split path from f64 partials (sum g, sum g (x - mean)) per chunk of 64 rows, rounded to f32
        g64 = torch.zeros(nchunk * 64, C, dtype=torch.float64)
        g64[:M] = g.double()
        gx64 = torch.zeros(nchunk * 64, C, dtype=torch.float64)
        gx64[:M] = g.double() * (x.double() - stats[0].double())
        part = torch.stack([g64.view(nchunk, 64, C).sum(1), gx64.view(nchunk, 64, C).sum(1)], -1).float().contiguous()
        pd, gd = part.cuda(), g.cuda()
        dg, db = dg0.cuda(), db0.cuda()
        coef = torch.full((3, C), float("nan"), device="cuda")
        dx = torch.full((M, C), float("nan"), device="cuda").to(_tdt(dtype))
        L.call("mzba_bn_backward_coef", L.ptr(pd), nchunk, M, C, L.ptr(sd), L.ptr(dg), L.ptr(db), L.ptr(coef), L.stream())
        L.call("mzba_bn_backward_apply", dtype, L.ptr(gd), L.ptr(xd), L.ptr(sd), L.ptr(coef), L.ptr(dx), M, C, L.stream())
        dg2, db2 = dg0.cuda(), db0.cuda()
        dx2 = torch.full((M, C), float("nan"), device="cuda").to(_tdt(dtype))
        ws2 = _bytes(12 * C)
        L.call("mzba_bn_backward_final", dtype, L.ptr(gd), L.ptr(xd), L.ptr(sd), L.ptr(pd), nchunk, M, C, L.ptr(dg2),
               L.ptr(db2), L.ptr(dx2), L.ptr(ws2), ws2.numel(), L.stream())
        torch.cuda.synchronize()
        for name, a, b, c in ((" coef+apply", dx, dg, db), (" final", dx2, dg2, db2)):
            _check(tag + name + " dx", a, rdx, wdx, cdx, out_bf16=bf)
            _check(tag + name + " dgamma", b, rdg, wdg, cdg)
            _check(tag + name + " dbeta", c, rdb, wdb, cdb)


# ====================================================================== avg-pool backward, axpy
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("C", [8, 6])
@pytest.mark.parametrize("H,W", [(16, 20), (2, 2)])
def test_avgpool2_backward(dtype, C, H, W):
    """mzba_avgpool2_backward (C = 8: the float4 kernel, C = 6: the scalar one) equals f64 autograd of avg_pool2d(2, 2)
    exactly: a division by 4 is exact in f32 and bf16."""
    L = _lib()
    B = 3
    dy = torch.randn(B, H // 2, W // 2, C, generator=_gen(14, C, H, dtype)).to(_tdt(dtype))
    xg = torch.zeros(B, C, H, W, dtype=torch.float64, requires_grad=True)
    F.avg_pool2d(xg, 2, 2).backward(dy.double().permute(0, 3, 1, 2))
    ref = xg.grad.permute(0, 2, 3, 1).contiguous()
    dyd = dy.cuda()
    dx = torch.full((B, H, W, C), float("nan"), device="cuda").to(_tdt(dtype))
    L.call("mzba_avgpool2_backward", dtype, L.ptr(dyd), L.ptr(dx), B, H, W, C, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(dx.cpu().double(), ref)


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("n", [1, 255, 16384 * 256 + 3])
def test_axpy(dtype, n):
    """mzba_axpy: y += x equals (y.float() + x.float()).to(dtype) exactly (the f32 sum of two storage values, rounded
    once to the storage type); n = 16384 * 256 + 3 is past the capped grid and takes a second grid-stride pass."""
    L = _lib()
    g = _gen(15, n, dtype)
    y, x = torch.randn(n, generator=g).to(_tdt(dtype)), torch.randn(n, generator=g).to(_tdt(dtype))
    yd, xd = y.cuda(), x.cuda()
    L.call("mzba_axpy", dtype, L.ptr(yd), L.ptr(xd), n, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(yd.cpu(), (y.float() + x.float()).to(_tdt(dtype)))
    assert torch.equal(xd.cpu(), x)


# ====================================================================== min-max scale
SCALE_B, SCALE_HW = 5, 20


@functools.lru_cache(maxsize=None)
def _scale_images(C):
    """B = 5 NHWC images [HW][C] of post-ReLU values on the bf16 grid (exact in both storage types): the minimum 0
    ties many times; images 1 and 2 hold their maximum twice, first in NHWC order at (pixel 0, channel C-1), first in
    NCHW order at (pixel HW-1, channel 0); image 4 is constant. Returns h and, from numpy, min / max and the NHWC
    index of the first min / max in NCHW flatten order."""
    HW = SCALE_HW
    h = torch.relu(torch.randn(SCALE_B, HW, C, generator=_gen(16, C))).bfloat16().float()
    for b in (1, 2):
        v = (h[b].max() + 1.0).bfloat16().float()
        h[b, 0, C - 1] = v
        h[b, HW - 1, 0] = v
    h[4] = 0.5
    a = h.numpy()
    mm = np.stack([a.reshape(SCALE_B, -1).min(1), a.reshape(SCALE_B, -1).max(1)], 1)
    nchw = a.transpose(0, 2, 1).reshape(SCALE_B, -1)  # (C, HW)-ordered view
    keys = np.stack([nchw.argmin(1), nchw.argmax(1)], 1)  # numpy: the first occurrence
    idx = ((keys % HW) * C + keys // HW).astype(np.int32)
    first_nhwc = np.stack([a.reshape(SCALE_B, -1).argmin(1), a.reshape(SCALE_B, -1).argmax(1)], 1)
    # without an image where the two orders disagree about the first tie the test could not tell the rules apart
    assert (first_nhwc[:, 0] != idx[:, 0]).any() and (first_nhwc[1:3, 1] != idx[1:3, 1]).all()
    assert (idx[4] == 0).all()
    return h, mm, keys, idx


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("C", [4, 32, 256])
def test_scale_forward(dtype, C):
    """mzba_scale_forward: minmax is the true min and max; each recorded NHWC index holds that value and is the first
    such position in NCHW flatten order (numpy argmin / argmax of the (C, HW)-ordered view), with tied minima in every
    image, a doubled maximum in two and a constant image (den = 1e-8, argmin == argmax); outputs against f64
    (h - min) / (max - min + 1e-8). Chain: two operations for the denominator, a subtract, a divide: c = 4, S = 1."""
    L = _lib()
    h, mm, keys, idx = _scale_images(C)
    B, HW = SCALE_B, SCALE_HW
    hd = h.to(_tdt(dtype)).cuda()
    out = torch.full((B, HW, C), float("nan"), device="cuda").to(_tdt(dtype))
    mmd = torch.full((B, 2), float("nan"), device="cuda")
    ixd = torch.full((B, 2), -1, dtype=torch.int32, device="cuda")
    L.call("mzba_scale_forward", dtype, L.ptr(hd), L.ptr(out), L.ptr(mmd), L.ptr(ixd), B, HW, C, L.stream())
    torch.cuda.synchronize()
    assert torch.equal(mmd.cpu(), torch.from_numpy(mm))
    got = ixd.cpu().numpy()
    flat = h.numpy().reshape(B, -1)
    assert (got >= 0).all() and (got < HW * C).all()
    assert np.array_equal(np.take_along_axis(flat, got.astype(np.int64), 1), mm)
    assert np.array_equal(got, idx), (got, idx)
    mn, mx = torch.from_numpy(mm[:, 0]).view(B, 1, 1), torch.from_numpy(mm[:, 1]).view(B, 1, 1)
    ref = (h.double() - mn.double()) / (mx.double() - mn.double() + 1e-8)
    wit = (h - mn) / (mx - mn + 1e-8)
    _check(f"scale_forward dtype {dtype} C {C}", out, ref, wit, 4.0, out_bf16=bool(dtype))


def _scale_autograd(h, dy, keys, tdt):
    hg = h.detach().to(tdt).clone().requires_grad_()
    f = hg.permute(0, 2, 1).reshape(h.shape[0], -1)  # NCHW flatten order
    mn, imn = f.min(1)
    mx, imx = f.max(1)
    # torch's CPU min / max(dim) return (and route their gradient to) the first index, as numpy does
    assert np.array_equal(imn.numpy(), keys[:, 0]) and np.array_equal(imx.numpy(), keys[:, 1])
    ((hg - mn.view(-1, 1, 1)) / (mx - mn + 1e-8).view(-1, 1, 1)).backward(dy.to(tdt))
    return hg.grad


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("C", [4, 32, 256])
@pytest.mark.parametrize("accumulate", [0, 1])
def test_scale_backward(dtype, C, accumulate):
    """mzba_scale_backward on test_scale_forward's images with min / max and their indices from numpy (not from the
    kernel), against f64 autograd through h.min(1) / h.max(1) of the NCHW-flattened image, dh overwritten and added to.
    Chain: dy / den and the add: c = 2 on |dh0| + |dy| / den; the two routed elements add the block sums: up to 20
    adds per thread, 6 + 3 for the fold, 6 for the quotients: c = 35 on A1 + 2 A2, A1 = sum |dy| / den, A2 =
    sum |dy (h - min)| / den^2. In bf16 the routed elements are stored, read back and stored again: two roundings;
    the inputs make the first store's value no larger than the final one (asserted), so both are within 2^-8 |ref|."""
    L = _lib()
    h, mm, keys, idx = _scale_images(C)
    B, HW, n = SCALE_B, SCALE_HW, SCALE_HW * C
    g = _gen(17, C, dtype, accumulate)
    dy = (torch.randn(B, HW, C, generator=g) + 1.0).to(_tdt(dtype))
    dh0 = (0.1 * torch.randn(B, HW, C, generator=g)).to(_tdt(dtype))
    ref = _scale_autograd(h, dy.double(), keys, torch.float64)
    wit = _scale_autograd(h, dy.float(), keys, torch.float32)
    old = dh0.double() if accumulate else torch.zeros(B, HW, C, dtype=torch.float64)
    ref, wit = ref + old, wit + old.float()
    den = (torch.from_numpy(mm[:, 1]).double() - torch.from_numpy(mm[:, 0]).double() + 1e-8).view(B, 1, 1)
    mn = torch.from_numpy(mm[:, 0]).double().view(B, 1, 1)
    first = old + dy.double() / den  # the value of the first store
    cs = 2 * (old.abs() + dy.double().abs() / den)
    a1 = (dy.double().abs() / den).sum((1, 2))
    a2 = (dy.double().abs() * (h.double() - mn) / den ** 2).sum((1, 2))
    ulps = torch.ones(B, n, dtype=torch.float64)
    cs = cs.reshape(B, n).clone()
    ix = torch.from_numpy(idx.astype(np.int64))
    for b in range(B):
        for k in ix[b].tolist():
            cs[b, k] += 35 * (a1[b] + 2 * a2[b])
            ulps[b, k] = 2.0
            assert not dtype or ref.reshape(B, n)[b, k].abs() >= first.reshape(B, n)[b, k].abs(), (b, k)
    hd, dyd = h.to(_tdt(dtype)).cuda(), dy.cuda()
    dh = dh0.cuda() if accumulate else torch.full((B, HW, C), float("nan"), device="cuda").to(_tdt(dtype))
    mmd, ixd = torch.from_numpy(mm).cuda(), torch.from_numpy(idx).cuda()
    L.call("mzba_scale_backward", dtype, L.ptr(dyd), L.ptr(hd), L.ptr(mmd), L.ptr(ixd), L.ptr(dh), B, n, accumulate,
           L.stream())
    torch.cuda.synchronize()
    # the constant image (den = 1e-8, values of order 1e8 n) on its own, so its witness error does not widen the others' bound
    got, ref, wit = dh.reshape(B, n).cpu(), ref.reshape(B, n), wit.reshape(B, n)
    for name, r in (("images 0-3", slice(0, 4)), ("constant image", slice(4, 5))):
        _check(f"scale_backward dtype {dtype} C {C} accumulate {accumulate} {name}", got[r], ref[r], wit[r], cs[r],
               out_bf16=bool(dtype), ulps=ulps[r])


# ====================================================================== Linear heads
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_linear_forward_backward(dtype, B):
    """mzba_linear_forward / mzba_linear_backward against f64 matmuls for O in {1, 3, 11, 16} and K in {100, 1280}
    (no multiple of 256); B = 64 starts the 16-way split of the weight gradient, at B = 65 (5 rows per split) the last
    three splits are empty. dx written, added to and skipped (NULL); dw and db added to non-zero starting values.
    Chains: forward 2 ceil(K / 256) multiply-adds per thread, 6 + 2 for the fold, the bias: c = 2 ceil(K / 256) + 9
    on |bias| + sum |w x|. dx: c = 2 O + 1 on |dx0| + sum |dy w|. dw: 2 rows-per-split operations, then nsplit adds and
    the accumulate: c = 2 rps + nsplit + 1 on |dw0| + sum |dy x|; db the same with one operation per row."""
    L = _lib()
    for O, K in itertools.product((1, 3, 11, 16), (100, 320 * 4)):
        g = _gen(18, dtype, B, O, K)
        x = torch.randn(B, K, generator=g).to(_tdt(dtype))
        w = torch.randn(O, K, generator=g) / K ** 0.5
        bias = torch.randn(O, generator=g)
        dy = torch.randn(B, O, generator=g)
        dw0, db0 = torch.randn(O, K, generator=g), torch.randn(O, generator=g)
        dx0 = torch.randn(B, K, generator=g).to(_tdt(dtype))
        x64, w64, dy64 = x.double(), w.double(), dy.double()
        tag = f"linear dtype {dtype} B {B} O {O} K {K}"
        xd, wd, bd, dyd = x.cuda(), w.cuda(), bias.cuda(), dy.cuda()
        out = torch.full((B, O), float("nan"), device="cuda")
        L.call("mzba_linear_forward", dtype, L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(out), B, K, O, L.stream())
        torch.cuda.synchronize()
        _check(tag + " forward", out, x64 @ w64.t() + bias.double(), x.float() @ w.t() + bias,
               (2 * math.ceil(K / 256) + 9) * (bias.double().abs() + x64.abs() @ w64.abs().t()))
        nsplit = 16 if B >= 64 else 1
        rps = (B + nsplit - 1) // nsplit
        ws = _bytes(L.lib().mzba_linear_ws_bytes(B, K, O))
        assert ws.numel() >= nsplit * (O * K + O) * 4
        rdw, rdb = dw0.double() + dy64.t() @ x64, db0.double() + dy64.sum(0)
        wdw, wdb = dw0 + dy.t() @ x.float(), db0 + dy.sum(0)
        cdw = (2 * rps + nsplit + 1) * (dw0.double().abs() + dy64.abs().t() @ x64.abs())
        cdb = (rps + nsplit + 1) * (db0.double().abs() + dy64.abs().sum(0))
        for mode in ("write", "accumulate", "null"):
            dw, db = dw0.cuda(), db0.cuda()
            dx = None if mode == "null" else dx0.cuda() if mode == "accumulate" else \
                torch.full((B, K), float("nan"), device="cuda").to(_tdt(dtype))
            L.call("mzba_linear_backward", dtype, L.ptr(xd), L.ptr(wd), L.ptr(dyd), L.ptr(dx), int(mode == "accumulate"),
                   L.ptr(dw), L.ptr(db), B, K, O, L.ptr(ws), ws.numel(), L.stream())
            torch.cuda.synchronize()
            _check(f"{tag} {mode} dw", dw, rdw, wdw, cdw)
            _check(f"{tag} {mode} db", db, rdb, wdb, cdb)
            if dx is not None:
                old = dx0.double() if mode == "accumulate" else torch.zeros(B, K, dtype=torch.float64)
                _check(f"{tag} {mode} dx", dx, old + dy64 @ w64, old.float() + dy @ w,
                       (2 * O + 1) * (old.abs() + dy64.abs() @ w64.abs()), out_bf16=bool(dtype))


# ====================================================================== loss
SMIN, SMAX = -5.0, 5.0


def _compact64(x):
    """utils.py:30-64's transform sign(x) (sqrt(|x| + 1) - 1 + 0.001 x) in f64 (for the test's inputs and bounds; the
    reference values come from oracle.learner.supports_representation)."""
    return np.sign(x) * (np.sqrt(np.abs(x) + 1.0) - 1.0 + 0.001 * x)


def _largest_below_smax():
    """The largest f32 whose f64 transform is still below SMAX (bisection on the f64 transform, then the f32 grid)."""
    lo, hi = 0.0, 100.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _compact64(mid) < SMAX else (lo, mid)
    x = np.float32(lo)
    while _compact64(float(x)) >= SMAX:
        x = np.nextafter(x, np.float32(0))
    assert _compact64(float(np.nextafter(x, np.float32(np.inf)))) >= SMAX > _compact64(float(x))
    return float(x)


def _loss_reference(lr, lv, lp, rw, tg, ct, K, ns, na, tdt):
    """loss_fn through oracle.learner's supports_representation and kl_batchmean in dtype tdt; the logit gradients by
    autograd of the total. lr / lv / lp are [K][B][n]; rw / tg [B][K]; ct [B][K][na] (rows already gathered)."""
    from oracle.learner import kl_batchmean, supports_representation
    z = [t.detach().to(tdt).clone().requires_grad_() for t in (lr, lv, lp)]
    tr = supports_representation(rw.to(tdt), SMIN, SMAX, ns)
    tv = supports_representation(tg.to(tdt), SMIN, SMAX, ns)
    c = ct.to(tdt)
    tp = c / c.sum(-1, keepdim=True)
    parts = [kl_batchmean(zz.permute(1, 0, 2), tt) for zz, tt in zip(z, (tr, tv, tp))]
    total = (1 / K) * (parts[0] + parts[1] + parts[2])
    total.backward()
    return torch.stack([total] + parts).detach(), [zz.grad for zz in z], (tr, tv, tp)


def _loss_bounds(z, t, comp, K, step):
    """c S of one head's mean KL and of its logit gradients, from f64 logits z [K][B][n] and targets t [B][K][n].
    kl_row: max, n exp-adds, log, and per entry two subtracts, log t, a subtract and a multiply: c = n + 10 on
    sum t (|ln t| + |logp|) + max |logp|. A two-hot target carries the f32 transform's and supports' rounding, dt = 12
    2^-24 (|compact| + 1) / step, which moves t ln t by up to dt (1 + |ln dt| + max |logp|) per entry. Gradient entry:
    (n + 10) 2^-24 (1 + |z - max| + |log sum|) softmax + dt + 2 2^-24 (softmax + t), times 1 / (K B K)."""
    n = z.shape[-1]
    zz = z.permute(1, 0, 2)
    lp = torch.log_softmax(zz, -1)
    soft = lp.exp()
    tl = torch.where(t > 0, t * t.clamp_min(1e-300).log().abs(), torch.zeros_like(t))
    lpmax = lp.abs().max(-1)[0]
    c = n + 10 + (0 if comp is not None else n + 1)
    row = c * ((tl + t * lp.abs()).sum(-1) + lpmax)
    if comp is not None:
        dt = 12 * U * (comp.abs() + 1) / step
        row = row + 2 * dt * (1 + dt.log().abs() + lpmax) / U
        dte = (dt / U).unsqueeze(-1).expand_as(t)
    else:
        dte = (n + 1) * t
    zmax = zz.max(-1, keepdim=True)[0]
    ls = (zz - zmax).exp().sum(-1, keepdim=True).log().abs()
    gr = (c * (1 + (zz - zmax).abs() + ls) * soft + dte + 2 * (soft + t)) / (K * zz.shape[0] * K)
    return row.mean(), gr.permute(1, 0, 2)


@pytest.mark.parametrize("B,K", [(1, 1), (37, 3), (300, 5)])
@pytest.mark.parametrize("ns,na", [(11, 3), (16, 16)])
@pytest.mark.parametrize("with_slots", [True, False])
def test_learner_loss(B, K, ns, na, with_slots):
    """mzba_learner_loss and mzba_learner_loss_ws, each against oracle.learner's supports_representation + kl_batchmean
    in f64 with the logit gradients from autograd of the total ((300, 5): more rows than 4 x 256, the reduction's
    4-way unrolled fold). Rewards and value targets hold 0 (exactly on a support at ns = 11), +-1e-6, values of both
    signs, the largest f32 whose transform is still below smax and its negative; count rows hold [S, 0, 0, ...] and
    other zeros (0 log 0 = 0).

    What these inputs cannot show: kl_row's sum(t) factor (normalised counts and a two-hot both sum to 1 up to an f32
    rounding) and `<=` against `<` in two_hot's bracket search (a transform exactly on support i gives the same two-hot
    from [i-1, i] with weights 0 / 1 as from [i, i+1] with 1 / 0).

    Precondition: every target's transform lies in [smin, smax]. Outside it the reference's own two-hot has a negative
    entry and the loss is not defined; such targets are not tested (asserted on the reference's two-hot)."""
    L = _lib()
    g = _gen(19, B, K, ns, na, with_slots)
    cap = B + 4 if with_slots else B
    slots = torch.randperm(cap, generator=g)[:B].to(torch.int32) if with_slots else None
    sel = slots.long() if with_slots else torch.arange(B)
    lr, lv = torch.randn(K, B, ns, generator=g) * 3, torch.randn(K, B, ns, generator=g) * 3
    lp = torch.randn(K, B, na, generator=g)
    edge = _largest_below_smax()
    special = torch.tensor([0.0, 1e-6, -1e-6, 2.5, -7.0, edge, -edge])
    rewards = torch.randint(-1, 2, (cap, K), generator=g).float()
    targets = torch.randn(cap, K, generator=g) * 4
    nsp = min(B * K, len(special))
    rsel, tsel = rewards[sel].clone(), targets[sel].clone()
    rsel.view(-1)[:nsp] = special[:nsp]
    tsel.view(-1)[:nsp] = special.flip(0)[:nsp]
    rewards[sel], targets[sel] = rsel, tsel
    counts = torch.randint(0, 51, (cap, K, na), generator=g).float()
    counts[..., 0] += 1
    counts[sel[0], 0] = 0
    counts[sel[0], 0, 0] = 50
    rw, tg, ct = rewards[sel], targets[sel], counts[sel]
    ref, rgrad, tt = _loss_reference(lr, lv, lp, rw, tg, ct, K, ns, na, torch.float64)
    wit, wgrad, _ = _loss_reference(lr, lv, lp, rw, tg, ct, K, ns, na, torch.float32)
    for t in tt:  # the precondition: a valid distribution per row
        assert (t >= 0).all() and (t <= 1).all() and torch.allclose(t.sum(-1), torch.ones(B, K, dtype=torch.float64))
    step = (SMAX - SMIN) / (ns - 1)
    comps = (torch.from_numpy(_compact64(rw.double().numpy())), torch.from_numpy(_compact64(tg.double().numpy())), None)
    rows, gbs = zip(*[_loss_bounds(z.double(), t, c, K, step) for z, t, c in zip((lr, lv, lp), tt, comps)])
    cs_parts = [r + 2 * p.abs() for r, p in zip(rows, ref[1:])]
    cs_loss = torch.stack([(1 / K) * sum(cs_parts) + 3 * ref[0].abs()] + cs_parts)
    dev = [t.cuda() for t in (lr, lv, lp, rewards, targets, counts)]
    sd = slots.cuda() if with_slots else None
    for use_ws in (False, True):
        d = [torch.full_like(t, float("nan")) for t in dev[:3]]
        loss = torch.full((4,), float("nan"), device="cuda")
        args = [L.ptr(t) for t in dev] + [L.ptr(sd), B, K, ns, na, SMIN, SMAX] + [L.ptr(t) for t in d] + [L.ptr(loss)]
        if use_ws:
            ws = _bytes(L.lib().mzba_learner_loss_ws_bytes(B, K))
            L.call("mzba_learner_loss_ws", *args, L.ptr(ws), ws.numel(), L.stream())
        else:
            L.call("mzba_learner_loss", *args, L.stream())
        torch.cuda.synchronize()
        tag = f"learner_loss{'_ws' if use_ws else ''} B {B} K {K} ns {ns} na {na} slots {int(with_slots)}"
        _check(tag + " loss", loss, ref, wit, cs_loss)
        for name, a, r, w_, c in zip(("dlogit_r", "dlogit_v", "dlogit_p"), d, rgrad, wgrad, gbs):
            _check(f"{tag} {name}", a, r, w_, c)


# ====================================================================== Adam
@functools.lru_cache(maxsize=None)
def _adam_data(n):
    g = _gen(20, n)
    return (torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g), 0.01 * torch.randn(n, generator=g),
            1e-3 * torch.rand(n, generator=g))


@pytest.mark.parametrize("n,misaligned", [(7, False), (8, False), (8, True), (4 * 16384 * 256 + 4, False)])
@pytest.mark.parametrize("t", [1, 1000])
def test_adam(n, misaligned, t):
    """mzba_adam and mzba_adam_dev (scalars as Learner._adam_scalars computes them) against the update formula in f64
    from the same f32-rounded scalars, with torch.optim.Adam in f32 on the CPU as the witness; the two entry points
    bit-identical. n = 7 and a 16-byte-misaligned n = 8 take the scalar kernel, n = 8 and 4 * 16384 * 256 + 4 (a second
    grid-stride pass) the float4 one. Chains: m' = m + (1 - b1) (g - m), g = grad + wd p: 5 operations on |m| + |g|;
    v' = b2 v + ((1 - b2) g) g: 8 relative (g's two enter squared); denom = sqrt(v') / bc2 + eps: 7 relative; the
    update U = neg_step m' / denom: |neg_step| 5 (|m| + |g|) / denom + 10 |U|; p' = p + U: one more on |p| + |U|."""
    from mzba.learner import ADAM_EPS, BETAS, WEIGHT_DECAY, Learner
    L = _lib()
    lr = 3e-4
    sc = Learner._adam_scalars(types.SimpleNamespace(lr=lr), t)
    assert len(sc) == 7 and sc[5] == ADAM_EPS and sc[6] == WEIGHT_DECAY
    p0, grad, m0, v0 = _adam_data(n)
    ns_, omb1, b2, omb2, bc, eps, wd = [float(np.float32(s)) for s in sc]
    p64, g64, m64, v64 = p0.double(), grad.double(), m0.double(), v0.double()
    gg = g64 + wd * p64
    m1 = m64 + omb1 * (gg - m64)
    v1 = v64 * b2 + (omb2 * gg) * gg
    den = v1.sqrt() / bc + eps
    upd = (ns_ * m1) / den
    p1 = p64 + upd
    cs_m = 5 * (m64.abs() + gg.abs())
    cs_v = 8 * v1
    cs_p = abs(ns_) * cs_m / den + 10 * upd.abs() + (p64.abs() + upd.abs())
    del gg, den, upd
    # witness: torch.optim.Adam, single-tensor, f32, CPU
    pw = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pw], lr=lr, betas=BETAS, eps=ADAM_EPS, weight_decay=WEIGHT_DECAY)
    opt.state[pw] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    pw.grad = grad.clone()
    opt.step()
    mw, vw = opt.state[pw]["exp_avg"], opt.state[pw]["exp_avg_sq"]
    off = 1 if misaligned else 0
    got = []
    for dev_scalars in (False, True):
        bufs = []
        for src in (p0, grad, m0, v0):
            b = torch.zeros(n + 4, device="cuda")
            b[off:off + n] = src.cuda()
            bufs.append(b)
        views = [b[off:off + n] for b in bufs]
        assert all((v.data_ptr() % 16 != 0) == misaligned for v in views)
        if dev_scalars:
            scd = torch.tensor(sc, dtype=torch.float32, device="cuda")
            L.call("mzba_adam_dev", *[L.ptr(v) for v in views], n, L.ptr(scd), L.stream())
        else:
            L.call("mzba_adam", *[L.ptr(v) for v in views], n, *sc, L.stream())
        torch.cuda.synchronize()
        tag = f"adam{'_dev' if dev_scalars else ''} n {n} misaligned {int(misaligned)} t {t}"
        pk, gk, mk, vk = [v.cpu() for v in views]
        assert torch.equal(gk, grad)
        for b in bufs:  # nothing written outside the n elements
            assert (b[:off] == 0).all() and (b[off + n:] == 0).all()
        if not dev_scalars or n < 1 << 20:  # the large case's bounds once: adam_dev is bit-identical below
            _check(tag + " p", pk, p1, pw.detach(), cs_p)
            _check(tag + " m", mk, m1, mw, cs_m)
            _check(tag + " v", vk, v1, vw, cs_v)
        got.append((pk, mk, vk))
    for a, b in zip(*got):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ====================================================================== learner inputs
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("Cp", [8, 16])
def test_learner_input(dtype, Cp):
    """mzba_learner_input: out [B][HW][Cp] = (lut8[frame code & 7] x L, past action / 3 x L, zeros) for B = 5 windows
    whose slots point into a ring of 9 rows, exactly; frame codes above 3 and above 7 (masked with & 7); out pre-filled
    with NaN so an unwritten element shows."""
    L = _lib()
    B, Lh, HW, cap = 5, 4, 20, 9
    g = _gen(21, dtype, Cp)
    states = torch.randint(0, 256, (cap, Lh, HW), generator=g).to(torch.uint8)
    states[0, 0, :8] = torch.arange(8, dtype=torch.uint8)
    past = torch.randint(0, 3, (cap, Lh), generator=g)
    slots = torch.randperm(cap, generator=g)[:B].to(torch.int32)
    lut = torch.tensor([0.0, 0.3, 0.6, 1.0, 0.123456, 0.7, 0.9, 0.05])
    out = torch.full((B, HW, Cp), float("nan"), device="cuda").to(_tdt(dtype))
    sd, pd, sl, ld = states.cuda(), past.cuda(), slots.cuda(), lut.cuda()
    L.call("mzba_learner_input", dtype, L.ptr(sd), L.ptr(pd), L.ptr(sl), L.ptr(ld), L.ptr(out), B, Lh, HW, Cp, L.stream())
    torch.cuda.synchronize()
    exp = torch.zeros(B, HW, Cp)
    s = slots.long()
    exp[:, :, :Lh] = lut[(states[s].long() & 7)].permute(0, 2, 1)
    exp[:, :, Lh:2 * Lh] = (past[s].float() / 3.0)[:, None, :]
    assert (states[s] > 7).any() and ((states[s] & 7) > 3).any()
    assert torch.equal(out.cpu(), exp.to(_tdt(dtype)))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("k", [0, 4])
def test_dyn_input(dtype, k):
    """mzba_dyn_input: out [B][HW][40] = (h's 32 channels, one-hot(future_actions[slots[b]][k]) x 3, zeros), exactly, at
    the first and last unroll step of K = 5."""
    L = _lib()
    B, HW, C, A, Cp, K, cap = 5, 20, 32, 3, 40, 5, 9
    g = _gen(22, dtype, k)
    h = torch.randn(B, HW, C, generator=g).to(_tdt(dtype))
    fut = torch.randint(0, A, (cap, K), generator=g)
    slots = torch.randperm(cap, generator=g)[:B].to(torch.int32)
    out = torch.full((B, HW, Cp), float("nan"), device="cuda").to(_tdt(dtype))
    hd, fd, sl = h.cuda(), fut.cuda(), slots.cuda()
    L.call("mzba_dyn_input", dtype, L.ptr(hd), L.ptr(fd), L.ptr(sl), K, k, L.ptr(out), B, HW, C, A, Cp, L.stream())
    torch.cuda.synchronize()
    exp = torch.zeros(B, HW, Cp)
    exp[:, :, :C] = h.float()
    exp[:, :, C:C + A] = F.one_hot(fut[slots.long(), k], A).float()[:, None, :]
    assert torch.equal(out.cpu(), exp.to(_tdt(dtype)))


# ====================================================================== batched weight pack
# (Cout, taps, Cin, N, Cc, flip, layout, pad): both layouts, plain and flipped, 1x1 and 3x3, Cc < Cin, N < Cin
PACK_JOBS = [(32, 9, 32, 32, 32, 0, 1, 8), (64, 1, 35, 64, 32, 0, 1, 0), (32, 9, 64, 64, 32, 1, 1, 16),
             (16, 9, 64, 16, 64, 0, 2, 8), (32, 9, 48, 48, 32, 1, 2, 0)]


def _pack_numpy(w, Cout, taps, Cin, N, Cc, flip, layout, pad):
    """include/mzba.h's layout comment in numpy: logical W'[n][tap][c] = flip ? w[c][taps-1-tap][n] : w[n][tap][c]
    (N x Cc); layout 1: out[ct][kh][tap][cc][h][r][j] = W'[32ct + r][tap][kh Cc/2 + 16cc + 8h + j]; layout 2:
    out[ct][s][g][r][j] = W'[16ct + r] at k' = 32s + 8g + j, k' = q Cc + c with the taps in (dx, dy) order,
    tap = (q % 3) * 3 + q / 3; then `pad` zeros."""
    wp = w[:Cc, ::-1, :N].transpose(2, 1, 0) if flip else w[:N, :, :Cc]
    if layout == 1:
        o = wp.reshape(N // 32, 32, taps, 2, Cc // 32, 2, 8).transpose(0, 3, 2, 4, 5, 1, 6)
    else:
        order = [(q % 3) * 3 + q // 3 for q in range(9)]
        o = wp[:, order, :].reshape(N // 16, 16, taps * Cc // 32, 4, 8).transpose(0, 2, 3, 1, 4)
    flat = np.concatenate([np.ascontiguousarray(o).reshape(-1), np.zeros(pad, np.float32)])
    return torch.from_numpy(flat).to(torch.bfloat16)


@pytest.mark.parametrize("njobs", [1, 32, 33])
def test_conv_pack_bf16_multi(njobs):
    """mzba_conv_pack_bf16_multi (32 jobs per launch: 33 takes a second one) over mixed shapes, flips and layouts:
    every output bit-identical to the pack the test computes in numpy from the header's layout comment (layout 1 also
    to mzba.agent.pack_lat, host Python), nothing written past an output's end."""
    from mzba.agent import LAT_PAD_ELEMS, pack_lat
    L = _lib()
    g = _gen(23, njobs)
    jobs = [PACK_JOBS[(j + njobs) % len(PACK_JOBS)] for j in range(njobs)]
    ws, outs, exps = [], [], []
    for Cout, taps, Cin, N, Cc, flip, layout, pad in jobs:
        w = torch.randn(Cout, taps, Cin, generator=g)
        exp = _pack_numpy(w.numpy(), Cout, taps, Cin, N, Cc, flip, layout, pad)
        assert exp.numel() == N * taps * Cc + pad
        if layout == 1 and not flip and Cc == Cin:  # the host packer on the bf16-rounded weights
            host = pack_lat(w.bfloat16().float().numpy().reshape(Cout, -1), Cout, int(round(taps ** 0.5)), Cin)
            assert np.array_equal(host[:-LAT_PAD_ELEMS], exp[:N * taps * Cc].float().numpy())
        ws.append(w.cuda())
        outs.append(torch.full((exp.numel() + 8,), -1, dtype=torch.int16, device="cuda"))  # 8 guard elements
        exps.append(exp)
    wp = (ctypes.c_void_p * njobs)(*[t.data_ptr() for t in ws])
    op = (ctypes.c_void_p * njobs)(*[t.data_ptr() for t in outs])
    prm = (ctypes.c_int * (8 * njobs))(*[v for jb in jobs for v in jb])
    L.call("mzba_conv_pack_bf16_multi", wp, op, prm, njobs, L.stream())
    torch.cuda.synchronize()
    for j, (o, e) in enumerate(zip(outs, exps)):
        o = o.cpu()
        assert torch.equal(o[:e.numel()], e.view(torch.int16)), (j, jobs[j])
        assert (o[e.numel():] == -1).all(), (j, jobs[j])
