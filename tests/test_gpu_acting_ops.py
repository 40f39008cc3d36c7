"""The acting side's small kernels (csrc/heads.hip: the Linear heads in their three forms with the fused softmax /
support decode, and mzba_support_decode; csrc/conv.hip: mzba_scale_state, mzba_avgpool2, the generic mzba_conv2d
kernel), each called through the C ABI and compared with a float64 evaluation of the same operation on the CPU (plain
torch) from the same, already rounded, inputs. No mzba_* entry point serves as a reference for another; where two are
compared bit for bit (the fused decode with mzba_support_decode, a fallback with the form it falls back to) that stands
beside the f64 comparison, not in its place. The cases, references and c S terms live in tests/acting_cases.py;
tests/test_cpu_acting_cases.py shows on the CPU that they are not vacuous.

Error bounds (the idiom of tests/test_gpu_learner_ops.py). e_k is the kernel's error against f64, e_w the error of a
plain torch f32 CPU evaluation of the same operation (the witness) against the same reference. For an f32 output

    e_k <= 4 e_w + c 2^-24 S

with S the magnitude of the terms that enter the result and c the number of f32 operations on the kernel's longest
dependent chain, counted from the source and stated at each test (every product an MFMA sums counts as one operation);
where an intermediate's error is amplified on its way out — the softmax quotient, the decode's 2 (|x| + 0.999) — c S
is that propagation written out (acting_cases.softmax_ref, decode_ref). A bf16 output adds one bf16 rounding of the
reference, 2^-8 |ref|. Operations that are exact are compared with torch.equal. Every test prints its e_k and e_w
(pytest -s). Outputs are over-allocated and pre-filled with a sentinel; what lies outside the written part is asserted
untouched."""
import contextlib
import itertools
import os

import pytest
import torch

import acting_cases as A
from ops_bounds import _check, _gen

pytestmark = pytest.mark.gpu

SENT = -768.0  # pre-fill of every output: exact in f32 and bf16, outside every result's range
torch.set_num_threads(min(16, os.cpu_count() or 1))


def _lib():
    from mzba import _lib as L
    return L


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _sentinel(shape, dtype=torch.float32):
    return torch.full(shape, SENT, device="cuda").to(dtype)


# ====================================================================== heads
@contextlib.contextmanager
def _heads_variant(v):
    L = _lib()
    assert L.lib().mzba_heads_set_variant(v) == 0
    try:
        yield
    finally:
        L.lib().mzba_heads_set_variant(1)


def _launch_heads(form, B, heads, misalign_x=False):
    """One launch of `form` over heads = [(x, w, bias, K, O, decode, with_logits)] (CPU tensors; x's first B rows). The
    outputs have 16 to 31 sentinel rows past B, asserted untouched. Returns [(logits or None, dec)] on the CPU."""
    L = _lib()
    rows = (B + 15) // 16 * 16 + 16
    keep, args, outs = [], [], []
    for x, w, bias, K, O, dec, with_logits in heads:
        xs = x[:B].contiguous()
        if misalign_x:  # a view starting one element (4 bytes) into a 16-byte-aligned buffer
            buf = torch.zeros(B * K + 4, dtype=xs.dtype, device="cuda")
            xd = buf[1:1 + B * K]
            xd.copy_(xs.flatten())
            assert xs.dtype == torch.float32 and xd.data_ptr() % 16 == 4
        else:
            xd = xs.cuda()
            assert xd.data_ptr() % 16 == 0
        if form == "bf16_mfma":  # [16][K] bf16 with rows >= O zero, as agent.py packs it
            wd = torch.zeros(16, K, dtype=torch.bfloat16, device="cuda")
            wd[:O] = w.cuda()
        else:
            wd = w.cuda()
        bd = bias.cuda()
        lg = _sentinel((rows, O)) if with_logits else None
        dc = _sentinel((rows,) if dec else (rows, O))
        keep += [xd, wd, bd]
        outs.append((lg, dc))
        args += [L.ptr(xd), L.ptr(wd), L.ptr(bd), K, O, dec, L.ptr(lg), L.ptr(dc)]
    if len(heads) == 1:
        args += [None, None, None, 0, 0, 0, None, None]
    if form == "bf16_mfma":
        L.call("mzba_heads_bf16", len(heads), *args, A.SMIN, A.SMAX, B, L.stream())
    else:
        L.call("mzba_heads", int(form == "bf16_fma"), len(heads), *args, A.SMIN, A.SMAX, B, L.stream())
    torch.cuda.synchronize()
    res = []
    for lg, dc in outs:
        for t in (lg, dc):
            assert t is None or (t[B:] == SENT).all(), "rows >= B written"
        res.append((None if lg is None else lg[:B].cpu(), dc[:B].cpu()))
    return res


def _support_decode(l):
    """mzba_support_decode of CPU logits l [rows][n] -> CPU [rows] (8 sentinel elements past the end stay untouched)."""
    L = _lib()
    rows, n = l.shape
    ld, out = l.contiguous().cuda(), _sentinel((rows + 8,))
    L.call("mzba_support_decode", L.ptr(ld), L.ptr(out), rows, n, A.SMIN, A.SMAX, L.stream())
    torch.cuda.synchronize()
    assert (out[rows:] == SENT).all()
    return out[:rows].cpu()


def _check_head(tag, form, B, head, lg, dc):
    """One head's outputs: the logits against f64 x . W^T + b; the softmax / the value decode against f64 from the
    logits the launch wrote (rows sum to 1 within the summed bound; the decode also bit-equal to mzba_support_decode)."""
    x, w, bias, K, O, dec, _ = head
    ref, wit, S = A.head_logits_ref(x[:B], w, bias)
    _check(f"{tag} logits", lg, ref, wit, A.heads_c(form, K) * S)
    if dec == 0:
        p, pw, cS = A.softmax_ref(lg)
        _check(f"{tag} softmax", dc, p, pw, cS)
        _check(f"{tag} softmax row sums", dc.double().sum(-1), p.sum(-1), pw.double().sum(-1), cS.sum(-1))
    else:
        r, rw, cS, xe = A.decode_ref(lg)
        assert A.x_gap_ok(xe), tag
        _check(f"{tag} decode", dc, r, rw, cS)
        assert _same_bits(dc, _support_decode(lg)), f"{tag}: fused decode != mzba_support_decode"


def _heads_of(form, launch, ki, regime):
    """The launch's heads; the second head takes the next K of the form's list, so the two differ."""
    Ks = A.HEAD_K[form]
    heads = []
    for j, (O, dec, with_logits) in enumerate(launch):
        K = Ks[(ki + j) % len(Ks)]
        heads.append(A.head_case(form, K, O, regime, j) + (K, O, dec, with_logits))
    return heads


def _run_head_launch(tag, form, B, heads, regime):
    full = _launch_heads(form, B, [h[:6] + (True,) for h in heads])
    if not all(h[6] for h in heads):  # a null logits pointer changes nothing else
        part = _launch_heads(form, B, heads)
        for h, (lg, dc), (lg2, dc2) in zip(heads, part, full):
            assert (lg is None) == (not h[6]) and _same_bits(dc, dc2) and (lg is None or _same_bits(lg, lg2)), tag
    for j, (h, (lg, dc)) in enumerate(zip(heads, full)):
        _check_head(f"{tag} head {j} K {h[3]} O {h[4]}", form, B, h, lg, dc)
        if regime == "gaps" and h[4] > 3:  # the tied outputs: same weight row, same bias, same operations
            assert torch.equal(lg[:, 2], lg[:, 3])
            if h[5] == 0:
                assert (dc == 0).any() and torch.equal(dc[:, 2], dc[:, 3])  # exp underflowed to exact zeros


@pytest.mark.parametrize("B", A.HEAD_B)
@pytest.mark.parametrize("form", A.HEAD_FORMS)
def test_heads(form, B):
    """mzba_heads f32 under both mzba_heads_set_variant values (f32_fma: heads_kernel<float>, f32_mfma:
    heads_mfma_f32_kernel), mzba_heads dtype 1 (bf16_fma: heads_kernel<bf16_t>) and mzba_heads_bf16 (bf16_mfma:
    heads_mfma_kernel), at B on the tile edges of the 8- and 16-env workgroups, K of 1 / 17 / 320 (f32) or 1 / 9 / 160
    (bf16) MFMA steps, O in {2, 3, 11, 16} each as a policy and as supports, one and two heads per launch, a null
    logits pointer, random weights and weights whose logits lie 150 apart with ties.

    c (acting_cases.heads_c): FMA forms 2 ceil(K / 256) + 9; f32 MFMA 4 ceil(K / 128) + 8; bf16 MFMA 32 ceil(K / 256) + 9,
    on S = |b| + sum |x w|. Softmax and decode: acting_cases.softmax_ref / decode_ref, from the logits written."""
    with _heads_variant(0 if form == "f32_fma" else 1):
        for regime, ki, launch in itertools.product(A.HEAD_REGIMES, range(3), A.HEAD_LAUNCHES):
            heads = _heads_of(form, launch, ki, regime)
            _run_head_launch(f"heads {form} B {B} {regime}", form, B, heads, regime)


@pytest.mark.parametrize("B", [9, 37])
def test_heads_f32_fallbacks_take_the_fma_form(B):
    """mzba_heads f32 with the MFMA variant selected falls back to heads_kernel<float> when K % 16 != 0 (K = 40) or x is
    not 16-byte aligned (a view one float in, K = 272): bit-equal to the variant-0 launch of the same inputs, which is
    itself checked against f64 (c = 2 ceil(K / 256) + 9). That the comparison can tell the forms apart: at K = 272,
    aligned, the two variants differ in some logit."""
    def heads_at(K):
        return [A.head_case("f32_fma", K, 11, "random", 0) + (K, 11, 1, True),
                A.head_case("f32_fma", K, 3, "random", 1) + (K, 3, 0, True)]
    for K, mis in ((A.HEAD_K_FALLBACK, False), (272, True)):
        heads = heads_at(K)
        with _heads_variant(0):
            fma = _launch_heads("f32_fma", B, heads)
        fall = _launch_heads("f32_mfma", B, heads, misalign_x=mis)
        for j, (h, (lg, dc), (lg2, dc2)) in enumerate(zip(heads, fma, fall)):
            _check_head(f"heads f32 fallback K {K} misaligned {int(mis)} B {B} head {j}", "f32_fma", B, h, lg2, dc2)
            assert _same_bits(lg, lg2) and _same_bits(dc, dc2), (K, mis, j)
    heads = heads_at(272)
    with _heads_variant(0):
        fma = _launch_heads("f32_fma", B, heads)
    mfma = _launch_heads("f32_mfma", B, heads)
    assert not all(_same_bits(a[0], b[0]) for a, b in zip(fma, mfma))


def test_heads_bf16_rejects_k_not_a_multiple_of_32():
    """mzba_heads_bf16 with K % 32 != 0 (either head) returns -1 and launches nothing: the outputs keep their sentinel."""
    L = _lib()
    B = 5
    x = torch.zeros(B, 64, dtype=torch.bfloat16, device="cuda")
    w = torch.zeros(16, 64, dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(16, device="cuda")
    lg, dc = _sentinel((B, 3)), _sentinel((B, 3))
    one = [L.ptr(x), L.ptr(w), L.ptr(b), 48, 3, 0, L.ptr(lg), L.ptr(dc)]
    ok = [L.ptr(x), L.ptr(w), L.ptr(b), 64, 3, 0, L.ptr(lg), L.ptr(dc)]
    f = L.lib().mzba_heads_bf16
    assert f(1, *one, None, None, None, 0, 0, 0, None, None, A.SMIN, A.SMAX, B, L.stream()) == -1
    assert f(2, *ok, *one, A.SMIN, A.SMAX, B, L.stream()) == -1
    torch.cuda.synchronize()
    assert (lg == SENT).all() and (dc == SENT).all()


# ====================================================================== support decode
def _transforms(n):
    from mzba.scalar import ScalarTransforms
    return ScalarTransforms({"supports_min": A.SMIN, "supports_max": A.SMAX, "num_supports": n})


@pytest.mark.parametrize("rows", A.DECODE_ROWS)
@pytest.mark.parametrize("n", A.DECODE_N)
def test_support_decode(n, rows):
    """mzba_support_decode and ScalarTransforms.inverted_softmax_expectation (bit-equal to it) on (-5, 5) with 2, 11
    and 16 supports, 1 row and rows around the 256-thread block, against the f64 decode over the f32 values of
    torch.linspace: random rows, one logit 40 above the rest at every index (both ends saturated), -inf everywhere but
    one index (x exactly 0 at n = 11: the result is 0), logits offset by +-1e4. c S: acting_cases.decode_ref. At
    n = 16 the kernel's supports smin + i step differ from torch.linspace's by one f32 ulp in places; the bound's
    support term (3 |i step| + |sup|, the kernel's own roundings) covers it, the kernel is left as it is."""
    l = A.decode_rows(n, rows)
    ref, wit, cS, x = A.decode_ref(l)
    assert A.x_gap_ok(x)
    got = _support_decode(l)
    _check(f"support_decode n {n} rows {rows}", got, ref, wit, cS)
    assert (got[x == 0] == 0).all()
    via = _transforms(n).inverted_softmax_expectation(l)
    assert via.device.type == "cpu" and _same_bits(via, got)


def test_support_decode_leading_dimensions_empty_input_and_rejects():
    """A (4, 6, 11) input gives (4, 6); an empty (0, n) input gives an empty (0,) tensor and (3, 0, n) gives (3, 0), as
    the reference's torch ops do; more than 16 supports raise; the C ABI rejects n > 16, n < 2 and rows < 1 by return
    code (nothing is launched)."""
    L = _lib()
    l = A.decode_rows(11, 24)
    ref, wit, cS, x = A.decode_ref(l)
    assert A.x_gap_ok(x)
    st = _transforms(11)
    got = st.inverted_softmax_expectation(l.view(4, 6, 11))
    assert got.shape == (4, 6)
    _check("support_decode (4, 6, 11)", got.reshape(24), ref, wit, cS)
    for shape in ((0, 11), (3, 0, 11)):
        e = st.inverted_softmax_expectation(torch.empty(shape))
        assert e.shape == shape[:-1] and e.dtype == torch.float32
        e = st.inverted_softmax_expectation(torch.empty(shape, device="cuda"))
        assert e.shape == shape[:-1] and e.device.type == "cuda"
    with pytest.raises(RuntimeError):
        _transforms(17).inverted_softmax_expectation(torch.zeros(3, 17))
    with pytest.raises(RuntimeError):
        _transforms(17).inverted_softmax_expectation(torch.zeros(0, 17))
    ld, out = torch.zeros(4, 17, device="cuda"), _sentinel((8,))
    f = L.lib().mzba_support_decode
    assert f(L.ptr(ld), L.ptr(out), 4, 17, A.SMIN, A.SMAX, L.stream()) == -1
    assert f(L.ptr(ld), L.ptr(out), 4, 1, A.SMIN, A.SMAX, L.stream()) == -1
    assert f(L.ptr(ld), L.ptr(out), 0, 11, A.SMIN, A.SMAX, L.stream()) == -1
    torch.cuda.synchronize()
    assert (out == SENT).all()


# ====================================================================== min-max scale
SCALE_SLOTS = 5
SCALE_SLOT_ARR = (4, 0, 2, 1, 3)  # distinct, non-monotone


@pytest.mark.parametrize("dtype,n,form", A.SCALE_CASES)
def test_scale_state(dtype, n, form):
    """mzba_scale_state at the sizes on both sides of its dispatch (register form: scale_state_kernel; two-pass form:
    scale_state_big_kernel; acting_cases.scale_form restates the condition), B in {1, 4, 5} (a wave per env, four per
    workgroup), without a pool, with slot_const = 3 and with a per-env slot_arr, over random, constant (every output
    exactly 0), min-first / max-last, all-negative and 1e-6-wide latents. f32: bit-equal to the op-by-op torch f32 chain
    (h - min) / ((max - min) + 1e-8), as csrc/common.h claims; both types against f64 with c = 4 (two operations for the
    denominator, a subtract, a divide) on S = 1. The pool (pool_env_stride > slots x slot_stride, slot_stride > n,
    sentinel-filled) equals the sentinel everywhere but the written slots, which are bit-equal to out; h is unchanged."""
    L = _lib()
    assert A.scale_form(dtype, n) == form
    t = A.tdt(dtype)
    h = A.scale_input(dtype, n)
    ref, wit, c = A.scale_ref(h)
    slot_stride = (n + 7) // 8 * 8 + 8
    env_stride = SCALE_SLOTS * slot_stride + 16
    const = A.SCALE_KINDS.index("constant")
    for rows in [list(range(5)), list(range(4))] + [[k] for k in range(5)]:
        B = len(rows)
        for mode in ("none", "const", "arr"):
            tag = f"scale_state dtype {dtype} n {n} {form} rows {rows[0]}-{rows[-1]} pool {mode}"
            hd = h[rows].cuda()
            out = _sentinel((B + 1, n), t)
            pool = _sentinel((B * env_stride + 8,), t) if mode != "none" else None
            slots = list(SCALE_SLOT_ARR[:B]) if mode == "arr" else [3] * B
            sd = torch.tensor(slots, dtype=torch.int32, device="cuda") if mode == "arr" else None
            L.call("mzba_scale_state", dtype, L.ptr(hd), L.ptr(out), L.ptr(pool), env_stride, L.ptr(sd), 3, slot_stride,
                   B, n, L.stream())
            torch.cuda.synchronize()
            assert torch.equal(hd.cpu(), h[rows]) and (out[B] == SENT).all(), tag
            got = out[:B].cpu()
            if dtype == 0:
                assert _same_bits(got, wit[rows]), tag + ": f32 differs from the op-by-op torch chain"
            _check(tag, got, ref[rows], wit[rows], c, out_bf16=bool(dtype))
            if const in rows:
                assert (got[rows.index(const)] == 0).all()
            if pool is not None:
                exp = torch.full((B * env_stride + 8,), SENT).to(t)
                for b, s in enumerate(slots):
                    o = b * env_stride + s * slot_stride
                    exp[o:o + n] = got[b]
                assert _same_bits(pool, exp), tag + ": pool"


# ====================================================================== avg-pool forward
def _avgpool_case(dtype, B, H, W, C):
    L = _lib()
    t = A.tdt(dtype)
    x = torch.randn(B, H, W, C, generator=_gen(35, dtype, B, H, W, C)).to(t)
    ref, wit, S = A.pool_ref(x)
    n = ref.numel()
    xd, out = x.cuda(), _sentinel((n + 8,), t)
    L.call("mzba_avgpool2", dtype, L.ptr(xd), L.ptr(out), B, H, W, C, L.stream())
    torch.cuda.synchronize()
    assert (out[n:] == SENT).all() and torch.equal(xd.cpu(), x)
    _check(f"avgpool2 dtype {dtype} B {B} {H}x{W} C {C}", out[:n].cpu().view(ref.shape), ref, wit, 3 * S, out_bf16=bool(dtype))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("C", A.POOL_C)
@pytest.mark.parametrize("H,W", A.POOL_HW)
def test_avgpool2_forward(dtype, C, H, W):
    """mzba_avgpool2 against f64 avg_pool2d(2, 2): a single output pixel, the shipping 16 x 20, and 5 x 7, where the odd
    row and column are dropped; C = 6 and 8. Chain: three adds and an exact division by 4: c = 3 on the mean of |x|."""
    _avgpool_case(dtype, 3, H, W, C)


@pytest.mark.parametrize("dtype", [0, 1])
def test_avgpool2_forward_second_grid_pass(dtype):
    """129 x 8 x 8 x 256 outputs are more than the 8192 x 256 threads of the capped grid: the grid-stride loop runs a
    second pass."""
    B, H, W, C = A.POOL_BIG
    assert B * (H // 2) * (W // 2) * C > 8192 * 256
    _avgpool_case(dtype, B, H, W, C)


# ====================================================================== generic conv edges
@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("idx", range(5))
def test_conv2d_generic_edges(dtype, idx):
    """mzba_conv2d on conv_igemm_kernel (mzba_conv2d_set_variant(0)) at acting_cases.conv_shapes: a ragged last K-step
    in every case, Cin of one 16-B chunk, four valid output columns, a second N tile of 4 columns, a second M tile of
    12 rows, a 1 x 1 and a one-row image, 1x1 with Cin no multiple of BK; with and without the residual and ReLU, a slot
    gather (non-monotone, repeated slots, in_slot_stride > HW Cin, in_env_stride > S in_slot_stride, the unread slots
    NaN) and an action-bias table [HW][3][Cout] with every action occurring, against an f64 conv of the stored operands
    plus bias, action bias and residual. c = ceil(Ktot / BK) BK + 3 (every product of a K-step, then the epilogue's
    three adds) on S from the conv of the absolute values; bf16 outputs add 2^-8 |ref|."""
    L = _lib()
    c = A.conv_case(dtype, idx)
    B, H, W, Cin, Cout, ks = c["shape"]
    HW, t = H * W, A.tdt(dtype)
    cc = A.conv_c(dtype, Cin, ks)
    slot_stride = HW * Cin + 16
    env_stride = A.CONV_S * slot_stride + 32
    src = torch.full((B, env_stride), float("nan")).to(t)
    for b in range(B):
        s = int(c["slots"][b])
        src[b, s * slot_stride:s * slot_stride + HW * Cin] = c["pool"][b, s].flatten()
    inputs = {False: (A.conv_input(c, False).cuda(), HW * Cin, None, 0),
              True: (src.cuda(), env_stride, c["slots"].cuda(), slot_stride)}
    wd, bd, rd, td = c["w"].cuda(), c["bias"].cuda(), c["res"].cuda(), c["tab"].cuda()
    acts = [(torch.arange(B) + r) % A.CONV_A for r in range(1 if B >= A.CONV_A else A.CONV_A)]
    assert set(torch.cat(acts).tolist()) == set(range(A.CONV_A))
    combos = [(False, res, relu, None) for res, relu in itertools.product((False, True), (0, 1))]
    combos += [(True, True, 1, None), (True, False, 0, None)]
    combos += [(g, res, relu, a) for a in acts for g, res, relu in ((False, False, 0), (True, True, 1))]
    assert L.lib().mzba_conv2d_set_variant(0) == 0
    try:
        for gather, with_res, relu, act in combos:
            xin, es, slot, ss = inputs[gather]
            ad = act.to(torch.int32).cuda() if act is not None else None
            out = _sentinel((B * HW + 1, Cout), t)
            L.call("mzba_conv2d", dtype, L.ptr(xin), es, L.ptr(slot), ss, L.ptr(wd), L.ptr(bd),
                   L.ptr(td) if act is not None else None, L.ptr(ad), A.CONV_A if act is not None else 0,
                   L.ptr(rd) if with_res else None, L.ptr(out), B, H, W, Cin, Cout, ks, relu, L.stream())
            torch.cuda.synchronize()
            assert (out[B * HW] == SENT).all()
            ref, wit, S = A.conv_ref(c, A.conv_input(c, gather), with_res, relu, act)
            tag = (f"conv2d generic dtype {dtype} {c['shape']} gather {int(gather)} res {int(with_res)} relu {relu} "
                   f"act {None if act is None else act.tolist()}")
            _check(tag, out[:B * HW].cpu(), ref, wit, cc * S, out_bf16=bool(dtype))
    finally:
        L.lib().mzba_conv2d_set_variant(1)
