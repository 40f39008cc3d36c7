"""The MFMA convolution kernels against a rounded f64 reference, bit for bit, on inputs whose f32 sums are exact
(tests/exact_cases.py states the argument, the grids and the certificate; tests/test_cpu_conv_exact.py checks the
cases themselves). Under the certificate, which every case asserts on the reference side before its kernel runs, any
summation order, MFMA shape and split gives the exact sum, so the one rounding is the final store and there is no
tolerance anywhere in this file: a wrong index, a skipped tap, a stale LDS row or a wrong tie is an inequality at a
named (env, y, x, channel), printed with the differing set's extent by exact_cases.assert_bits_equal.

Every case asserts its kernel's *_supported(...) == 1 first: a refused shape is an error in the case list. Every
process-wide switch is put back in a `finally` (the _switch context manager). The shapes are the smallest that cross
each kernel's tile edges. Out of scope: mzba_rep_tail and the fused head epilogues (their min-max scaling and softmax
divide) and the BN statistics of mzba_conv_lat_bn (means and variances are not sums on a grid)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import exact_cases as X
from exact_cases import BF16, FP16, F32, assert_bits_equal

pytestmark = pytest.mark.gpu

NHWC = ("env", "y", "x", "channel")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"


@contextlib.contextmanager
def _switch(name, value, default):
    from mzba import _lib as L
    assert getattr(L.lib(), name)(value) == 0, (name, value)
    try:
        yield
    finally:
        getattr(L.lib(), name)(default)


def _dev(t, dt):
    return None if t is None else t.to(dt).contiguous().cuda()


def _pack(arr, dt):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(dt).cuda()


def _nan(shape, dt):
    return torch.full(tuple(shape), float("nan"), device="cuda").to(dt)


def _tap_major(w):
    """OIHW -> [Cout][tap (ky, kx)][Cin], flattened per output channel."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).numpy()


def _tower_wf(ws, dt):
    from mzba.agent import pack_tower_conv
    from mzba.weights import LAT_PAD_ELEMS
    return _pack(np.concatenate([pack_tower_conv(w.numpy()) for w in ws] + [np.zeros(LAT_PAD_ELEMS)]), dt)


def _src(c, dt):
    """(device pool, env stride, device slot or None, slot stride) of a case's input."""
    n = c["pool"][0, 0].numel()
    if c["S1"] == 1:
        return _dev(c["pool"][:, 0], dt), n, None, 0
    return _dev(c["pool"], dt), c["S1"] * n, c["slot"].cuda(), n


def _sync_equal(name, out, c, ref=None):
    torch.cuda.synchronize()
    ref = c["ref"] if ref is None else ref
    assert_bits_equal(name, out.view(ref.shape), ref, c["dims"])


# ------------------------------------------------------------------------------------------------ towers
@pytest.mark.parametrize("B,nb,gather", X.TOWER_CASES)
def test_tower_exact(B, nb, gather):
    """mzba_towerp (16 envs per workgroup) and mzba_tower's plans 1, 2, 3 (4 / 8 / 4 envs), each against the
    reference, never against each other: sparse grid, C 256, 4x5, with and without the slot gather."""
    from mzba import _lib as L
    c = X.tower_case(B, nb, gather)
    pool, es, slot, ss = _src(c, BF16)
    ss = ss or 20 * 256
    wf, b = _tower_wf(c["ws"], BF16), _dev(torch.cat(c["bs"]), F32)
    out = _nan((B, 20 * 256), BF16)
    L.call("mzba_towerp", L.ptr(pool), es, L.ptr(slot), ss, L.ptr(out), L.ptr(wf), L.ptr(b), nb, B, L.stream())
    _sync_equal(c["name"] + " towerp", out, c)
    for plan in (1, 2, 3):
        out = _nan((B, 20 * 256), BF16)
        with _switch("mzba_tower_set_variant", plan, 0):
            assert L.lib().mzba_tower_plan(B) == plan
            L.call("mzba_tower", L.ptr(pool), es, L.ptr(slot), ss, L.ptr(out), L.ptr(wf), L.ptr(b), nb, B, None, 0,
                   L.stream())
            torch.cuda.synchronize()
        _sync_equal(f"{c['name']} plan {plan}", out, c)


@pytest.mark.parametrize("B,elem", X.TOWER_FUSED_CASES)
def test_tower_fused_exact(B, elem):
    """mzba_towerp_fused and mzba_tower_fused (plans 1, 2, 3) with epilogue 0 and the dynamics prologue: the 3x3
    ConvBlock with the [20][A][256] action-bias table (A = 3, all actions present), then two blocks. elem 1: fp16 image
    and weights, the reference's intermediates rounded to fp16, latent in and out bf16 (towerp.hip's header)."""
    from mzba import _lib as L
    c = X.tower_case(B, 2, 1, fused=True, elem=elem)
    wdt = FP16 if elem else BF16
    pool, es, slot, ss = _src(c, BF16)
    wf, b = _tower_wf(c["ws"], wdt), _dev(torch.cat(c["bs"]), F32)
    w0, b0 = _tower_wf([c["w0"]], wdt), _dev(c["b0"], F32)
    tab, act = _dev(c["tab"], F32), c["act"].cuda()
    for plan in (4, 1, 2, 3):
        ext = L.TowerExt()
        ext.w0, ext.b0, ext.act_bias, ext.act, ext.A = L.addr(w0), L.addr(b0), L.addr(tab), L.addr(act), c["A"]
        ext.epilogue, ext.elem, ext.plan = 0, elem, plan
        out = _nan((B, 20 * 256), BF16)
        fn = "mzba_towerp_fused" if plan == 4 else "mzba_tower_fused"
        L.call(fn, L.ptr(pool), es, L.ptr(slot), ss, L.ptr(out), L.ptr(wf), L.ptr(b), 2, B, ctypes.byref(ext), L.stream())
        _sync_equal(f"{c['name']} plan {plan}", out, c)


# ------------------------------------------------------------------------------------------------ conv_lat
def _lat_wf(c):
    from mzba.agent import pack_lat
    return _pack(pack_lat(_tap_major(c["w"]), c["Cout"], c["ks"], c["Cin"]), BF16)


@pytest.mark.parametrize("p", X.LAT_CASES)
def test_conv_lat_exact(p):
    """mzba_conv_lat, dense grid: variants 0, 2 and 3, each against the reference; ragged last workgroups, the partial
    second 128-channel column block (Cout 160), gather / action bias / residual / ReLU on and off."""
    from mzba import _lib as L
    c = X.lat_case(*p)
    B, H, W, Cin, Cout, ks = p[:6]
    assert L.lib().mzba_conv_lat_supported(H, W, Cin, Cout, ks) == 1
    pool, es, slot, ss = _src(c, BF16)
    wf, b, tab, res = _lat_wf(c), _dev(c["b"], F32), _dev(c["tab"], F32), _dev(c["res"], BF16)
    act = None if c["act"] is None else c["act"].cuda()
    for variant in (0, 2, 3):
        out = _nan((B, H, W, Cout), BF16)
        with _switch("mzba_conv_lat_set_variant", variant, 0):
            L.call("mzba_conv_lat", L.ptr(pool), es, L.ptr(slot), ss, L.ptr(wf), L.ptr(b), L.ptr(tab), L.ptr(act),
                   c["A"] if tab is not None else 0, L.ptr(res), L.ptr(out), B, H, W, Cin, Cout, ks, c["relu"], L.stream())
            torch.cuda.synchronize()
        _sync_equal(f"{c['name']} variant {variant}", out, c)


@pytest.mark.parametrize("p", X.LAT_BN_CASES)
def test_conv_lat_bn_out_exact(p):
    """mzba_conv_lat_bn's `out` tensor in modes 0, 1 and 2 (the statistics stay with test_gpu_learner.py): mode 0
    conv + bias + res, mode 1 conv + bias, mode 2 bf16(conv + bias + res) [y > 0] written over its residual."""
    from mzba import _lib as L
    c = X.lat_bn_case(*p)
    B, H, W, Cin, Cout, ks = p
    assert L.lib().mzba_conv_lat_supported(H, W, Cin, Cout, ks) == 1 and Cout % 128 == 0
    x, wf, b, res = _dev(c["pool"][:, 0], BF16), _lat_wf(c), _dev(c["b"], F32), _dev(c["res"], BF16)
    y, xbn, mean = _dev(c["y"], BF16), _dev(c["xbn"], BF16), torch.zeros(4 * Cout, device="cuda")
    for variant in (0, 2, 3):
        with _switch("mzba_conv_lat_set_variant", variant, 0):
            nc, rpc = ctypes.c_int(), ctypes.c_int()
            L.call("mzba_conv_lat_bn_chunks", B, H, W, Cin, Cout, ks, ctypes.byref(nc), ctypes.byref(rpc))
            part = torch.zeros(nc.value * Cout * 2, device="cuda")
            o0, o1, o2 = _nan((B, H, W, Cout), BF16), _nan((B, H, W, Cout), BF16), res.clone()
            L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(b), L.ptr(res), L.ptr(o0), B, H, W, Cin, Cout, ks, 0,
                   None, None, None, None, None, None, 0, None, None, L.stream())
            L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(b), None, L.ptr(o1), B, H, W, Cin, Cout, ks, 1,
                   L.ptr(part), None, None, None, None, None, 0, None, None, L.stream())
            L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(b), L.ptr(o2), L.ptr(o2), B, H, W, Cin, Cout, ks, 2,
                   L.ptr(part), L.ptr(y), L.ptr(xbn), L.ptr(mean), None, None, 0, None, None, L.stream())
            torch.cuda.synchronize()
        for mode, o in enumerate((o0, o1, o2)):
            _sync_equal(f"{c['name']} variant {variant} mode {mode}", o, c, c[f"ref{mode}"])


@pytest.mark.parametrize("p", X.FLIP_CASES)
def test_conv_input_gradient_packs_exact(p):
    """The input-gradient use: mzba_conv_pack_bf16's flip = 1 pack (lat and band layouts) of integer master weights,
    run by mzba_conv_lat / mzba_conv_band on dy, against torch.nn.grad.conv2d_input."""
    from mzba import _lib as L
    from mzba.weights import LAT_PAD_ELEMS
    c = X.flip_case(*p)
    kind, H, W, Cin, Cout, ks = p
    B, taps = c["B"], ks * ks
    assert getattr(L.lib(), f"mzba_conv_{kind}_supported")(H, W, Cout, Cin, ks) == 1
    wd, dy, b = _dev(c["w"], F32), _dev(c["dy"], BF16), _dev(c["b"], F32)
    pack = torch.empty(Cin * taps * Cout + LAT_PAD_ELEMS, dtype=BF16, device="cuda")
    L.call("mzba_conv_pack_bf16", L.ptr(wd), L.ptr(pack), Cout, taps, Cin, Cin, Cout, 1, 1 if kind == "lat" else 2,
           LAT_PAD_ELEMS, L.stream())
    out = _nan((B, H, W, Cin), BF16)
    if kind == "lat":
        L.call("mzba_conv_lat", L.ptr(dy), H * W * Cout, None, 0, L.ptr(pack), L.ptr(b), None, None, 0, None, L.ptr(out),
               B, H, W, Cout, Cin, ks, 0, L.stream())
    else:
        L.call("mzba_conv_band", L.ptr(dy), L.ptr(pack), L.ptr(b), None, L.ptr(out), B, H, W, Cout, Cin, 0, L.stream())
    _sync_equal(c["name"], out, c)


# ------------------------------------------------------------------------------------------------ conv_halo
def _halo_wh(c):
    from mzba.agent import pack_lat16
    return _pack(pack_lat16(_tap_major(c["w"]), c["Cout"], 3, c["Cin"]), BF16)


@pytest.mark.parametrize("p", X.HALO_CASES)
def test_conv_halo_exact(p):
    """mzba_conv_halo, dense grid: forms 0, 1, 2 x waves 4, 8, each against the reference, and the residual aliasing
    `out`. The shapes are exact_cases.HALO_CASES (its comment names the two refused combinations and what stands in)."""
    from mzba import _lib as L
    c = X.halo_case(*p)
    B, H, W, Cin, Cout, relu, _ = p
    assert L.lib().mzba_conv_halo_supported(H, W, Cin, Cout, 3) == 1
    x, wh, b, res = _dev(c["pool"][:, 0], BF16), _halo_wh(c), _dev(c["b"], F32), _dev(c["res"], BF16)
    for form in (0, 1, 2):
        for nw in (4, 8):
            out = _nan((B, H, W, Cout), BF16)
            with _switch("mzba_conv_halo_set_form", form, 0), _switch("mzba_conv_halo_set_waves", nw, 0):
                L.call("mzba_conv_halo", L.ptr(x), L.ptr(wh), L.ptr(b), L.ptr(res), L.ptr(out), B, H, W, Cin, Cout, relu,
                       L.stream())
                torch.cuda.synchronize()
            _sync_equal(f"{c['name']} form {form} waves {nw}", out, c)
        if res is not None:
            inplace = res.clone()
            with _switch("mzba_conv_halo_set_form", form, 0):
                L.call("mzba_conv_halo", L.ptr(x), L.ptr(wh), L.ptr(b), L.ptr(inplace), L.ptr(inplace), B, H, W, Cin, Cout,
                       relu, L.stream())
                torch.cuda.synchronize()
            _sync_equal(f"{c['name']} form {form} in place", inplace, c)


@pytest.mark.parametrize("p", X.HALO_GATHER_CASES)
def test_conv_halo_gather_exact(p):
    """mzba_conv_halo_ex: the input gathered from S + 1 latents per env (non-monotone slots), the action-bias table,
    ReLU; 21x21, 256 -> 256; forms 0, 1, 2 x waves 4, 8."""
    from mzba import _lib as L
    c = X.halo_gather_case(*p)
    B, H, W, Cin, Cout = c["B"], 21, 21, 256, 256
    assert L.lib().mzba_conv_halo_ex_supported(H, W, Cin, Cout, 3, 1) == 1
    pool, es, slot, ss = _src(c, BF16)
    wh, b, tab, act = _halo_wh(c), _dev(c["b"], F32), _dev(c["tab"], F32), c["act"].cuda()
    for form in (0, 1, 2):
        for nw in (4, 8):
            out = _nan((B, H, W, Cout), BF16)
            with _switch("mzba_conv_halo_set_form", form, 0), _switch("mzba_conv_halo_set_waves", nw, 0):
                L.call("mzba_conv_halo_ex", L.ptr(pool), es, L.ptr(slot), ss, L.ptr(wh), L.ptr(b), L.ptr(tab), L.ptr(act),
                       c["A"], None, L.ptr(out), B, H, W, Cin, Cout, 1, L.stream())
                torch.cuda.synchronize()
            _sync_equal(f"{c['name']} form {form} waves {nw}", out, c)


# ------------------------------------------------------------------------------------------------ band family
@pytest.mark.parametrize("p", X.BAND_CASES)
def test_conv_band_exact(p):
    """mzba_conv_band at 16x20, dense grid: every supported (Cin, Cout), 5- and 10-column bands."""
    from mzba import _lib as L
    c = X.band_case(*p)
    B, Cin, Cout, _, relu = p
    assert L.lib().mzba_conv_band_supported(16, 20, Cin, Cout, 3) == 1
    x, wf, b, res = _dev(c["pool"][:, 0], BF16), _tower_wf([c["w"]], BF16), _dev(c["b"], F32), _dev(c["res"], BF16)
    for xt in (5, 10):
        out = _nan((B, 16, 20, Cout), BF16)
        with _switch("mzba_conv_band_set_xt", xt, 5):
            L.call("mzba_conv_band", L.ptr(x), L.ptr(wf), L.ptr(b), L.ptr(res), L.ptr(out), B, 16, 20, Cin, Cout, relu,
                   L.stream())
            torch.cuda.synchronize()
        _sync_equal(f"{c['name']} xt {xt}", out, c)


@pytest.mark.parametrize("B,C", X.BAND_RES_CASES)
def test_conv_band_res_exact(B, C):
    from mzba import _lib as L
    c = X.band_res_case(B, C)
    assert L.lib().mzba_conv_band_res_supported(16, 20, C) == 1
    x = _dev(c["x"], BF16)
    w1, w2 = _tower_wf(c["ws"][:1], BF16), _tower_wf(c["ws"][1:], BF16)
    b1, b2 = _dev(c["bs"][0], F32), _dev(c["bs"][1], F32)
    out = _nan((B, 16, 20, C), BF16)
    L.call("mzba_conv_band_res", L.ptr(x), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2), L.ptr(out), B, 16, 20, C, L.stream())
    _sync_equal(c["name"], out, c)


@pytest.mark.parametrize("B,nb", X.REP_BLOCKS_CASES)
def test_rep_blocks_exact(B, nb):
    from mzba import _lib as L
    c = X.rep_blocks_case(B, nb)
    x, wf, b = _dev(c["x"], BF16), _tower_wf(c["ws"], BF16), _dev(torch.cat(c["bs"]), F32)
    out = _nan((B, 16, 20, 256), BF16)
    L.call("mzba_rep_blocks", L.ptr(x), L.ptr(out), L.ptr(wf), L.ptr(b), nb, B, L.stream())
    _sync_equal(c["name"], out, c)


@pytest.mark.parametrize("B,n0,n1", X.REP_TRUNK_CASES)
def test_rep_trunk_exact(B, n0, n1):
    from mzba import _lib as L
    c = X.rep_trunk_case(B, n0, n1)
    x = _dev(c["x"], BF16)
    wd = [_tower_wf([w], BF16) for w in c["ws"]]
    bd = [_dev(b, F32) for b in c["bs"]]
    wp = (ctypes.c_void_p * len(wd))(*[t.data_ptr() for t in wd])
    bp = (ctypes.c_void_p * len(bd))(*[t.data_ptr() for t in bd])
    out = _nan((B, 16, 20, 256), BF16)
    L.call("mzba_rep_trunk", L.ptr(x), L.ptr(out), wp, bp, n0, n1, B, L.stream())
    _sync_equal(c["name"], out, c)


# ------------------------------------------------------------------------------------------------ wgrad
def _wgrad_run(fn, c, dt, head):
    from mzba import _lib as L
    tdt = F32 if dt == "f32" else BF16
    xs, dys = [_dev(t, tdt) for t in c["xs"]], [_dev(t, tdt) for t in c["dys"]]
    dw, db = _dev(c["dw0"], F32), _dev(c["db0"], F32)
    nb = L.lib().mzba_conv_wgrad_ws_bytes(c["nseg"] * c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["ks"])
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    shape = (c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["ks"])
    if fn == "mzba_conv_wgrad":
        L.call(fn, 0 if dt == "f32" else 1, L.ptr(xs[0]), L.ptr(dys[0]), *shape, L.ptr(dw), L.ptr(db), L.ptr(ws), nb, L.stream())
    else:
        xp = (ctypes.c_void_p * c["nseg"])(*[t.data_ptr() for t in xs])
        dp = (ctypes.c_void_p * c["nseg"])(*[t.data_ptr() for t in dys])
        L.call(fn, 0 if dt == "f32" else 1, xp, dp, c["nseg"], *shape, L.ptr(dw), L.ptr(db), L.ptr(ws), nb, L.stream())
    torch.cuda.synchronize()
    assert_bits_equal(f"{c['name']} {head} dw", dw, c["dw"], ("cout", "tap", "cin"))
    assert_bits_equal(f"{c['name']} {head} db", db, c["db"], ("cout",))


@pytest.mark.parametrize("p", X.WGRAD_CASES)
def test_conv_wgrad_exact(p):
    """mzba_conv_wgrad, f32 and bf16, accumulated onto integer dw0 / db0: f32 outputs equal to the f64 reference."""
    c = X.wgrad_case(1, *p[:6])
    for dt in p[6]:
        _wgrad_run("mzba_conv_wgrad", c, dt, dt)


@pytest.mark.parametrize("p", X.WGRAD_SEGS_CASES)
def test_conv_wgrad_segs_exact(p):
    """mzba_conv_wgrad_segs (bf16, Cout 256): variants 1 and 2 x forms 0, 1, 2, 3. On this grid every form equals the
    reference, hence each other. At 5 x 512 envs variant 1 itself takes the whole-image kernel (nseg B >= 2048,
    wgrad.hip wgrad_img_eligible); variant 2 forces it for every shape its plan accepts."""
    c = X.wgrad_case(*p, 256, 3)
    for variant in (1, 2):
        for form in (0, 1, 2, 3):
            with _switch("mzba_conv_wgrad_set_variant", variant, 1), _switch("mzba_conv_wgrad_set_form", form, 2):
                _wgrad_run("mzba_conv_wgrad_segs", c, "bf16", f"variant {variant} form {form}")


# ------------------------------------------------------------------------------------------------ f32 parity convs
def _x_run(fn, c, wts, extra=()):
    from mzba import _lib as L
    pool, es, slot, ss = _src(c, F32)
    b, tab, res = _dev(c["b"], F32), _dev(c["tab"], F32), _dev(c["res"], F32)
    act = None if c["act"] is None else c["act"].cuda()
    B, H, W, Cin, Cout, ks = (c[k] for k in ("B", "H", "W", "Cin", "Cout", "ks"))
    out = _nan((B, H, W, Cout), F32)
    if fn == "mzba_conv_x6":
        assert slot is None and tab is None and ks == 3
        L.call(fn, L.ptr(pool), L.ptr(wts), L.ptr(b), L.ptr(res), L.ptr(out), B, H, W, Cin, Cout, c["relu"], L.stream())
    else:
        L.call(fn, L.ptr(pool), es, L.ptr(slot), ss, L.ptr(wts), *extra, L.ptr(b), L.ptr(tab), L.ptr(act),
               c["A"] if tab is not None else 0, L.ptr(res), L.ptr(out), B, H, W, Cin, Cout, ks, c["relu"], L.stream())
    torch.cuda.synchronize()
    return out


def _x_packs(c):
    from mzba.agent import split_pack_x6, split_pack_x3
    wn = _tap_major(c["w"])
    wx = split_pack_x6(wn, c["Cout"], c["ks"], c["Cin"]).cuda()
    wx3, wsc = split_pack_x3(wn, c["Cout"], c["ks"], c["Cin"])
    return wx, wx3.cuda(), wsc.cuda()


@pytest.mark.parametrize("p", X.XT_CASES)
def test_conv_x_pixel_tiled_exact(p):
    """mzba_conv_x6_ex (variant 3) and mzba_conv_x3_ex at the 4x5 latent, dense grid (integers are single-part
    operands, the x3 form's per-channel power-of-two scale is exact): f32 outputs equal to the reference; 4- and 8-wave
    workgroups, the x3 pipe 0 and 1; with and without gather + action bias, 3x3 and 1x1, Cout 256 and 128."""
    from mzba import _lib as L
    c = X.xt_case(*p)
    B, Cout, ks, mode = p
    ga = int(mode == "gather")
    assert L.lib().mzba_conv_x6_ex_supported(4, 5, 256, Cout, ks, ga) == 1
    assert L.lib().mzba_conv_x3_supported(4, 5, 256, Cout, ks, ga) == 1
    wx, wx3, wsc = _x_packs(c)
    for nw in (4, 8):
        with _switch("mzba_conv_x6_set_waves", nw, 0):
            with _switch("mzba_conv_x6_set_variant", 3, 2):
                out = _x_run("mzba_conv_x6_ex", c, wx)
            _sync_equal(f"{c['name']} x6 waves {nw}", out, c)
            for pipe in (0, 1):
                with _switch("mzba_conv_x3_set_pipe", pipe, 1):
                    out = _x_run("mzba_conv_x3_ex", c, wx3, (L.ptr(wsc),))
                _sync_equal(f"{c['name']} x3 waves {nw} pipe {pipe}", out, c)


@pytest.mark.parametrize("p", X.XP_CASES)
def test_conv_x_halo_forms_exact(p):
    """mzba_conv_x6 under variants 0 (per-read split), 1 (pre-split), 2 (default) and 3 (pixel-tiled where it applies)
    and mzba_conv_x3_ex on the pre-split tiles: 16x20 and 8x10 at B 1 / 3, and the 4x5 latent through the halo forms."""
    from mzba import _lib as L
    c = X.xp_case(*p)
    B, H, W, Cin, Cout = p[:5]
    assert L.lib().mzba_conv_x6_supported(H, W, Cin, Cout, 3) == 1
    assert L.lib().mzba_conv_x3_supported(H, W, Cin, Cout, 3, 0) == 1
    wx, wx3, wsc = _x_packs(c)
    for variant in (0, 1, 2, 3):
        with _switch("mzba_conv_x6_set_variant", variant, 2):
            out = _x_run("mzba_conv_x6", c, wx)
        _sync_equal(f"{c['name']} x6 variant {variant}", out, c)
    out = _x_run("mzba_conv_x3_ex", c, wx3, (L.ptr(wsc),))
    _sync_equal(f"{c['name']} x3", out, c)


@pytest.mark.parametrize("form", X.X2_FORMS)
@pytest.mark.parametrize("two", ["x", "w"])
def test_conv_x_two_part_exact(form, two):
    """The two-part grid, one case per form and per operand. conv_x6.hip keeps xh wh + xh wm + xm wh + xh wl + xm wm +
    xl wh and drops xm wl, xl wm, xl wl; the x3 form keeps xh wl + xl wh + xh wh. An operand i + j 2^-12 splits into
    hi = i and mid (bf16) / lo (fp16) = j 2^-12 with nothing below, so with the other operand a single-part integer the
    product is hi x hi + (mid or lo) x hi: both kept by both forms, whichever operand carries the two parts. Hence both
    choices run on every form ("x": two-part activations, sparse integer weights; "w": the mirror); two two-part
    operands at once would need xm wm / xl wl and are not asked of the x3 form."""
    from mzba import _lib as L
    c = X.x2_case(form, two)
    wx, wx3, wsc = _x_packs(c)
    H, W = c["H"], c["W"]
    if form in ("x3t", "x3p"):
        assert L.lib().mzba_conv_x3_supported(H, W, 256, 256, 3, 0) == 1
        out = _x_run("mzba_conv_x3_ex", c, wx3, (L.ptr(wsc),))
    else:
        assert L.lib().mzba_conv_x6_supported(H, W, 256, 256, 3) == 1
        with _switch("mzba_conv_x6_set_variant", {"x6t": 3, "x6p": 1, "x6r": 0}[form], 2):
            out = _x_run("mzba_conv_x6", c, wx)
    _sync_equal(c["name"], out, c)


# ------------------------------------------------------------------------------------------------ the net's own mesh
def test_one_dropped_product_is_seen_through_the_kernels():
    """What the comparison can see, shown through the kernels themselves: with one (tap, cin, cout) weight of the packed
    operand zeroed, conv_lat and towerp equal the reference of the altered weights bit for bit, and differ from the
    unaltered reference in that output channel only."""
    from mzba import _lib as L
    from mzba.agent import pack_lat
    c = X.lat_case(*X.LAT_CASES[1])
    B, H, W, Cin, Cout, ks = X.LAT_CASES[1][:6]
    co, ci, ky, kx = [int(v) for v in (c["w"] != 0).nonzero()[4321]]
    w2 = c["w"].clone()
    w2[co, ci, ky, kx] = 0
    ref2 = X.nhwc(X.rnd(X.conv_step("dropped", X.nchw(c["pool"][:, 0]), w2, c["b"], res=X.nchw(c["res"])), BF16))
    x, b, res = _dev(c["pool"][:, 0], BF16), _dev(c["b"], F32), _dev(c["res"], BF16)
    wf = _pack(pack_lat(_tap_major(w2), Cout, ks, Cin), BF16)
    out = _nan((B, H, W, Cout), BF16)
    L.call("mzba_conv_lat", L.ptr(x), H * W * Cin, None, 0, L.ptr(wf), L.ptr(b), None, None, 0, L.ptr(res), L.ptr(out),
           B, H, W, Cin, Cout, ks, 0, L.stream())
    torch.cuda.synchronize()
    assert_bits_equal("conv_lat, one weight zeroed", out, ref2, NHWC)
    with pytest.raises(AssertionError, match=rf"\n  channel: {co}\n"):
        assert_bits_equal("conv_lat vs the unaltered reference", out, c["ref"], NHWC)

    c = X.tower_case(16, 1, 1)
    co, ci, ky, kx = [int(v) for v in (c["ws"][1] != 0).nonzero()[1234]]
    w2 = c["ws"][1].clone()
    w2[co, ci, ky, kx] = 0
    x0 = X.nchw(c["pool"][torch.arange(16), c["slot"].long()])
    ref2 = X.nhwc(X.rnd(X.res_chain("dropped", x0, [c["ws"][0], w2], c["bs"], BF16), BF16))
    pool, es, slot, ss = _src(c, BF16)
    wf, b = _tower_wf([c["ws"][0], w2], BF16), _dev(torch.cat(c["bs"]), F32)
    out = _nan((16, 4, 5, 256), BF16)
    L.call("mzba_towerp", L.ptr(pool), es, L.ptr(slot), ss, L.ptr(out), L.ptr(wf), L.ptr(b), 1, 16, L.stream())
    torch.cuda.synchronize()
    assert_bits_equal("towerp, one weight zeroed", out, ref2, NHWC)
    with pytest.raises(AssertionError, match=rf"\n  channel: {co}\n"):
        assert_bits_equal("towerp vs the unaltered reference", out, c["ref"], NHWC)
