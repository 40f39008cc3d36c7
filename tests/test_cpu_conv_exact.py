"""The exact-grid cases of tests/exact_cases.py, on the CPU: every case of tests/test_gpu_conv_exact.py is generated
and its certificate asserted (the builders assert it conv by conv; here is where "the reference alone stays within
the condition" is settled), the coverage properties the cases promise are checked, a plain f32 evaluation in two
different K orders shows the order independence the argument claims, and a few deliberate defects show that the
rounded reference moves when a single product moves."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_cases as X
from exact_cases import BF16, FP16


def _bf16_case_ok(c, pre=None, dt=BF16):
    ties, nonrep = X.tie_stats(c["pre"] if pre is None else pre, dt)
    assert ties >= 1 and nonrep >= 1, (c["name"], ties, nonrep)


def _gather_ok(c):
    if c.get("S1", 1) > 1:
        slot = c["slot"].tolist()
        assert len(set(slot)) == min(c["B"], c["S1"]), (c["name"], slot)
        if c["B"] >= 3:
            assert any(a > b for a, b in zip(slot, slot[1:])) and any(a < b for a, b in zip(slot, slot[1:]))
    if c.get("act") is not None:
        assert len(set(c["act"].tolist())) == min(c["B"], c["A"]), (c["name"], c["act"])


def _dense_ok(c):
    pairs, taps = X.covers_taps(c["w"])
    assert pairs and taps, c["name"]


def _sparse_ok(c, ws):
    for w in ws:
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert int((w != 0).sum(dim=(1, 2, 3)).min()) >= 9
        pairs, taps = X.covers_taps(w)
        assert pairs and taps, c["name"]
    # a dead (or never clipped) chain tests nothing: the share of non-zeros after the chain's last ReLU
    alive = (c.get("last_relu", c["pre"]) != 0).float()
    assert 0.1 <= float(alive.mean()) <= 0.9, (c["name"], float(alive.mean()))
    per_channel = alive.mean(dim=(0, 2, 3))  # and no output channel all dead or never clipped (B >= 3: 60+ elements)
    if c["B"] >= 3:
        assert 0.05 <= float(per_channel.min()) and float(per_channel.max()) <= 0.95, (c["name"], per_channel)


@pytest.mark.parametrize("B,nb,gather", X.TOWER_CASES)
def test_tower_cases(B, nb, gather):
    c = X.tower_case(B, nb, gather)
    _sparse_ok(c, c["ws"])
    _gather_ok(c)
    _bf16_case_ok(c)


@pytest.mark.parametrize("B,elem", X.TOWER_FUSED_CASES)
def test_tower_fused_cases(B, elem):
    c = X.tower_case(B, 2, 1, fused=True, elem=elem)
    _sparse_ok(c, c["ws"] + [c["w0"]])
    _gather_ok(c)
    assert set(c["act"].tolist()) == {0, 1, 2}
    _bf16_case_ok(c, dt=FP16 if elem else BF16)  # the store that rounds the f32 sum: the fp16 image at elem 1


@pytest.mark.parametrize("p", X.LAT_CASES)
def test_lat_cases(p):
    c = X.lat_case(*p)
    _dense_ok(c)
    _gather_ok(c)
    _bf16_case_ok(c)


@pytest.mark.parametrize("p", X.LAT_BN_CASES)
def test_lat_bn_cases(p):
    c = X.lat_bn_case(*p)
    _dense_ok(c)
    _bf16_case_ok(c)
    _bf16_case_ok(c, pre=c["pre1"])
    kept = float((c["y"] > 0).float().mean())
    assert 0.2 < kept < 0.6 and bool((c["ref2"].float()[c["y"] <= 0] == 0).all())


@pytest.mark.parametrize("p", X.FLIP_CASES)
def test_flip_cases(p):
    c = X.flip_case(*p)
    assert all(X.covers_taps(c["wt"]))
    _bf16_case_ok(c)


@pytest.mark.parametrize("p", X.HALO_CASES)
def test_halo_cases(p):
    c = X.halo_case(*p)
    _dense_ok(c)
    _bf16_case_ok(c)


@pytest.mark.parametrize("p", X.HALO_GATHER_CASES)
def test_halo_gather_cases(p):
    c = X.halo_gather_case(*p)
    _dense_ok(c)
    _gather_ok(c)
    _bf16_case_ok(c)


@pytest.mark.parametrize("p", X.BAND_CASES)
def test_band_cases(p):
    c = X.band_case(*p)
    _dense_ok(c)
    _bf16_case_ok(c)


@pytest.mark.parametrize("build,cases", [(X.band_res_case, X.BAND_RES_CASES), (X.rep_blocks_case, X.REP_BLOCKS_CASES),
                                         (X.rep_trunk_case, X.REP_TRUNK_CASES)], ids=["band_res", "rep_blocks", "rep_trunk"])
def test_chain_cases(build, cases):
    for p in cases:
        c = build(*p)
        _sparse_ok(c, c["ws"])
        _bf16_case_ok(c)


@pytest.mark.parametrize("p", X.WGRAD_CASES)
def test_wgrad_cases(p):
    c = X.wgrad_case(1, *p[:6])
    assert float(c["dw"].abs().max()) < 2 ** 24 and torch.equal(c["dw"], c["dw"].round())


@pytest.mark.parametrize("p", X.WGRAD_SEGS_CASES)
def test_wgrad_segs_cases(p):
    c = X.wgrad_case(*p, 256, 3)
    assert float(c["dw"].abs().max()) < 2 ** 24 and torch.equal(c["db"], c["db"].round())


@pytest.mark.parametrize("p", X.XT_CASES)
def test_xt_cases(p):
    c = X.xt_case(*p)
    _dense_ok(c)
    _gather_ok(c)


@pytest.mark.parametrize("p", X.XP_CASES)
def test_xp_cases(p):
    _dense_ok(X.xp_case(*p))


@pytest.mark.parametrize("form", X.X2_FORMS)
@pytest.mark.parametrize("two", ["x", "w"])
def test_two_part_cases(form, two):
    """The two-part operand needs more than 11 significant bits (the low part of a bf16 / fp16 split is live), the
    other operand is single-part, and the output is not on the integer grid (the low parts reach it)."""
    c = X.x2_case(form, two)
    t = c["pool"] if two == "x" else c["w"][c["w"] != 0]
    for dt in (BF16, FP16):
        assert bool((t.float().to(dt).double() != t).all()), (c["name"], dt)
    other = c["w"] if two == "x" else c["pool"]
    assert torch.equal(other, other.round())
    assert all(X.covers_taps(c["w"]))
    out = c["ref"].double()[c["ref"] != 0]
    assert float((out != out.round()).float().mean()) > 0.8
    assert 0.1 <= float((c["ref"] != 0).float().mean()) <= 0.9


def test_margins_printed():
    """The smallest 2^24 q / (sum of magnitudes) of every case family generated above (informational; each case has
    asserted its own certificate). m = 16 with three residual blocks passes with orders of magnitude to spare."""
    c = X.tower_case(33, 3, 1)
    assert X.MARGINS[c["name"]] > 100.0, X.MARGINS[c["name"]]
    for k, v in sorted(X.MARGINS.items()):
        print(f"{k}: margin {v:.3g}")


# --------------------------------------------------------------------------------------------- order independence
def _f32_blocked(x, w, order, init):
    """A plain f32 numpy conv (3x3 or 1x1, zero padding): K = (tap, 32-channel block) steps taken in `order`, every
    step's 32 products added one at a time into an f32 accumulator that starts at `init` [B][Cout][H][W]."""
    x64, w64 = x.numpy(), w.numpy()
    x, w = x64.astype(np.float32), w64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64) and np.array_equal(w.astype(np.float64), w64)
    B, Cin, H, W = x.shape
    ks = w.shape[-1]
    p = ks // 2
    xp = np.zeros((B, Cin, H + 2 * p, W + 2 * p), np.float32)
    xp[:, :, p:p + H, p:p + W] = x
    acc = init.numpy().astype(np.float32).copy()
    for s in order:
        tap, blk = divmod(int(s), Cin // 32)
        ky, kx = divmod(tap, ks)
        for ci in range(32 * blk, 32 * blk + 32):
            prod = xp[:, None, ci, ky:ky + H, kx:kx + W] * w[None, :, ci, ky, kx, None, None]
            acc = (acc + prod).astype(np.float32)
    return acc


def _orders_agree(x, w, terms, pre, relu):
    nsteps = w.shape[-1] ** 2 * (x.shape[1] // 32)
    init = sum(terms)
    fwd = np.arange(nsteps)
    perm = np.random.default_rng(5).permutation(nsteps)
    want = pre.float().numpy()
    for order in (fwd, perm):
        got = _f32_blocked(x, w, order, init)
        if relu:
            got = np.maximum(got, 0)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_order_independence_dense():
    c = X.lat_case(1, 4, 5, 256, 256, 3, 1, 1, 1, 1)
    x = X.nchw(c["pool"][torch.arange(1), c["slot"].long()])
    terms = [c["b"].view(1, -1, 1, 1).expand(1, -1, 4, 5), X.table_rows(c["tab"], c["act"], 4, 5), X.nchw(c["res"])]
    _orders_agree(x, c["w"], terms, c["pre"], True)


def test_order_independence_sparse_chain():
    """The last conv of a three-block tower: its input is the reference's own rounded intermediate."""
    c = X.tower_case(3, 3, 1)
    x = X.nchw(c["pool"][torch.arange(3), c["slot"].long()])
    for k in range(3):
        if k:
            x = X.rnd(pre, BF16).double()  # noqa: F821
        t = X.rnd(X.conv_step("oi", x, c["ws"][2 * k], c["bs"][2 * k], relu=True), BF16).double()
        pre = X.conv_step("oi", t, c["ws"][2 * k + 1], c["bs"][2 * k + 1], res=x, relu=True)
    assert torch.equal(pre, c["pre"])
    _orders_agree(t, c["ws"][5], [c["bs"][5].view(1, -1, 1, 1).expand(3, -1, 4, 5), x], pre, True)


def test_order_independence_two_part():
    c = X.x2_case("x6t", "x")
    x = X.nchw(c["pool"][:, 0])
    _orders_agree(x, c["w"], [c["b"].view(1, -1, 1, 1).expand(3, -1, 4, 5), X.nchw(c["res"])], c["pre"], True)


# --------------------------------------------------------------------------------------------- sensitivity
def test_sensitivity_of_the_rounded_reference():
    """One dense case: dropping a single (tap, cin, cout) product, or swapping two input channels, changes the rounded
    reference; nudging one exact tie by the smallest representable input change flips its bf16."""
    c = X.lat_case(7, 4, 5, 256, 160, 3, 0, 0, 1, 0)
    x, w, b, res = X.nchw(c["pool"][:, 0]), c["w"], c["b"].view(1, -1, 1, 1), X.nchw(c["res"])
    ref = X.rnd(F.conv2d(x, w, padding=1) + b + res, BF16)
    assert torch.equal(X.nhwc(ref), c["ref"])
    co, ci, ky, kx = [int(v) for v in (w != 0).nonzero()[777]]
    w2 = w.clone()
    w2[co, ci, ky, kx] = 0
    r2 = X.rnd(F.conv2d(x, w2, padding=1) + b + res, BF16)
    diff = (r2.view(torch.int16) != ref.view(torch.int16))
    assert diff.any() and diff.any(dim=(0, 2, 3)).nonzero().flatten().tolist() == [co]
    x3 = x.clone()
    x3[:, [5, 6]] = x[:, [6, 5]]
    r3 = X.rnd(F.conv2d(x3, w, padding=1) + b + res, BF16)
    assert (r3.view(torch.int16) != ref.view(torch.int16)).any()
    # an exact tie whose centre tap is non-zero: one grid step (1) on one input moves the sum by |w| >= 1 off the tie
    pre = c["pre"]
    r = ref.double()
    d = pre - r
    tie = (d != 0) & ((r + 2 * d).float().to(BF16).double() == r + 2 * d)
    found = False
    for e, o, y, xx in tie.nonzero().tolist():
        cin = (w[o, :, 1, 1] != 0).nonzero()
        cin = [int(k) for k in cin.flatten() if abs(float(x[e, int(k), y, xx])) < 3]
        if not cin:
            continue
        for step in (1.0, -1.0):
            x4 = x.clone()
            x4[e, cin[0], y, xx] += step
            p4 = (F.conv2d(x4[e:e + 1], w[o:o + 1], padding=1) + b[:, o:o + 1] + res[e:e + 1, o:o + 1])[0, 0, y, xx]
            assert p4 != pre[e, o, y, xx]
            found = found or X.rnd(p4, BF16).view(torch.int16) != ref[e, o, y, xx].view(torch.int16)
        break
    assert found


def test_assert_bits_equal_reports_the_tile(capsys):
    a = torch.zeros(3, 4, 5, 32, dtype=BF16)
    b = a.clone()
    b[2, 1:3, 4, 16:20] = 1.0
    X.assert_bits_equal("same", a, a.clone(), ("env", "y", "x", "channel"))
    with pytest.raises(AssertionError) as e:
        X.assert_bits_equal("tile", b, a, ("env", "y", "x", "channel"))
    msg = str(e.value)
    assert "8 of 1920 elements differ" in msg and "env: 2" in msg and "y: 1-2" in msg and "channel: 16-19" in msg
    assert "channel blocks of 16: 1" in msg and "(env 2, y 1, x 4, channel 16): got 1.0 want 0.0" in msg
    # -0.0 and +0.0 differ as bits
    with pytest.raises(AssertionError):
        X.assert_bits_equal("zero", -a.float(), a.float(), ("env", "y", "x", "channel"))
