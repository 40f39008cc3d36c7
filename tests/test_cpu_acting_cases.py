"""The acting-ops cases do what tests/test_gpu_acting_ops.py needs them to (references alone, no GPU): no decode row
sits in the inverse transform's jump, every scale size lands on the form it is meant for, and the mistakes the cases
are there to catch — a dropped last k step of a head, a 16-B chunk left out of the min / max, a dropped conv tap or
ragged K-step — move the reference by more than the bound the GPU test allows."""
import itertools

import pytest
import torch

import acting_cases as A


def test_no_decode_row_sits_in_the_jump_at_zero():
    """Every row the GPU tests decode has x_ref == 0 or |x_ref| >= 1e-4; the special rows reach both saturated ends,
    every support, and an x of exactly 0."""
    for n, rows in itertools.product(A.DECODE_N, A.DECODE_ROWS):
        l = A.decode_rows(n, rows)
        ref, wit, cS, x = A.decode_ref(l)
        assert A.x_gap_ok(x), (n, rows, x[(x != 0) & (x.abs() < 1e-4)])
        assert torch.isfinite(ref).all() and torch.isfinite(cS).all() and torch.isfinite(wit).all()
        if rows > n + 3:
            sp = x[rows - (n + 3):]
            sup = torch.linspace(A.SMIN, A.SMAX, n).double()
            assert torch.allclose(sp[:n], sup, rtol=0, atol=1e-15), (n, sp[:n])
            assert sp[n] == sup[n // 2]
            assert (x == 0).any() == (n % 2 == 1)
            assert (l[-2:].abs() > 9e3).all() and torch.isinf(l).any()
    l = A.decode_rows(11, 24)
    assert A.x_gap_ok(A.decode_ref(l.view(4, 6, 11))[3])


def test_decode_supports_differ_from_linspace_by_at_most_the_counted_roundings():
    """smin + i step in f32 against torch.linspace's f32 values: equal at n = 2 and 11, up to one ulp apart at n = 16,
    within the 3 |i step| + |sup| roundings decode_ref counts."""
    import numpy as np
    for n in A.DECODE_N:
        lin = torch.linspace(A.SMIN, A.SMAX, n).numpy()
        step = np.float32(np.float32(A.SMAX) - np.float32(A.SMIN)) / np.float32(n - 1)
        fwd = (np.float32(A.SMIN) + np.arange(n, dtype=np.float32) * step).astype(np.float32)
        d = np.abs(fwd.astype(np.float64) - lin.astype(np.float64))
        allowed = A.U * (3 * np.abs(np.arange(n) * float(step)) + np.abs(lin.astype(np.float64)))
        print("n", n, "entries that differ", int((d > 0).sum()), "max", d.max())
        assert (d <= allowed).all()
        assert (d > 0).any() == (n == 16)


@pytest.mark.parametrize("form", A.HEAD_FORMS)
@pytest.mark.parametrize("regime", A.HEAD_REGIMES)
def test_dropping_a_heads_last_32_k_moves_a_logit_past_its_bound(form, regime):
    for K, O in itertools.product(A.HEAD_K[form] + ((A.HEAD_K_FALLBACK,) if form == "f32_fma" else ()), A.HEAD_O):
        x, w, bias = A.head_case(form, K, O, regime)
        ref, wit, S = A.head_logits_ref(x, w, bias)
        short = A.head_logits_ref(x, w, bias, kmax=max(K - 32, 0))[0]
        b = A.bound(ref, wit, A.heads_c(form, K) * S)
        moved = (short - ref).abs() > b
        print(form, regime, K, O, "logits moved past the bound:", float(moved.double().mean()))
        assert moved.any(1).all(), (form, regime, K, O)  # in every env row
        if regime == "gaps":
            srt = ref.sort(1)[0]
            gaps = srt[:, 1:] - srt[:, :-1]
            assert (gaps.max(1)[0] > 100).all()
            if O > 3:
                assert torch.equal(ref[:, 2], ref[:, 3])  # a tie
            p = A.softmax_ref(ref.float())[0]
            assert (p.float() == 0).any()  # exp underflows to an exact zero
        assert A.x_gap_ok(A.decode_ref(ref.float())[3]), (form, regime, K, O)  # the fused decode's rows


@pytest.mark.parametrize("dtype,n,form", A.SCALE_CASES)
def test_scale_sizes_land_on_their_form_and_the_last_chunk_matters(dtype, n, form):
    assert A.scale_form(dtype, n) == form
    epc, cpl = (8, 10) if dtype else (4, 20)
    if form == "register":
        assert n % epc == 0 and n // epc <= 64 * cpl
    if n == 5120:  # the last size the register form takes; the next aligned one is a two-pass case
        assert n // epc == 64 * cpl and (dtype, n + epc, "two_pass") in A.SCALE_CASES
    h = A.scale_input(dtype, n)
    ref, wit, c = A.scale_ref(h)
    k = A.SCALE_KINDS.index
    assert (ref[k("constant")] == 0).all() and (wit[k("constant")] == 0).all()
    assert ref[k("ends"), 0] == 0 and ref[k("ends")].argmax() == n - 1
    assert (h[k("narrow")].double().max() - h[k("narrow")].double().min()) <= 1e-6
    assert ref.min() >= 0 and ref.max() <= 1
    if n > epc:  # with a single chunk nothing is left to take the min / max of
        skip = n % epc or epc
        short = A.scale_ref(h, skip_last=skip)[0]
        b = A.bound(ref, wit, c, out_bf16=bool(dtype))
        r = k("ends")
        assert ((short[r] - ref[r]).abs() > b[r]).any(), (dtype, n)


@pytest.mark.parametrize("dtype", [0, 1])
def test_dropping_a_conv_tap_or_the_ragged_k_step_moves_every_case(dtype):
    bk = A.conv_bk(dtype)
    no_ragged = []
    for idx, (B, H, W, Cin, Cout, ks) in enumerate(A.conv_shapes(dtype)):
        c = A.conv_case(dtype, idx)
        Ktot = ks * ks * Cin
        nK = -(-Ktot // bk)
        assert Ktot % bk != 0, "the last K-step is ragged in every case"
        assert B < 3 or len(set(c["slots"].tolist())) < B  # a repeated slot wherever three envs allow one
        for gather in (False, True):
            x = A.conv_input(c, gather)
            ref, wit, S = A.conv_ref(c, x, True, 0)
            b = A.bound(ref, wit, A.conv_c(dtype, Cin, ks) * S, out_bf16=bool(dtype))
            centre = torch.ones(Ktot)
            centre[(ks * ks // 2) * Cin:(ks * ks // 2 + 1) * Cin] = 0  # the centre tap: in bounds at every pixel
            d = (A.conv_ref(c, x, True, 0, kmask=centre)[0] - ref).abs()
            assert (d > b).any(), ("centre tap", dtype, idx)
            last = torch.ones(Ktot)
            last[(nK - 1) * bk:] = 0
            d = (A.conv_ref(c, x, True, 0, kmask=last)[0] - ref).abs()
            taps = set(range((nK - 1) * bk // Cin, ks * ks))
            in_bounds = any(abs(t // ks - ks // 2) < H and abs(t % ks - ks // 2) < W for t in taps)
            if in_bounds:
                assert (d > b).any(), ("last K-step", dtype, idx)
            elif not gather:
                assert not d.any()
                no_ragged.append(idx)
        assert (A.conv_ref(c, A.conv_input(c, False), True, 0)[0] < 0).any()  # the ReLU has something to clamp
    # the last K-step of the 1 x 1 and of the one-row image holds only tap 8 (ky = +1), out of bounds at every pixel:
    # there the centre tap is the condition
    assert no_ragged == [1, 2]
