"""HIP learner against the reference's own training minibatches
(tests/golden/learner_*.npz, made by tests/golden/make_golden.py make_learner).

Forward: losses and logits against the reference's f32 values (rtol 2e-4 / atol 5e-5; the
reference's own f32 logits lie 1.5e-5 from an f64 evaluation, recorded in the fixture).

Gradients: against an f64 evaluation of the same algorithm (oracle/learner.py, bit-exact with
the reference in f32) run with the HIP learner's min/max positions of every _scale_state (the
min-max scale routes its min / max gradient to ONE element). The training loss is only
piecewise smooth (ReLU masks, min/max routing): at these small batches a relative parameter
perturbation of 1e-6 moves the f64 gradient by up to ~3 % (tools/learner_check.py), so any f32
evaluation — the reference's own included — may land that far from f64. The test therefore
measures the local kink scale with f64 probes at p * (1 + 1e-6 n) and requires, per tensor,
|ours - f64| <= 2e-4 max|f64| + 2 max_probe |f64(probe) - f64|. Away from kinks (small step 1)
the observed error is ~5e-6 of the tensor max. Biases of convolutions that feed a BatchNorm
have an exact gradient of 0 (BN subtracts the batch mean): checked to be rounding-noise sized.

Parameters after Adam: the update is checked against the torch single-tensor Adam restated
on the host from the learner's own gradients and moments (the oracle's / reference's op order),
and bounded by 2 lr against the reference (first-step updates are ~lr * sign(g)). BN running
statistics (forward only): rtol 1e-4 vs the reference. Step 2 starts from the reference's
post-step-1 parameters, running stats and Adam moments (teacher forcing).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle.fixtures import load_npz_parts

pytestmark = pytest.mark.gpu


def _mb(z, s):
    return {k.split("/")[-1]: z[k] for k in z.files if k.startswith(f"s{s}/in/")}


def _pre_bn_bias(k):
    return k.endswith((".conv1.bias", ".conv2.bias", ".conv.bias"))


def _f64_grads(ln, mcfg, start_sd, mb, K, probes=2, seed=0):
    """f64 gradients at start_sd with the learner's scale routing, and the per-tensor kink scale:
    max over probes of |f64(p (1 + 1e-6 n)) - f64(p)|."""
    from oracle.learner import LearnerOracle
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    idx = ln.scale_indices()

    def run(sd):
        o = LearnerOracle(mcfg, sd, K=K, dtype=torch.float64)
        o.force_index = idx
        return o.gradients(mb)[2]
    g0 = run(start_sd)
    spread = {k: np.zeros(()) for k in g0}
    rng = np.random.default_rng(seed)
    for _ in range(probes):
        sd = {}
        for k, v in start_sd.items():
            a = np.asarray(v)
            if a.dtype == np.float32 and not k.endswith(("running_mean", "running_var")):
                a = a.astype(np.float64) * (1 + 1e-6 * rng.standard_normal(a.shape))
            sd[k] = a
        g1 = run(sd)
        for k in g0:
            spread[k] = np.maximum(spread[k], np.abs(g1[k].numpy() - g0[k].numpy()).max())
    return g0, spread


def _check_grads(grads, g64, spread):
    for k, g in grads.items():
        t = g64[k].numpy()
        if _pre_bn_bias(k):
            wmax = np.abs(g64[k[: -len("bias")] + "weight"].numpy()).max()
            assert np.abs(g.numpy()).max() <= 1e-4 * wmax, (k, np.abs(g.numpy()).max(), wmax)
            continue
        e = np.abs(g.numpy().astype(np.float64) - t).max()
        bound = 2e-4 * np.abs(t).max() + 2 * float(spread[k])
        assert e <= bound, (k, e, np.abs(t).max(), float(spread[k]))


def _adam_expect(p, g, m, v, t, lr):
    """torch single-tensor Adam (weight_decay 1e-4) on host f32 tensors (the oracle's op order)."""
    b1, b2 = 0.9, 0.999
    g = g.add(p, alpha=1e-4)
    m = m.lerp(g, 1 - b1)
    v = v.mul(b2).addcmul(g, g, value=1 - b2)
    denom = (v.sqrt() / ((1 - b2 ** t) ** 0.5)).add(1e-8)
    return p.addcdiv(m, denom, value=-(lr / (1 - b1 ** t)))


def _check_update(before, opt_before, grads, after, t, lr):
    st = opt_before["state"]
    for i, (k, g) in enumerate(grads.items()):
        m = torch.as_tensor(st[i]["exp_avg"]) if i in st else torch.zeros_like(g)
        v = torch.as_tensor(st[i]["exp_avg_sq"]) if i in st else torch.zeros_like(g)
        exp = _adam_expect(torch.as_tensor(np.asarray(before[k], np.float32)), g, m.float(), v.float(), t, lr)
        torch.testing.assert_close(after[k], exp, rtol=1e-6, atol=lr * 1e-5, msg=k)


def _check_vs_reference(sd, ref_of, lr):
    for k, v in sd.items():
        got, refp = v.numpy().astype(np.float64), ref_of(k).astype(np.float64)
        if k.endswith(("running_mean", "running_var")):
            np.testing.assert_allclose(got, refp, rtol=1e-4, atol=1e-6, err_msg=k)
        elif k.endswith("num_batches_tracked"):
            assert int(got) == int(refp), k
        else:
            assert np.abs(got - refp).max() <= 2.0 * lr * 1.001, (k, np.abs(got - refp).max() / lr)


def test_learner_small_matches_reference():
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner, MinibatchRing
    from mzba.weights import init_state_dict
    z = load_npz_parts(GOLDEN, "learner_small")
    mcfg, K, lr = learner_model_cfg(), int(z["K"]), float(z["lr"])
    start = init_state_dict(mcfg, int(z["seed"]))
    ln = Learner(mcfg, start, K=K)
    for s in (1, 2):
        if s == 2:  # teacher forcing: the reference's state after step 1
            start = {k[len("s1/param/"):]: z[k] for k in z.files if k.startswith("s1/param/")}
            ln.load_state_dict(start)
            ln.load_optimizer_state_dict({"state": {i: {"step": 1.0, "exp_avg": z[f"s1/opt/exp_avg/{k}"],
                                                        "exp_avg_sq": z[f"s1/opt/exp_avg_sq/{k}"]}
                                                    for i, k in enumerate(ln.params)}})
        before, opt_before = ln.state_dict(), ln.optimizer_state_dict()
        ring = MinibatchRing(_mb(z, s))
        loss = ln.train_minibatch(ring, ring.slots()).cpu().numpy()
        ref = np.array([float(z[f"s{s}/{k}"]) for k in ("loss", "rl", "vl", "pl")])
        np.testing.assert_allclose(loss, ref, rtol=2e-4, atol=2e-5)
        for got, key in zip(ln.last_logits, ("pr", "pv", "pp")):
            np.testing.assert_allclose(got.cpu().numpy().transpose(1, 0, 2), z[f"s{s}/{key}"], rtol=2e-4, atol=5e-5)
        grads = ln.gradients()
        g64, spread = _f64_grads(ln, mcfg, start, _mb(z, s), K, probes=3)
        _check_grads(grads, g64, spread)
        after = ln.state_dict()
        _check_update(before, opt_before, grads, after, s, lr)
        _check_vs_reference(after, lambda k: z[f"s{s}/param/{k}"], lr)


def test_learner_full_matches_reference():
    """Full-width nets (B = 4), step 1: losses vs the reference, every gradient vs f64, sampled
    parameters and running stats vs the reference."""
    from mzba.config import default_config
    from mzba.learner import Learner, MinibatchRing
    from mzba.weights import init_state_dict
    z = load_npz_parts(GOLDEN, "learner_full")
    mcfg, K, lr = default_config()["model"], int(z["K"]), float(z["lr"])
    start = init_state_dict(mcfg, int(z["seed"]))
    ln = Learner(mcfg, start, K=K)
    before, opt_before = ln.state_dict(), ln.optimizer_state_dict()
    ring = MinibatchRing(_mb(z, 1))
    loss = ln.train_minibatch(ring, ring.slots()).cpu().numpy()
    ref = np.array([float(z[f"s1/{k}"]) for k in ("loss", "rl", "vl", "pl")])
    np.testing.assert_allclose(loss, ref, rtol=2e-4, atol=2e-5)
    grads = ln.gradients()
    g64, spread = _f64_grads(ln, mcfg, start, _mb(z, 1), K, probes=2)
    _check_grads(grads, g64, spread)
    after = ln.state_dict()
    _check_update(before, opt_before, grads, after, 1, lr)
    for k, v in after.items():
        got = v.numpy().reshape(-1)[z[f"s1/idx/{k}"]].astype(np.float64)
        refv = z[f"s1/param_at/{k}"].astype(np.float64)
        if k.endswith(("running_mean", "running_var")):
            # B = 4 full-width forward: two f32 evaluations differ by ~1e-3 in the logits
            np.testing.assert_allclose(got, refv, rtol=1e-3, atol=1e-4, err_msg=k)
        elif not k.endswith("num_batches_tracked"):
            assert np.abs(got - refv).max() <= 2.0 * lr * 1.001, k


def test_learner_state_and_optimizer_roundtrip():
    """state_dict / optimizer_state_dict (reference checkpoint formats) round trip: a learner
    rebuilt from them continues bit-identically."""
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner, MinibatchRing
    from mzba.weights import init_state_dict
    z = load_npz_parts(GOLDEN, "learner_small")
    mcfg = learner_model_cfg()
    sd0 = init_state_dict(mcfg, 3)
    ln = Learner(mcfg, sd0, K=int(z["K"]))
    for k, v in ln.state_dict().items():
        np.testing.assert_array_equal(v.numpy(), np.asarray(sd0[k]), err_msg=k)
    ring = MinibatchRing(_mb(z, 1))
    ln.train_minibatch(ring, ring.slots())
    sd, od = ln.state_dict(), ln.optimizer_state_dict()
    assert sorted(od["state"]) == list(range(len(ln.params))) and od["param_groups"][0]["weight_decay"] == 1e-4
    ln2 = Learner(mcfg, sd, K=int(z["K"]))
    ln2.load_optimizer_state_dict(od)
    a = ln.train_minibatch(ring, ring.slots()).cpu()
    b = ln2.train_minibatch(ring, ring.slots()).cpu()
    torch.testing.assert_close(a, b, rtol=0, atol=0)
    sd2 = ln2.state_dict()
    for k, v in ln.state_dict().items():
        torch.testing.assert_close(v, sd2[k], rtol=0, atol=0, msg=k)


def test_checkpoint_carries_learner_optimizer_state(tmp_path):
    """save_checkpoint(learner=...) writes the learner's Adam state in the reference's format;
    load_checkpoint(learner=...) restores weights and moments, so training continues bit-identically."""
    from mzba.agent import MuZeroAgent
    from mzba.checkpoint import save_checkpoint, load_checkpoint
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner, MinibatchRing
    from mzba.weights import init_state_dict
    z = load_npz_parts(GOLDEN, "learner_small")
    mcfg = learner_model_cfg()
    ln = Learner(mcfg, init_state_dict(mcfg, 3), K=int(z["K"]))
    ring = MinibatchRing(_mb(z, 1))
    ln.train_minibatch(ring, ring.slots())
    ag = MuZeroAgent(mcfg, dtype="f32")
    ag.load_state_dict(ln.state_dict())
    p = str(tmp_path / "ck.pth")
    save_checkpoint(p, ag, learner=ln, training_iteration=1)
    ln2 = Learner(mcfg, init_state_dict(mcfg, 99), K=int(z["K"]))
    load_checkpoint(p, learner=ln2)
    a = ln.train_minibatch(ring, ring.slots()).cpu()
    b = ln2.train_minibatch(ring, ring.slots()).cpu()
    torch.testing.assert_close(a, b, rtol=0, atol=0)


def _random_ring(B, L, K, seed):
    from mzba.learner import MinibatchRing
    g = np.random.default_rng(seed)
    lut = np.array([0, 0.3, 0.6, 1.0], np.float32)
    mb = dict(states=lut[g.integers(0, 4, (B, L, 16, 20)) * (g.random((B, L, 16, 20)) < 0.3)],
              past_actions=g.integers(0, 3, (B, L)), future_actions=g.integers(0, 3, (B, K)),
              rewards=g.choice(np.array([-1, 0, 0, 1, 5], np.float32), (B, K)),
              targets=(g.normal(size=(B, K)) * 2).astype(np.float32),
              counts=g.multinomial(50, [0.3, 0.3, 0.4], (B, K)).astype(np.float32))
    return MinibatchRing(mb)


def test_learner_bf16_tracks_f32():
    """bf16 activations / conv weights (f32 BN statistics, gradients, Adam state, master weights)
    vs the f32 path on a 256-window minibatch of the narrow config: loss within 1 %, per-tensor
    gradient cosine median >= 0.9 and min >= 0.5 (an f32 evaluation at parameters perturbed by
    1e-3 relative scores 0.98 / 0.89 here). The full-width nets are not compared this way: there
    the f32 gradient itself decorrelates under a 1e-4 relative parameter perturbation (cosine
    0.34, tools/learner_bf16_study.py) — the k-step training loss is chaotic at that scale.
    A cosine is blind to scale and to a few hundredths lost to a wiring error; the per-tensor check of the bf16
    learner is tests/test_gpu_learner_tape.py (its own tape replayed in f64: forward layer by layer, the backward as
    a linear map within twice the replay's rounding spread)."""
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    mcfg = learner_model_cfg()
    ring = _random_ring(256, mcfg["state_history_length"], 5, 11)
    out = {}
    for dt in ("f32", "bf16"):
        ln = Learner(mcfg, init_state_dict(mcfg, 5), K=5, dtype=dt)
        out[dt] = (ln.train_minibatch(ring, ring.slots()).cpu().numpy(), ln.gradients())
        del ln
    assert abs(out["bf16"][0][0] - out["f32"][0][0]) <= 1e-2 * out["f32"][0][0], (out["bf16"][0], out["f32"][0])
    cos = {}
    for k, g in out["f32"][1].items():
        if g.numel() < 1000 or _pre_bn_bias(k):
            continue
        a, b = g.reshape(-1).double(), out["bf16"][1][k].reshape(-1).double()
        cos[k] = float(a @ b / (a.norm() * b.norm() + 1e-30))
    vals = np.array(list(cos.values()))
    print("bf16 gradient cosines: min", vals.min(), "median", np.median(vals))
    assert vals.min() >= 0.5 and np.median(vals) >= 0.9, sorted(cos.items(), key=lambda kv: kv[1])[:5]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(8, 16, 20, 64, 128, 3), (16, 4, 5, 264, 256, 3), (16, 4, 5, 256, 128, 1),
                                   (3, 8, 10, 256, 256, 3), (5, 4, 5, 40, 24, 3)])
def test_conv_wgrad_matches_torch(dt, shape):
    """mzba_conv_wgrad (weight + bias gradient, accumulated into the gradient buffers) against
    torch.nn.grad.conv2d_weight in f64 on the same (bf16-rounded for bf16) operands."""
    from mzba import _lib as L
    B, H, W, Cin, Cout, ks = shape
    if dt == "bf16" and (Cin % 8 or Cout % 8):
        pytest.skip("bf16 path needs Cin, Cout % 8")
    g = torch.Generator().manual_seed(sum(shape))
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    x = torch.randn(B, H, W, Cin, generator=g).to(tdt)
    dy = torch.randn(B, H, W, Cout, generator=g).to(tdt)
    dw0 = torch.randn(Cout, ks * ks, Cin, generator=g)
    db0 = torch.randn(Cout, generator=g)
    dev = torch.device("cuda")
    xd, dyd, dw, db = x.to(dev), dy.to(dev), dw0.clone().to(dev), db0.clone().to(dev)
    nb = L.lib().mzba_conv_wgrad_ws_bytes(B, H, W, Cin, Cout, ks)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    L.call("mzba_conv_wgrad", 0 if dt == "f32" else 1, L.ptr(xd), L.ptr(dyd), B, H, W, Cin, Cout, ks, L.ptr(dw),
           L.ptr(db), L.ptr(ws), nb, L.stream())
    ref = torch.nn.grad.conv2d_weight(x.double().permute(0, 3, 1, 2), (Cout, Cin, ks, ks),
                                      dy.double().permute(0, 3, 1, 2), padding=ks // 2)
    ref = ref.permute(0, 2, 3, 1).reshape(Cout, ks * ks, Cin) + dw0.double()
    refb = dy.double().sum(dim=(0, 1, 2)) + db0.double()
    tol = 1e-5 if dt == "f32" else 2e-3
    scale = ref.abs().max().item()
    assert (dw.cpu().double() - ref).abs().max().item() <= tol * scale
    assert (db.cpu().double() - refb).abs().max().item() <= tol * refb.abs().max().item() + 1e-4


@pytest.mark.parametrize("case", [("lat", 4, 5, 256, 256, 3), ("lat", 4, 5, 256, 128, 1), ("lat", 4, 5, 128, 256, 3),
                                  ("lat", 8, 10, 256, 256, 3), ("band", 16, 20, 128, 256, 3),
                                  ("band", 16, 20, 256, 128, 3)])
@pytest.mark.parametrize("flip", [0, 1])
def test_learner_bf16_conv_packs(case, flip):
    """mzba_conv_pack_bf16 (conv_lat / band layouts, plain and flipped-transposed) driving the
    latent / band conv kernels: forward conv (flip 0) and input-gradient conv (flip 1) of a random
    f32 master weight against torch in f64 on the same bf16-rounded operands."""
    from mzba import _lib as L
    from mzba.learner import LAT_PAD_ELEMS
    kind, H, W, Cin, Cout, ks = case
    B, taps = 3, ks * ks
    g = torch.Generator().manual_seed(Cin + Cout + H + flip)
    w = torch.randn(Cout, taps, Cin, generator=g) * 0.05            # master layout [Cout][tap][Cin]
    N, Cc = (Cin, Cout) if flip else (Cout, Cin)                     # the pack's rows / columns
    if not getattr(L.lib(), f"mzba_conv_{kind}_supported")(H, W, Cc, N, ks):
        pytest.skip("shape not supported by this kernel")
    x = torch.randn(B, H, W, Cc, generator=g).bfloat16()
    dev = torch.device("cuda")
    wd = w.to(dev)
    pack = torch.empty(N * taps * Cc + LAT_PAD_ELEMS, dtype=torch.bfloat16, device=dev)
    L.call("mzba_conv_pack_bf16", L.ptr(wd), L.ptr(pack), Cout, taps, Cin, N, Cc, flip, 1 if kind == "lat" else 2,
           LAT_PAD_ELEMS, L.stream())
    xd = x.to(dev)
    out = torch.empty(B, H, W, N, dtype=torch.bfloat16, device=dev)
    bias = torch.zeros(N, device=dev)
    if kind == "lat":
        L.call("mzba_conv_lat", L.ptr(xd), H * W * Cc, None, 0, L.ptr(pack), L.ptr(bias), None, None, 0, None,
               L.ptr(out), B, H, W, Cc, N, ks, 0, L.stream())
    else:
        L.call("mzba_conv_band", L.ptr(xd), L.ptr(pack), L.ptr(bias), None, L.ptr(out), B, H, W, Cc, N, 0, L.stream())
    wb = w.bfloat16().double().reshape(Cout, ks, ks, Cin).permute(0, 3, 1, 2)   # OIHW
    xin = x.double().permute(0, 3, 1, 2)
    if flip:
        ref = torch.nn.grad.conv2d_input((B, Cin, H, W), wb, xin, padding=ks // 2)
    else:
        ref = torch.nn.functional.conv2d(xin, wb, padding=ks // 2)
    ref = ref.permute(0, 2, 3, 1)
    err = (out.cpu().double() - ref).abs().max().item()
    assert err <= 1e-2 * ref.abs().max().item(), (err, ref.abs().max().item())


@pytest.mark.parametrize("case", [("bf16", 1, 5, 512, 4, 5, 256, 256), ("bf16", 1, 5, 512, 4, 5, 264, 256),
                                  ("bf16", 2, 3, 7, 4, 5, 64, 64),
                                  ("bf16", 1, 3, 7, 4, 5, 64, 64), ("f32", 1, 2, 6, 4, 5, 40, 24),
                                  ("bf16", 2, 8, 16, 8, 10, 128, 128), ("bf16", 2, 3, 24, 3, 7, 64, 72),
                                  ("bf16", 2, 2, 4, 16, 20, 128, 256)])
@pytest.mark.parametrize("form", [2, 3, 1, 0])
def test_conv_wgrad_segs_matches_torch(case, form):
    """mzba_conv_wgrad_segs (the learner's deferred latent weight gradient: K (x, dY) pairs in
    one contraction) against the torch fp32 weight gradient of the concatenated segments.
    variant 1 = automatic (5 x 512 envs at 4x5 -> whole-image kernel, small batches -> one
    per-tap launch pair per segment), 2 = whole-image kernel forced. form 1 = the pixel-row
    whole-image kernel with 32-co wave tiles, 2 = the same with 64-co wave tiles (default), 0 = the
    zero-bordered one (the 3x7 case: HW = 21, odd rows per
    stage; the bordered form refuses it and the per-tap kernel runs)."""
    from mzba import _lib as L
    dt, var, nseg, B, H, W, Cin, Cout = case
    L.call("mzba_conv_wgrad_set_form", form)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(nseg * 1000 + B)
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    xs = [torch.randn(B, H, W, Cin, generator=g, device=dev).to(tdt) for _ in range(nseg)]
    dys = [torch.randn(B, H, W, Cout, generator=g, device=dev).to(tdt) for _ in range(nseg)]
    dw0 = torch.randn(Cout, 9, Cin, generator=g, device=dev)
    db0 = torch.randn(Cout, generator=g, device=dev)
    dw, db = dw0.clone(), db0.clone()
    nb = L.lib().mzba_conv_wgrad_ws_bytes(nseg * B, H, W, Cin, Cout, 3)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    xp = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in xs])
    dp = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in dys])
    L.call("mzba_conv_wgrad_set_variant", var)
    try:
        L.call("mzba_conv_wgrad_segs", 0 if dt == "f32" else 1, xp, dp, nseg, B, H, W, Cin, Cout, 3, L.ptr(dw),
               L.ptr(db), L.ptr(ws), nb, L.stream())
    finally:
        L.call("mzba_conv_wgrad_set_variant", 1)
        L.call("mzba_conv_wgrad_set_form", 2)
    x = torch.cat(xs).float().permute(0, 3, 1, 2)
    dy = torch.cat(dys).float().permute(0, 3, 1, 2)
    ref = torch.nn.grad.conv2d_weight(x, (Cout, Cin, 3, 3), dy, padding=1)
    ref = ref.permute(0, 2, 3, 1).reshape(Cout, 9, Cin) + dw0
    refb = dy.sum(dim=(0, 2, 3)) + db0
    tol = 1e-4 if dt == "f32" else 2e-3
    assert (dw - ref).abs().max().item() <= tol * ref.abs().max().item()
    assert (db - refb).abs().max().item() <= tol * refb.abs().max().item() + 1e-3


@pytest.mark.parametrize("case", [(5, 512, 4, 5, 256, 256), (5, 512, 4, 5, 264, 256), (5, 512, 4, 5, 256, 128),
                                  (1, 512, 8, 10, 256, 256), (1, 512, 16, 20, 128, 128), (2, 24, 3, 7, 64, 72)])
def test_conv_wgrad_px_wave_tile_forms_bit_identical(case):
    """The pixel-row weight gradient's two wave decompositions (form 1: 32 co x 32 ci x 5 / 4 taps per wave;
    form 2: 64 co x 32 ci x 3 / 2 taps per wave; form 3: form 2 with its k steps software-pipelined) give the
    same bits: every output element is the same chain of
    the same MFMAs over the same fragments (the learner's shapes, the representation's, a ragged one)."""
    from mzba import _lib as L
    nseg, B, H, W, Cin, Cout = case
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(7 * nseg + B)
    xs = [torch.randn(B, H, W, Cin, generator=g, device=dev).to(torch.bfloat16) for _ in range(nseg)]
    dys = [torch.randn(B, H, W, Cout, generator=g, device=dev).to(torch.bfloat16) for _ in range(nseg)]
    dw0 = torch.randn(Cout, 9, Cin, generator=g, device=dev)
    db0 = torch.randn(Cout, generator=g, device=dev)
    nb = L.lib().mzba_conv_wgrad_ws_bytes(nseg * B, H, W, Cin, Cout, 3)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    xp = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in xs])
    dp = (ctypes.c_void_p * nseg)(*[t.data_ptr() for t in dys])
    outs = []
    L.call("mzba_conv_wgrad_set_variant", 2)
    try:
        for form in (1, 2, 3):
            L.call("mzba_conv_wgrad_set_form", form)
            dw, db = dw0.clone(), db0.clone()
            L.call("mzba_conv_wgrad_segs", 1, xp, dp, nseg, B, H, W, Cin, Cout, 3, L.ptr(dw), L.ptr(db), L.ptr(ws),
                   nb, L.stream())
            torch.cuda.synchronize()
            outs.append((dw, db))
    finally:
        L.call("mzba_conv_wgrad_set_variant", 1)
        L.call("mzba_conv_wgrad_set_form", 2)
    for dw, db in outs[1:]:
        assert torch.equal(outs[0][0], dw)
        assert torch.equal(outs[0][1], db)
    assert not torch.equal(outs[0][0], dw0)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_learner_deferred_wgrad(dt):
    """Deferring the latent weight gradients to one segmented contraction after the unrolled
    backward: f32 (per-segment launches in backward order) is bit-identical to the immediate
    calls; bf16 with the whole-image kernel forced differs only in f32 summation order."""
    from mzba import _lib as L
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    mcfg = learner_model_cfg()
    ring = _random_ring(64, mcfg["state_history_length"], 5, 3)
    out = {}
    L.call("mzba_conv_wgrad_set_variant", 2 if dt == "bf16" else 1)
    try:
        for defer in (False, True):
            ln = Learner(mcfg, init_state_dict(mcfg, 8), K=5, dtype=dt, defer_wgrad=defer)
            out[defer] = (ln.train_minibatch(ring, ring.slots()).cpu().numpy(), ln.gradients())
            del ln
    finally:
        L.call("mzba_conv_wgrad_set_variant", 1)
    np.testing.assert_array_equal(out[True][0], out[False][0])
    for k, g0 in out[False][1].items():
        g1 = out[True][1][k]
        if dt == "f32":
            assert torch.equal(g0, g1), k
        else:
            assert (g1 - g0).abs().max().item() <= 1e-4 * g0.abs().max().item() + 1e-7, k


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_learner_graph_replay_matches_eager(dt):
    """Learner.capture: a minibatch replayed as one HIP graph (static slot buffer, Adam scalars
    from device memory) is launch-for-launch the eager minibatch: losses, parameters, Adam
    moments and BN running statistics bit-identical over 3 replays."""
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    mcfg = learner_model_cfg()
    ring = _random_ring(64, mcfg["state_history_length"], 5, 9)
    gen = torch.Generator().manual_seed(5)
    slots = [torch.randperm(64, generator=gen)[:32].to(torch.int32) for _ in range(4)]
    a = Learner(mcfg, init_state_dict(mcfg, 3), K=5, dtype=dt)
    b = Learner(mcfg, init_state_dict(mcfg, 3), K=5, dtype=dt)
    la = [a.train_minibatch(ring, s).cpu().clone() for s in slots]
    lb = [b.train_minibatch(ring, slots[0]).cpu().clone()]
    b.capture(ring, 32)
    lb += [b.train_minibatch(ring, s).cpu().clone() for s in slots[1:]]
    for x, y in zip(la, lb):
        assert torch.equal(x, y), (x, y)
    sa, sb = a.state_dict(), b.state_dict()
    for k in sa:
        assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])), k
    assert torch.equal(a.M1, b.M1) and torch.equal(a.M2, b.M2)
    assert a.step_count == b.step_count == 4


@pytest.mark.parametrize("dt,ch", [("f32", 32), ("bf16", 32), ("bf16", 128)])
def test_learner_side_stream_matches_one_stream(dt, ch):
    """streams=2 (prediction nets on a side stream beside the dynamics chain, forward and backward)
    issues the same launches in the same per-stream order as streams=1: losses, parameters, Adam
    moments and BN running statistics bit-identical over 3 minibatches, eager and graph-replayed.
    ch = 128 runs the fused conv_lat + BN path (deferred BN applies crossing the side stream)."""
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    mcfg = learner_model_cfg()
    mcfg["latent_channels"] = [ch, ch]
    ring = _random_ring(64, mcfg["state_history_length"], 5, 13)
    gen = torch.Generator().manual_seed(7)
    slots = [torch.randperm(64, generator=gen)[:32].to(torch.int32) for _ in range(4)]
    a = Learner(mcfg, init_state_dict(mcfg, 6), K=5, dtype=dt, streams=1, lat_rows=3)  # same conv tiles as b, c
    b = Learner(mcfg, init_state_dict(mcfg, 6), K=5, dtype=dt, streams=2)
    c = Learner(mcfg, init_state_dict(mcfg, 6), K=5, dtype=dt, streams=2)
    la = [a.train_minibatch(ring, s).cpu().clone() for s in slots]
    lb = [b.train_minibatch(ring, s).cpu().clone() for s in slots]
    lc = [c.train_minibatch(ring, slots[0]).cpu().clone()]
    c.capture(ring, 32)
    lc += [c.train_minibatch(ring, s).cpu().clone() for s in slots[1:]]
    for x, y, z in zip(la, lb, lc):
        assert torch.equal(x, y) and torch.equal(x, z), (x, y, z)
    sa, sb, sc = a.state_dict(), b.state_dict(), c.state_dict()
    for k in sa:
        assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sb[k])), k
        assert torch.equal(torch.as_tensor(sa[k]), torch.as_tensor(sc[k])), k
    assert torch.equal(a.M1, b.M1) and torch.equal(a.M2, b.M2)
    assert torch.equal(a.M1, c.M1) and torch.equal(a.M2, c.M2)


@pytest.mark.parametrize("variant", [0, 2, 3])
@pytest.mark.parametrize("B,H,W,Cin,Cout,ks", [(512, 4, 5, 256, 256, 3), (37, 4, 5, 256, 128, 3),
                                                (19, 4, 5, 128, 256, 1), (64, 8, 10, 256, 256, 3)])
def test_conv_lat_bn_matches_separate_passes(B, H, W, Cin, Cout, ks, variant):
    """mzba_conv_lat_bn (the BatchNorm statistics in the conv epilogue) against the conv followed by
    the separate BN passes: mode 1 -> mzba_bn_stats_final equals mzba_bn_stats (same bf16 values,
    different chunking: f32 rounding only); mode 2 -> the masked output equals bn_backward's in-place
    mask bit for bit, dgamma / dbeta / dx within f32 rounding. variant 0 = auto tiles (3-row at
    B = 512), 2 = 5-row tiles only (the two-stream learner's)."""
    from mzba import _lib as L
    L.call("mzba_conv_lat_set_variant", variant)
    try:
        _conv_lat_bn_case(B, H, W, Cin, Cout, ks)
    finally:
        L.call("mzba_conv_lat_set_variant", 0)


@pytest.mark.parametrize("B,Cin,Cout,ks", [(512, 256, 256, 3), (37, 256, 128, 3), (19, 128, 256, 1), (1, 256, 256, 3)])
def test_conv_lat_two_per_cu_instance_is_bit_identical(B, Cin, Cout, ks):
    """conv_lat variant 3 (3-row tiles on the two-workgroups-per-CU instance: ring depth 4, <= 128 VGPRs) gives the
    3-row one-per-CU instance's outputs bit for bit (the same per-element arithmetic), every BN mode included:
    plain, statistics (mode 1) with the producing BN applied in the staging, and masked gradient (mode 2)."""
    from mzba import _lib as L
    from mzba.agent import pack_lat
    dev = torch.device("cuda")
    H, W = 4, 5
    g = torch.Generator().manual_seed(11 * B + Cout)
    x = torch.randn(B * H * W, Cin, generator=g).to(torch.bfloat16).to(dev)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
    wf = torch.from_numpy(pack_lat(w.permute(0, 2, 3, 1).reshape(Cout, -1).numpy(), Cout, ks, Cin)).to(
        torch.bfloat16).to(dev)
    bias = torch.randn(Cout, generator=g).to(dev) * 0.1
    res = torch.randn(B * H * W, Cout, generator=g).to(torch.bfloat16).to(dev)
    st = torch.randn(4, Cin, generator=g).to(dev)
    pres = torch.randn(B * H * W, Cin, generator=g).to(torch.bfloat16).to(dev)
    by = torch.relu(torch.randn(B * H * W, Cout, generator=g)).to(torch.bfloat16).to(dev)
    bx = torch.randn(B * H * W, Cout, generator=g).to(torch.bfloat16).to(dev)
    smean = torch.randn(Cout, generator=g).to(dev)

    def run(variant):
        L.call("mzba_conv_lat_set_variant", variant)
        try:
            outs = []
            o = torch.empty(B * H * W, Cout, dtype=torch.bfloat16, device=dev)
            L.call("mzba_conv_lat", L.ptr(x), H * W * Cin, None, 0, L.ptr(wf), L.ptr(bias), None, None, 0, L.ptr(res),
                   L.ptr(o), B, H, W, Cin, Cout, ks, 1, L.stream())
            outs.append(o)
            if Cout % 128 == 0:
                nc, rpc = ctypes.c_int(), ctypes.c_int()
                L.call("mzba_conv_lat_bn_chunks", B, H, W, Cin, Cout, ks, ctypes.byref(nc), ctypes.byref(rpc))
                for mode in (1, 2):
                    part = torch.zeros(nc.value * Cout * 2, device=dev)
                    o = res.clone()
                    po = torch.empty_like(x)
                    L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(bias), L.ptr(o) if mode == 2 else None,
                           L.ptr(o), B, H, W, Cin, Cout, ks, mode, L.ptr(part), L.ptr(by) if mode == 2 else None,
                           L.ptr(bx) if mode == 2 else None, L.ptr(smean) if mode == 2 else None, L.ptr(st),
                           L.ptr(pres), 1, L.ptr(po), None, L.stream())
                    outs += [o, part, po]
            torch.cuda.synchronize()
            return outs
        finally:
            L.call("mzba_conv_lat_set_variant", 0)
    L.call("mzba_conv_lat_set_variant", 3)
    nc3 = ctypes.c_int(); rpc3 = ctypes.c_int()
    L.call("mzba_conv_lat_bn_chunks", B, H, W, Cin, Cout, ks, ctypes.byref(nc3), ctypes.byref(rpc3))
    L.call("mzba_conv_lat_set_variant", 0)
    assert rpc3.value == (96 // (H * W)) * H * W  # variant 3 always takes the 3-row tiles
    a, b = run(0), run(3)  # these shapes: variant 0 takes 3-row tiles too (B = 1: one 20-row chunk either way)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


def _conv_lat_bn_case(B, H, W, Cin, Cout, ks):
    from mzba import _lib as L
    from mzba.agent import pack_lat
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(B + Cout)
    x = torch.randn(B * H * W, Cin, generator=g).to(torch.bfloat16).to(dev)
    w = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
    wf = torch.from_numpy(pack_lat(w.permute(0, 2, 3, 1).reshape(Cout, -1).numpy(), Cout, ks, Cin)).to(torch.bfloat16).to(dev)
    bias = torch.randn(Cout, generator=g).to(dev) * 0.1
    M = B * H * W
    nc, rpc = ctypes.c_int(), ctypes.c_int()
    L.call("mzba_conv_lat_bn_chunks", B, H, W, Cin, Cout, ks, ctypes.byref(nc), ctypes.byref(rpc))
    part = torch.empty(nc.value * Cout * 2, device=dev)
    t = torch.empty(M, Cout, dtype=torch.bfloat16, device=dev)
    L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(bias), None, L.ptr(t), B, H, W, Cin, Cout, ks, 1,
           L.ptr(part), None, None, None, None, None, 0, None, None, L.stream())
    t_ref = torch.empty_like(t)
    L.call("mzba_conv_lat", L.ptr(x), H * W * Cin, None, 0, L.ptr(wf), L.ptr(bias), None, None, 0, None, L.ptr(t_ref),
           B, H, W, Cin, Cout, ks, 0, L.stream())
    assert torch.equal(t, t_ref)
    gamma, beta = torch.rand(Cout, device=dev) + 0.5, torch.randn(Cout, device=dev)
    st1, st2 = torch.empty(4, Cout, device=dev), torch.empty(4, Cout, device=dev)
    rm1, rv1, rm2, rv2 = torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev), torch.zeros(Cout, device=dev), torch.ones(Cout, device=dev)
    L.call("mzba_bn_stats_final", L.ptr(part), nc.value, rpc.value, M, Cout, 1e-5, 0.1, L.ptr(gamma), L.ptr(beta),
           L.ptr(st1), L.ptr(rm1), L.ptr(rv1), L.stream())
    ws = torch.empty(((M + 63) // 64) * Cout * 8 + 12 * Cout, dtype=torch.uint8, device=dev)
    L.call("mzba_bn_stats", 1, L.ptr(t), M, Cout, 1e-5, 0.1, L.ptr(gamma), L.ptr(beta), L.ptr(st2), L.ptr(rm2),
           L.ptr(rv2), L.ptr(ws), ws.numel(), L.stream())
    torch.testing.assert_close(st1, st2, rtol=2e-6, atol=2e-6)
    torch.testing.assert_close(rv1, rv2, rtol=2e-6, atol=2e-6)
    # mode 2: this conv produces the output gradient of a BN (input bx, output by, stats st2)
    by = torch.relu(torch.randn(M, Cout, generator=g)).to(torch.bfloat16).to(dev)
    bx = torch.randn(M, Cout, generator=g).to(torch.bfloat16).to(dev)
    acc = torch.randn(M, Cout, generator=g).to(torch.bfloat16).to(dev)
    g1, g2 = acc.clone(), acc.clone()
    L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(bias), L.ptr(g1), L.ptr(g1), B, H, W, Cin, Cout, ks, 2,
           L.ptr(part), L.ptr(by), L.ptr(bx), L.ptr(st2), None, None, 0, None, None, L.stream())
    L.call("mzba_conv_lat", L.ptr(x), H * W * Cin, None, 0, L.ptr(wf), L.ptr(bias), None, None, 0, L.ptr(g2), L.ptr(g2),
           B, H, W, Cin, Cout, ks, 0, L.stream())
    dg1, db1, dg2, db2 = (torch.zeros(Cout, device=dev) for _ in range(4))
    dx1, dx2 = torch.empty_like(bx), torch.empty_like(bx)
    L.call("mzba_bn_backward_final", 1, L.ptr(g1), L.ptr(bx), L.ptr(st2), L.ptr(part), nc.value, M, Cout, L.ptr(dg1),
           L.ptr(db1), L.ptr(dx1), L.ptr(ws), ws.numel(), L.stream())
    L.call("mzba_bn_backward", 1, L.ptr(g2), L.ptr(by), L.ptr(bx), L.ptr(st2), M, Cout, L.ptr(dg2), L.ptr(db2),
           L.ptr(dx2), L.ptr(ws), ws.numel(), L.stream())
    assert torch.equal(g1, g2)  # the masked gradient
    # producing-BN apply in the staging: x itself is a BN input with stats st2 (Cin == Cout cases),
    # y = relu(x * alpha + beta' + res) both stored (pout) and convolved; vs mzba_bn_apply + conv_lat
    if Cin == Cout:
        resx = torch.randn(M, Cin, generator=g).to(torch.bfloat16).to(dev)
        y_p, y_a = torch.empty_like(x), torch.empty_like(x)
        t_p, t_a = torch.empty_like(t), torch.empty_like(t)
        L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(bias), None, L.ptr(t_p), B, H, W, Cin, Cout, ks, 1,
               L.ptr(part), None, None, None, L.ptr(st2), L.ptr(resx), 1, L.ptr(y_p), None, L.stream())
        L.call("mzba_bn_apply", 1, L.ptr(x), L.ptr(st2), L.ptr(resx), 1, L.ptr(y_a), M, Cin, L.stream())
        L.call("mzba_conv_lat", L.ptr(y_a), H * W * Cin, None, 0, L.ptr(wf), L.ptr(bias), None, None, 0, None,
               L.ptr(t_a), B, H, W, Cin, Cout, ks, 0, L.stream())
        assert torch.equal(y_p, y_a) and torch.equal(t_p, t_a)
        # backward: x is a BN output gradient g (BN input bx, stats st2); the staged input is
        # dt = ((g - (bx - mean) k) - mean_g) alpha with coef from mzba_bn_backward_coef
        coef = torch.empty(3 * Cin, device=dev)
        dgc, dbc = torch.zeros(Cin, device=dev), torch.zeros(Cin, device=dev)
        L.call("mzba_bn_backward_coef", L.ptr(part), nc.value, M, Cin, L.ptr(st2), L.ptr(dgc), L.ptr(dbc), L.ptr(coef),
               L.stream())
        d_p, d_a = torch.empty_like(x), torch.empty_like(x)
        o_p, o_a = torch.empty_like(t), torch.empty_like(t)
        L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(bias), None, L.ptr(o_p), B, H, W, Cin, Cout, ks, 0,
               None, None, None, None, L.ptr(st2), L.ptr(bx), 0, L.ptr(d_p), L.ptr(coef), L.stream())
        L.call("mzba_bn_backward_apply", 1, L.ptr(x), L.ptr(bx), L.ptr(st2), L.ptr(coef), L.ptr(d_a), M, Cin,
               L.stream())
        L.call("mzba_conv_lat", L.ptr(d_a), H * W * Cin, None, 0, L.ptr(wf), L.ptr(bias), None, None, 0, None,
               L.ptr(o_a), B, H, W, Cin, Cout, ks, 0, L.stream())
        assert torch.equal(d_p, d_a) and torch.equal(o_p, o_a)
    torch.testing.assert_close(dg1, dg2, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(db1, db2, rtol=1e-4, atol=1e-3)
    assert (dx1.float() - dx2.float()).abs().max().item() <= 1e-2 * dx2.float().abs().max().item()


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("B,H,W,Cin,Cout,ks", [(512, 4, 5, 256, 256, 3), (37, 4, 5, 256, 128, 3),
                                                (19, 4, 5, 128, 256, 1), (64, 8, 10, 256, 256, 3), (1, 4, 5, 256, 256, 3)])
def test_conv_lat_bn_fin_matches_separate_finalisers(B, H, W, Cin, Cout, ks, variant):
    """mzba_conv_lat_bn_fin (the consuming BN's finaliser folded into the producing launch by its last workgroup per
    column block, sc1 hand-off) against mzba_conv_lat_bn followed by the separate finaliser launches on the SAME
    partials: outputs and partials bit for bit; mode 1 stats and running statistics, mode 2 coef / dgamma / dbeta
    within f32 rounding of the other fold order (rtol 2e-6: both fold in double); the counter words are zero again
    after every launch, and a second launch on the same words gives the same bits (the reset works). variant 0 at
    B = 512 = 3-row tiles, 128 chunks per column block (the finaliser's register cache holds 64: the reload path)."""
    from mzba import _lib as L
    from mzba.agent import pack_lat
    L.call("mzba_conv_lat_set_variant", variant)
    try:
        dev = torch.device("cuda")
        g = torch.Generator().manual_seed(3 * B + Cout)
        x = torch.randn(B * H * W, Cin, generator=g).to(torch.bfloat16).to(dev)
        w = torch.randn(Cout, Cin, ks, ks, generator=g) / (Cin * ks * ks) ** 0.5
        wf = torch.from_numpy(pack_lat(w.permute(0, 2, 3, 1).reshape(Cout, -1).numpy(), Cout, ks, Cin)).to(
            torch.bfloat16).to(dev)
        bias = torch.randn(Cout, generator=g).to(dev) * 0.1
        M = B * H * W
        nc, rpc = ctypes.c_int(), ctypes.c_int()
        L.call("mzba_conv_lat_bn_chunks", B, H, W, Cin, Cout, ks, ctypes.byref(nc), ctypes.byref(rpc))
        ctr = torch.zeros(Cout // 128 + 3, dtype=torch.int32, device=dev)
        gamma, beta = torch.rand(Cout, device=dev) + 0.5, torch.randn(Cout, device=dev)
        # mode 1
        pa, pb = torch.empty(nc.value * Cout * 2, device=dev), torch.empty(nc.value * Cout * 2, device=dev)
        ta, tb = (torch.empty(M, Cout, dtype=torch.bfloat16, device=dev) for _ in range(2))
        L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(bias), None, L.ptr(ta), B, H, W, Cin, Cout, ks, 1,
               L.ptr(pa), None, None, None, None, None, 0, None, None, L.stream())
        sa = torch.empty(4, Cout, device=dev)
        rma, rva = torch.randn(Cout, device=dev), torch.rand(Cout, device=dev) + 0.5
        rmb, rvb = rma.clone(), rva.clone()
        L.call("mzba_bn_stats_final", L.ptr(pa), nc.value, rpc.value, M, Cout, 1e-5, 0.1, L.ptr(gamma), L.ptr(beta),
               L.ptr(sa), L.ptr(rma), L.ptr(rva), L.stream())
        sbs = []
        for rep in range(2):
            sb = torch.empty(4, Cout, device=dev)
            L.call("mzba_conv_lat_bn_fin", L.ptr(x), L.ptr(wf), L.ptr(bias), None, L.ptr(tb), B, H, W, Cin, Cout, ks,
                   1, L.ptr(pb), None, None, None, None, None, 0, None, None, L.ptr(ctr), 1e-5, 0.1, L.ptr(gamma),
                   L.ptr(beta), L.ptr(sb), L.ptr(rmb) if rep == 0 else None, L.ptr(rvb) if rep == 0 else None, None,
                   None, None, L.stream())
            torch.cuda.synchronize()
            assert int(ctr.abs().sum()) == 0
            sbs.append(sb)
        assert torch.equal(ta, tb) and torch.equal(pa, pb)
        assert torch.equal(sbs[0], sbs[1])
        torch.testing.assert_close(sbs[0], sa, rtol=2e-6, atol=1e-7)
        torch.testing.assert_close(rmb, rma, rtol=2e-6, atol=1e-7)
        torch.testing.assert_close(rvb, rva, rtol=2e-6, atol=1e-7)
        # mode 2: the conv output is a BN output gradient (BN input bx, output by, stats sa)
        by = torch.relu(torch.randn(M, Cout, generator=g)).to(torch.bfloat16).to(dev)
        bx = torch.randn(M, Cout, generator=g).to(torch.bfloat16).to(dev)
        acc = torch.randn(M, Cout, generator=g).to(torch.bfloat16).to(dev)
        ga, gb = acc.clone(), acc.clone()
        L.call("mzba_conv_lat_bn", L.ptr(x), L.ptr(wf), L.ptr(bias), L.ptr(ga), L.ptr(ga), B, H, W, Cin, Cout, ks, 2,
               L.ptr(pa), L.ptr(by), L.ptr(bx), L.ptr(sa), None, None, 0, None, None, L.stream())
        dga, dba = torch.randn(Cout, device=dev), torch.randn(Cout, device=dev)
        dgb, dbb = dga.clone(), dba.clone()
        ca, cb = torch.empty(3 * Cout, device=dev), torch.empty(3 * Cout, device=dev)
        L.call("mzba_bn_backward_coef", L.ptr(pa), nc.value, M, Cout, L.ptr(sa), L.ptr(dga), L.ptr(dba), L.ptr(ca),
               L.stream())
        L.call("mzba_conv_lat_bn_fin", L.ptr(x), L.ptr(wf), L.ptr(bias), L.ptr(gb), L.ptr(gb), B, H, W, Cin, Cout, ks,
               2, L.ptr(pb), L.ptr(by), L.ptr(bx), L.ptr(sa), None, None, 0, None, None, L.ptr(ctr), 1e-5, 0.1, None,
               None, L.ptr(sa), None, None, L.ptr(dgb), L.ptr(dbb), L.ptr(cb), L.stream())
        torch.cuda.synchronize()
        assert int(ctr.abs().sum()) == 0
        assert torch.equal(ga, gb) and torch.equal(pa, pb)
        torch.testing.assert_close(cb, ca, rtol=2e-6, atol=1e-9)
        torch.testing.assert_close(dgb, dga, rtol=2e-6, atol=1e-6)
        torch.testing.assert_close(dbb, dba, rtol=2e-6, atol=1e-6)
    finally:
        L.call("mzba_conv_lat_set_variant", 0)


def test_learner_bn_fin_tracks_separate_finalisers():
    """The bf16 learner with every fused BN finaliser in its producing conv_lat launch (fuse_fin, the default) vs the
    separate finaliser launches: the same algorithm with another double fold order of the chunk statistics, so a
    statistic can move by an f32 last place and the chaotic bf16 k-step loss with it (the fused-statistics test's
    bound: losses within 2e-3 relative over two minibatches); the counter pool is zero after each minibatch, eager and
    graph-replayed, and the replay equals the eager minibatch bit for bit."""
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    mcfg = learner_model_cfg()
    mcfg["latent_channels"] = [128, 128]  # conv_lat widths (the fused path needs Cout % 128 == 0)
    ring = _random_ring(96, mcfg["state_history_length"], 5, 77)
    losses = {}
    for fin in (False, True):
        ln = Learner(mcfg, init_state_dict(mcfg, 9), K=5, dtype="bf16", fuse_fin=fin)
        out = [ln.train_minibatch(ring, ring.slots()).cpu() for _ in range(2)]
        if fin:
            assert ln._ctr is not None and int(ln._ctr.abs().sum()) == 0 and ln._ctr_i > 0
            e = Learner(mcfg, init_state_dict(mcfg, 9), K=5, dtype="bf16", fuse_fin=True)
            r = Learner(mcfg, init_state_dict(mcfg, 9), K=5, dtype="bf16", fuse_fin=True)
            sl = ring.slots()
            le = [e.train_minibatch(ring, sl).cpu() for _ in range(3)]
            r.train_minibatch(ring, sl)
            r.capture(ring, sl.numel())
            lr = [r.train_minibatch(ring, sl).cpu() for _ in range(2)]
            torch.cuda.synchronize()
            assert torch.equal(le[1], lr[0]) and torch.equal(le[2], lr[1])
            assert int(r._ctr.abs().sum()) == 0
        losses[fin] = out
    for a, b in zip(losses[True], losses[False]):
        torch.testing.assert_close(a, b, rtol=2e-3, atol=1e-5)


@pytest.mark.parametrize("fuse_fin", [False, True])
def test_learner_masked_gradient_reaches_only_its_own_bn(fuse_fin):
    """A gradient that a conv_lat launch masked for BatchNorm A (with A's partial sums, and with fuse_fin already
    A's dgamma / dbeta) says so: the backward of another BatchNorm B of the same width refuses it (RuntimeError,
    B's dgamma / dbeta untouched: mzba_bn_backward over it would count sums a second time), and A's own backward
    takes the partials path and adds to A's dgamma / dbeta once: equal to mzba_bn_backward on copies of the same
    inputs within that pair's f32 rounding (_conv_lat_bn_case's tolerances; observed |dgamma| 17.2, difference
    1.9e-6). latent_channels 128, 8 windows: the smallest conv_lat launch with partials."""
    from mzba import _lib as L
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner, _Val
    from mzba.weights import init_state_dict
    mcfg = learner_model_cfg()
    mcfg["latent_channels"] = [128, 128]
    B, (H, W) = 8, mcfg["latent_resolution"]
    ring = _random_ring(B, mcfg["state_history_length"], 1, 31)
    ln = Learner(mcfg, init_state_dict(mcfg, 2), K=1, dtype="bf16", fuse_bn=True, streams=1, fuse_fin=fuse_fin)
    ln.train_minibatch(ring, ring.slots())  # weight packs, scratch
    ln.G.zero_()
    dev, M, C = ln.device, B * H * W, 128
    g = torch.Generator().manual_seed(17)
    c1, c2 = r = ln.dyn_res[0]  # BN A = c1's (output a1), BN B = c2's (output out)
    _, (x, t1, a1, s1, t2, s2, out) = ln._res_fwd(r, _Val(torch.randn(M, C, generator=g).to(torch.bfloat16).to(dev)),
                                                  B, H, W)
    ln._settle()
    dy = _Val(torch.randn(M, C, generator=g).to(torch.bfloat16).to(dev))
    da1 = ln._dgrad(c2, dy, B, H, W, bn=(c1, a1, t1, s1))
    assert da1.masked is not None  # the launch carried A's partials
    with pytest.raises(RuntimeError):
        ln._bn_bwd(c2, da1, out, t2, s2)
    torch.cuda.synchronize()
    assert int((c2.dgamma != 0).sum()) == 0 and int((c2.dbeta != 0).sum()) == 0
    g_ref, dx_ref = da1.t.clone(), torch.empty_like(t1)
    dg_ref, db_ref = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    ws = torch.empty(((M + 63) // 64) * C * 8 + 12 * C, dtype=torch.uint8, device=dev)
    L.call("mzba_bn_backward", 1, L.ptr(g_ref), L.ptr(a1.t), L.ptr(t1), L.ptr(s1), M, C, L.ptr(dg_ref), L.ptr(db_ref),
           L.ptr(dx_ref), L.ptr(ws), ws.numel(), L.stream())
    dt1 = ln._bn_bwd(c1, da1, a1, t1, s1)
    assert dt1.owed is not None and da1.masked is None  # the partials path: the apply is left to the consumer
    dx = dt1.ready()
    torch.cuda.synchronize()
    assert torch.equal(g_ref, da1.t)  # it was already A's masked gradient
    print("dgamma", c1.dgamma.abs().max().item(), (c1.dgamma - dg_ref).abs().max().item(),
          "dbeta", c1.dbeta.abs().max().item(), (c1.dbeta - db_ref).abs().max().item())
    assert dg_ref.abs().max().item() > 0.1  # once and twice are far apart at this tolerance
    torch.testing.assert_close(c1.dgamma, dg_ref, rtol=1e-4, atol=1e-3)
    torch.testing.assert_close(c1.dbeta, db_ref, rtol=1e-4, atol=1e-3)
    assert (dx.float() - dx_ref.float()).abs().max().item() <= 1e-2 * dx_ref.float().abs().max().item()
    assert int((c2.dgamma != 0).sum()) == 0 and int((c2.dbeta != 0).sum()) == 0


def test_learner_fused_bn_statistics_track_separate_passes():
    """bf16 learner with the BN statistics in the conv epilogues vs the separate BN passes. The per-kernel
    arithmetic is checked deterministically by test_conv_lat_bn_matches_separate_passes (partial
    statistics, masks, applies); end to end the two are the same algorithm with different f32 summation
    chunks, so some bf16 activations round the other way, and the k-step loss is chaotic: two such
    bf16 realisations are NOT close to each other per tensor (calibrated over 6 seeds on two band-kernel
    builds, tools/learner_bn_calib.py, profiles/r03/learner_calib/: min gradient cosine fused~sep 0.86 -
    0.9998, median >= 0.94). What a wiring error (wrong consumer BN, mask or chunk) would break is how
    close each realisation is to the f32 parity path, so per seed (4 seeds) the fused run must be as
    close to f32 as the separate-pass run: median cosine within 0.02 (observed |diff| <= 0.019) and min
    within 0.1 (observed >= -0.049); losses within 2e-3 relative (observed <= 1.5e-3).
    The wiring itself (consumer BN, mask, acc, segments) is checked per tensor, at the few-percent level, by
    tests/test_gpu_learner_tape.py on the fused learner's own tape."""
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    mcfg = learner_model_cfg()
    mcfg["latent_channels"] = [128, 128]
    for seed in range(4):
        ring = _random_ring(64, mcfg["state_history_length"], 5, 21 + seed)
        out = {}
        for tag, dt, fuse in (("sep", "bf16", False), ("fused", "bf16", True), ("f32", "f32", False)):
            ln = Learner(mcfg, init_state_dict(mcfg, 4 + seed), K=5, dtype=dt, fuse_bn=fuse, lat_rows="auto")
            out[tag] = (ln.train_minibatch(ring, ring.slots()).cpu(), ln.gradients())
            del ln
        torch.testing.assert_close(out["fused"][0], out["sep"][0], rtol=2e-3, atol=1e-5)

        def cosines(a, b):
            c = {}
            for k, g0 in out[b][1].items():
                if _pre_bn_bias(k) or g0.abs().max() == 0:
                    continue
                c[k] = torch.nn.functional.cosine_similarity(g0.flatten().double(), out[a][1][k].flatten().double(),
                                                             dim=0).item()
            return np.array(list(c.values()))
        fs, ff, sf = cosines("fused", "sep"), cosines("fused", "f32"), cosines("sep", "f32")
        print(f"seed {seed}: fused~sep {np.median(fs):.4f} / {fs.min():.4f}, fused~f32 {np.median(ff):.4f} / "
              f"{ff.min():.4f}, sep~f32 {np.median(sf):.4f} / {sf.min():.4f}")
        assert np.median(fs) >= 0.9, (seed, np.median(fs))
        assert np.median(ff) >= np.median(sf) - 0.02 and ff.min() >= sf.min() - 0.1, (seed, ff, sf)
        # per tensor where a wiring error shows and the chaos does not: the three Linear heads' weight
        # gradients (activation x logit gradient of the last layer, each a single consumer)
        heads = [k for k in out["sep"][1] if k.endswith(("reward_head.2.weight", "policy_head.2.weight",
                                                          "value_head.2.weight"))]
        assert len(heads) == 3
        for k in heads:
            a, b = out["fused"][1][k].flatten().double(), out["sep"][1][k].flatten().double()
            cs = torch.nn.functional.cosine_similarity(a, b, dim=0).item()
            print(f"seed {seed}: {k} fused~sep cosine {cs:.5f}")
            assert cs >= 0.95, (seed, k, cs)


@pytest.mark.parametrize("B,K,ns,na,with_slots", [(512, 5, 11, 3, True), (37, 3, 16, 4, False), (1, 1, 2, 1, True)])
def test_loss_ws_equals_one_workgroup_loss(B, K, ns, na, with_slots):
    """mzba_learner_loss_ws (a thread per (window, step) row, then one workgroup folding the rows in the one-workgroup
    kernel's order) gives mzba_learner_loss's loss and logit gradients bit for bit, at the learner's shape and at
    ragged row counts (B K not a multiple of 256, one row)."""
    from mzba import _lib as L
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(B * 7 + K)
    cap = B + 5
    lr = torch.randn(K, B, ns, generator=g, device=dev) * 3
    lv = torch.randn(K, B, ns, generator=g, device=dev) * 3
    lp = torch.randn(K, B, na, generator=g, device=dev)
    rewards = torch.randint(-1, 2, (cap, K), generator=g, device=dev).float()
    targets = torch.randn(cap, K, generator=g, device=dev) * 4
    counts = torch.randint(0, 51, (cap, K, na), generator=g, device=dev).float() + 1
    slots = torch.randperm(cap, generator=g, device=dev)[:B].to(torch.int32) if with_slots else None
    outs = []
    for use_ws in (False, True):
        d = [torch.full_like(t, float("nan")) for t in (lr, lv, lp)]
        loss = torch.full((4,), float("nan"), device=dev)
        args = [L.ptr(lr), L.ptr(lv), L.ptr(lp), L.ptr(rewards), L.ptr(targets), L.ptr(counts), L.ptr(slots), B, K, ns, na,
                -5.0, 5.0, L.ptr(d[0]), L.ptr(d[1]), L.ptr(d[2]), L.ptr(loss)]
        if use_ws:
            ws = torch.empty(int(L.lib().mzba_learner_loss_ws_bytes(B, K)), dtype=torch.uint8, device=dev)
            L.call("mzba_learner_loss_ws", *args, L.ptr(ws), ws.numel(), L.stream())
        else:
            L.call("mzba_learner_loss", *args, L.stream())
        outs.append([loss] + d)
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0][0]).all()
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    ws = torch.empty(8, dtype=torch.uint8, device=dev)
    assert L.lib().mzba_learner_loss_ws(L.ptr(lr), L.ptr(lv), L.ptr(lp), L.ptr(rewards), L.ptr(targets), L.ptr(counts),
                                        None, B, K, ns, na, ctypes.c_float(-5.0), ctypes.c_float(5.0), L.ptr(lr),
                                        L.ptr(lv), L.ptr(lp), L.ptr(lr), L.ptr(ws), 8, L.stream()) == -2
