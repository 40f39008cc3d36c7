"""The learner's own tape against f64, layer by layer (tests/learner_tape.py states the ops, the bounds and the replay).

Each case runs two minibatches of one learner with `keep_tape` on one ring and audits both: every stored forward
tensor against the f64 op on its stored inputs, then the whole backward, as the linear map of the logit gradients it
is once the forward tape is fixed, against the f64 replay E with the replay's own bf16 rounding spread as the bound
(d <= 2 w per parameter tensor and per checkpoint, 2-norm and max norm; d / w printed per tensor with pytest -s). Step 2
takes its parameters from state_dict() after step 1 (a stale weight pack would show as a conv that used other weights)
and reads the ring through permuted slots.

What the end-to-end tests (test_learner_bf16_tracks_f32, the fused-statistics test) cannot see and this does: a
gradient off by a scale, a dropped skip path, the other BN's mask, a missing prediction part of d h_k, a segment lost
or doubled in the deferred contraction — tests/test_cpu_learner_tape.py shows each rejected at this margin.
"""
import os

import pytest
import torch

import learner_tape as LT

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))


def _cfg(ch):
    from mzba.config import learner_model_cfg
    m = learner_model_cfg()
    if ch is not None:
        m["latent_channels"] = [ch, ch]
    return m


def _audit_two_steps(tag, dtype, ch, B, K, **kw):
    from mzba import _lib as L
    from mzba.env import gray_lut
    from mzba.learner import Learner, MinibatchRing
    from mzba.weights import init_state_dict
    m = _cfg(ch)
    bf16 = dtype == "bf16"
    ring = MinibatchRing(LT.random_mb(B, m["state_history_length"], K, 11))
    host = {k: ring._ring[k].cpu() for k in ("states", "past_actions", "future_actions")}
    ln = Learner(m, init_state_dict(m, 5), K=K, dtype=dtype, **kw)
    ln.keep_tape = True

    def fused(cin, cout, ks, H, W):  # Learner._conv's choice of the statistics' kernel
        return bool(bf16 and L.lib().mzba_conv_lat_supported(H, W, cin, cout, ks)) and ln._fusable("lat", cout)

    worst = 0.0
    for step in (1, 2):
        before = ln.state_dict()
        slots = ring.slots() if step == 1 else ring.slots().flip(0)
        ln.train_minibatch(ring, slots)
        T, after = LT.host_tape(ln), ln.state_dict()
        got = dict(ln.gradients())
        got.update({f"gps[{k}]": t for k, t in enumerate(T["gps"])})
        got.update({f"dh[{k}]": t for k, t in enumerate(T["dh"])})
        n = LT.audit_forward(m, T, before, after, host, slots, gray_lut(), bf16, fused)
        assert n > 60 * K
        E, W, wit32 = LT.witnesses(m, T, before, bf16)
        w, _ = LT.assert_backward(got, E, W, wit32, T, bf16, label=f"{tag} step {step}: ")
        worst = max(worst, w)
    print(f"{tag}: {n} forward tensors per step, largest d / w over both steps {worst:.3f}")


@pytest.mark.parametrize("B,K", [(8, 2), (37, 5)])
def test_tape_bf16_defaults_fused_latents(B, K):
    """(a) bf16, every default (fused BN statistics in conv_lat, deferred latent weight gradients, two streams) at 128
    latent channels, where the fused conv_lat path is live; (37, 5): 740 rows, no multiple of 64, five segments."""
    _audit_two_steps(f"a B{B} K{K}", "bf16", 128, B, K)


def test_tape_bf16_whole_image_wgrad():
    """(b) as (a) at (37, 5) with mzba_conv_wgrad_set_variant(2): the whole-image weight-gradient kernel takes the
    deferred 4 x 5 contraction at this size."""
    from mzba import _lib as L
    L.call("mzba_conv_wgrad_set_variant", 2)
    try:
        _audit_two_steps("b B37 K5", "bf16", 128, 37, 5)
    finally:
        L.call("mzba_conv_wgrad_set_variant", 1)


def test_tape_bf16_separate_passes_one_stream():
    """(c) bf16 with the separate BN passes, immediate weight gradients and one stream."""
    _audit_two_steps("c B8 K2", "bf16", 128, 8, 2, fuse_bn=False, defer_wgrad=False, streams=1)


def test_tape_bf16_narrow_config():
    """(d) bf16 defaults on the unedited learner_model_cfg(): 32 channels, the other _conv_kind choices."""
    _audit_two_steps("d B8 K2", "bf16", None, 8, 2)


def test_tape_f32():
    """(e) the f32 parity path on the unedited config: no stored rounding, every tensor against E with the f32 bound."""
    _audit_two_steps("e B8 K2", "f32", None, 8, 2)


@pytest.mark.parametrize("kw", [dict(), dict(streams=1, fuse_bn=False, defer_wgrad=False)], ids=["defaults", "unfused-1-stream"])
def test_keep_tape_changes_nothing(kw):
    """Loss, gradients, parameters, Adam moments and BN running statistics of two minibatches are bit-identical with
    and without the tape hook (bf16, 128 latent channels: the fused path and the side stream are live with the
    defaults); capture() with the hook set raises."""
    from mzba.learner import Learner, MinibatchRing
    from mzba.weights import init_state_dict
    m = _cfg(128)
    ring = MinibatchRing(LT.random_mb(8, m["state_history_length"], 2, 11))
    out = []
    for keep in (False, True):
        ln = Learner(m, init_state_dict(m, 5), K=2, dtype="bf16", **kw)
        ln.keep_tape = keep
        steps = []
        for _ in range(2):
            loss = ln.train_minibatch(ring, ring.slots()).cpu().clone()
            steps.append((loss, ln.G.cpu().clone()))
            assert (ln.last_tape is not None) == keep
        torch.cuda.synchronize()
        out.append((steps, ln.state_dict(), ln.M1.cpu(), ln.M2.cpu()))
        if keep:
            assert len(ln.last_tape["gps"]) == len(ln.last_tape["dh"]) == 2 and len(ln.last_tape["latents"]) == 3
            with pytest.raises(RuntimeError):
                ln.capture(ring, 8)
    (sa, da, m1a, m2a), (sb, db, m1b, m2b) = out
    for (la, ga), (lb, gb) in zip(sa, sb):
        assert torch.equal(la, lb) and torch.equal(ga, gb)
    for k in da:
        assert torch.equal(torch.as_tensor(da[k]), torch.as_tensor(db[k])), k
    assert torch.equal(m1a, m1b) and torch.equal(m2a, m2b)
