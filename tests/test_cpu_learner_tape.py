"""tests/learner_tape.py checked on the CPU: the replay is the backward (E equals torch.autograd of LearnerOracle on a
CPU tape), and the assertion the GPU test applies has power (wiring mutants of the backward are rejected, the
unmutated rounded replay is accepted)."""
import copy
import os

import numpy as np
import pytest
import torch

import learner_tape as LT

torch.set_num_threads(min(16, os.cpu_count() or 1))


def _cfg(ch):
    from mzba.config import learner_model_cfg
    m = learner_model_cfg()
    m["latent_channels"] = [ch, ch]
    return m


def _setup(ch, B, K, bf16=False):
    from mzba.weights import init_state_dict
    m = _cfg(ch)
    sd = init_state_dict(m, 5)
    mb = LT.random_mb(B, m["state_history_length"], K, 11)
    return m, sd, mb, LT.cpu_tape(m, sd, mb, K, bf16=bf16)


@pytest.mark.parametrize("ch", [32, 128])
@pytest.mark.parametrize("B,K", [(3, 1), (8, 2), (5, 5)])
def test_replay_equals_autograd(ch, B, K):
    """Replay E of an unrounded CPU tape equals loss.backward() of LearnerOracle in f64, the scale positions forced to
    the tape's, to 1e-9 of each tensor's max (pre-BN conv biases: of their weight gradient's max, the gradient is 0)."""
    from oracle.learner import LearnerOracle
    m, sd, mb, T = _setup(ch, B, K)
    o = LearnerOracle(m, sd, K=K, dtype=torch.float64)
    o.force_index = LT.force_index(T)
    _, logits, ref = o.gradients(mb)
    for k, name in enumerate(("lr", "lv", "lp")):  # the tape's forward is the oracle's
        mine = torch.stack([st["dyn" if name == "lr" else "pred"][name] for st in T["steps"]], 1)
        assert (mine - logits[k]).abs().max().item() <= 1e-10
    g, gps, dh = LT.replay(m, T, sd, False)
    assert set(g) == set(ref)
    for k, r in ref.items():
        scale = ref[k[:-len("bias")] + "weight"].abs().max().item() if LT._pre_bn_bias(k) else r.abs().max().item()
        assert scale > 0, k
        assert (g[k] - r).abs().max().item() <= 1e-9 * scale, (k, (g[k] - r).abs().max().item(), scale)


MUTANTS = [("skip", "dyn_net.res_blocks.1", 0), ("skip", "rep_net.blocks.3", None), ("mask", "pred_net.res_blocks.0", 1),
           ("nopred", 1), ("misswg", "dyn_net.res_blocks.0.conv2", 0), ("misswg", "pred_net.value_head.0.conv", 1),
           ("dwx2", "rep_net.blocks.2.weight"), ("dwx2", "dyn_net.conv_block.conv.weight"),
           ("dgamma2", "pred_net.res_blocks.1.bn1", 0)]


@pytest.fixture(scope="module")
def rounded_case():
    """(8, 2) on the 32-channel config, the forward rounded as the bf16 learner rounds it: E, the witnesses, R."""
    m, sd, mb, T = _setup(32, 8, 2, bf16=True)
    E, W, wit32 = LT.witnesses(m, T, sd, True)
    return m, sd, T, E, W, wit32


def test_unmutated_rounded_replay_is_accepted(rounded_case):
    """R itself, and a dithered replay with a seed of its own, against the dither witness alone (R taken out of the
    witness set for R's own check, so it is not accepted by construction)."""
    m, sd, T, E, W, wit32 = rounded_case
    LT.assert_backward(W[0], E, W[1:], wit32, T, True, label="R: ")
    other = LT.flat(LT.replay(m, T, sd, True, q=LT.dither_bf16(77)))
    LT.assert_backward(other, E, W, wit32, T, True, label="D77: ")


@pytest.mark.parametrize("mut", MUTANTS, ids=lambda t: "-".join(str(v) for v in t))
def test_mutant_is_rejected(rounded_case, mut):
    """A wiring defect in the rounded backward (dropped skip path, the other BN's mask, the prediction part of d h_k
    left out, an unrolled step missing from a weight gradient, a weight gradient doubled, a dgamma counted twice)
    fails the assertion at margin 2."""
    m, sd, T, E, W, wit32 = rounded_case
    bad = LT.flat(LT.replay(m, T, sd, True, q=LT.rne_bf16, mut=[mut]))
    with pytest.raises(AssertionError):
        LT.assert_backward(bad, E, W, wit32, T, True, label=f"{mut}: ")


@pytest.mark.parametrize("ch,B,K", [(128, 8, 2), (128, 37, 5), (32, 8, 2)])
def test_witness_spread_of_the_gpu_cases(ch, B, K):
    """The reference's own rounding spread, largest w / |g_E| per tensor, at the GPU cases' shapes (CPU tape, forward
    rounded): a few percent. A spread far above that would mean the tape sits on a kink and the 2 w bound says little;
    10 % is the limit taken here (measured: see DESIGN.md §4)."""
    m, sd, mb, T = _setup(ch, B, K, bf16=True)
    E, W, wit32 = LT.witnesses(m, T, sd, True)
    _, spread = LT.assert_backward(W[0], E, W[1:], wit32, T, True, label=f"ch{ch} B{B} K{K}: ")
    print(f"witness spread ch {ch} B {B} K {K}: {spread:.4f}")
    assert spread <= 0.10


def test_forward_audit_accepts_a_cpu_tape_and_rejects_a_wrong_one():
    """audit_forward on a CPU tape whose forward went through bf16 (stored tensors on the bf16 grid, as the learner's):
    every layer passes; with one residual block's output recomputed without its skip input, and with one BN's alpha row
    scaled by 1 + 2^-6, it fails."""
    m, sd, mb, T = _setup(32, 5, 2, bf16=True)
    lut = np.array([0, 0.3, 0.6, 1.0, 0, 0, 0, 0], np.float32)
    codes = np.searchsorted(lut[:4], np.asarray(mb["states"]).reshape(5, m["state_history_length"], -1))
    ring = dict(states=torch.from_numpy(codes.astype(np.uint8)), past_actions=torch.as_tensor(mb["past_actions"]),
                future_actions=torch.as_tensor(mb["future_actions"]))
    args = (sd, None, ring, torch.arange(5), lut, True, lambda *a: False)
    assert LT.audit_forward(m, T, *args) > 100
    bad = copy.deepcopy(T)
    sv = bad["steps"][1]["dyn"]["res"][0]
    s = sv["s2"]
    y = LT.f_apply(LT._img(sv["t2"], 5), s)  # the skip input left out
    sv["out"] = LT.rne_bf16(LT._rows(y))
    with pytest.raises(AssertionError):
        LT.audit_forward(m, bad, *args)
    bad = copy.deepcopy(T)
    bad["steps"][0]["pred"]["pol"]["s"][2] *= 1 + 2.0 ** -6
    with pytest.raises(AssertionError):
        LT.audit_forward(m, bad, *args)
