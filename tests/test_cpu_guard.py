"""CPU-only checks of the learner step guard's host side (mzba/guard.py): StepGuard's validation, the pure-Python
restatements of the formulas the device evaluates (csrc/guard.hip) against closed forms and against torch's own
clip_grad_norm_ / Adam, the stats block's layout against the library, and the new entry points' argument checks."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from mzba import guard as G

TS = (1, 2, 10, 1000, 100000)


def test_step_guard_validation():
    g = G.StepGuard()
    assert g.max_norm is None and g.skip_nonfinite is True and g.lr_schedule is None and g.lr_dev is None
    assert G.StepGuard(max_norm=2, lr_schedule=("exp", 0.5, 2)).lr_schedule == ("exp", 0.5, 2)
    assert G.StepGuard(max_norm=math.inf).max_norm == math.inf
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            G.StepGuard(max_norm=bad)
    for sched in (("exp", 0.0, 10), ("exp", -0.5, 10), ("exp", 0.5, 0), ("exp", 0.5, 1.5), ("cos", 0.5, 10),
                  ("exp", 0.5)):
        with pytest.raises(ValueError):
            G.StepGuard(lr_schedule=sched)
    with pytest.raises(ValueError):
        G.StepGuard(lr_schedule=("exp", 0.5, 10), lr_dev=torch.zeros(1))
    with pytest.raises(ValueError):
        G.StepGuard(lr_dev=torch.zeros(1))  # not a device tensor
    with pytest.raises(ValueError):
        G.StepGuard(lr_dev=0.1)


def test_clip_coef_closed_forms_and_torch():
    assert G.clip_coef(3.0, None) == 1.0 and G.clip_coef(3.0, math.inf) == 1.0
    assert G.clip_coef(0.0, 1.0) == 1.0                       # norm 0: 1e6 clamps to 1
    assert G.clip_coef(0.5, 1.0) == 1.0                       # below
    assert G.clip_coef(1.0, 1.0) == 1.0 / (1.0 + 1e-6) < 1.0  # equal: the 1e-6 shows
    assert G.clip_coef(4.0, 1.0) == 1.0 / (4.0 + 1e-6)        # above
    assert math.isnan(G.clip_coef(float("nan"), 1.0))
    assert G.clip_coef(math.inf, 1.0) == 0.0
    g = torch.tensor([3.0, -4.0, 12.0, 0.5, -0.25], dtype=torch.float64)
    for max_norm in (1.0, 5.0, 100.0):
        p = torch.nn.Parameter(torch.zeros(5, dtype=torch.float64))
        p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        assert abs(float(total) - math.sqrt(math.fsum(float(x) ** 2 for x in g))) <= 1e-12 * float(total)
        want = g * G.clip_coef(float(total), max_norm)
        assert torch.allclose(p.grad, want, rtol=1e-14, atol=0)


def test_lr_at_closed_forms():
    assert G.lr_at(3e-4, None, 77) == 3e-4
    s = ("exp", 0.5, 2)
    assert G.lr_at(0.25, s, 1) == 0.25 and G.lr_at(0.25, s, 3) == 0.125 and G.lr_at(0.25, s, 5) == 0.0625
    assert G.lr_at(0.25, s, 2) == 0.25 * 0.5 ** 0.5
    # MuZero's schedule: 0.1 decayed by 0.1 every 350e3 steps
    assert abs(G.lr_at(0.05, ("exp", 0.1, 350000), 350001) - 0.005) <= 1e-17


def _adam_f64(p, g, m, v, sc):
    """learn.hip's update, in f64, from the seven scalars."""
    ns, omb1, b2, omb2, bc, eps, wd = sc
    g = g + wd * p
    m = m + omb1 * (g - m)
    v = v * b2 + (omb2 * g) * g
    return p + (ns * m) / (v.sqrt() / bc + eps), m, v


@pytest.mark.parametrize("schedule", [None, ("exp", 0.5, 2)])
def test_adam_scalars_at_against_torch_adam(schedule):
    """Four steps of torch.optim.Adam (f64, weight decay, the lr of each step set as a scheduler would) on five
    elements against the kernel's update from adam_scalars_at(t)."""
    lr0 = 3e-2
    gen = torch.Generator().manual_seed(3)
    p = torch.nn.Parameter(torch.randn(5, dtype=torch.float64, generator=gen))
    opt = torch.optim.Adam([p], lr=lr0, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    q, m, v = p.detach().clone(), torch.zeros(5, dtype=torch.float64), torch.zeros(5, dtype=torch.float64)
    for t in range(1, 5):
        grad = torch.randn(5, dtype=torch.float64, generator=gen)
        opt.param_groups[0]["lr"] = G.lr_at(lr0, schedule, t)
        p.grad = grad.clone()
        opt.step()
        q, m, v = _adam_f64(q, grad, m, v, G.adam_scalars_at(t, lr0, schedule))
        assert torch.allclose(p.detach(), q, rtol=1e-13, atol=1e-15), t
        assert torch.allclose(opt.state[p]["exp_avg"], m, rtol=1e-13, atol=0)
        assert torch.allclose(opt.state[p]["exp_avg_sq"], v, rtol=1e-13, atol=0)


@pytest.mark.parametrize("t", TS)
def test_adam_scalars_at_equals_the_learner_s(t):
    from mzba.learner import ADAM_EPS, BETAS, WEIGHT_DECAY, Learner
    for lr in (3e-4, 0.05):
        a = np.asarray(G.adam_scalars_at(t, lr, None, BETAS, ADAM_EPS, WEIGHT_DECAY), np.float32)
        b = np.asarray(Learner._adam_scalars(types.SimpleNamespace(lr=lr), t), np.float32)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t, lr, a, b)
        assert G.adam_scalars_at(t, lr) == G.adam_scalars_at(t, lr, None, BETAS, ADAM_EPS, WEIGHT_DECAY)


def test_block_layout_matches_the_library():
    from mzba import _lib
    assert _lib.lib().mzba_guard_block_bytes() == G.BLOCK_DT.itemsize == 224 == 4 * G.BLOCK_WORDS
    off = {k: v[1] for k, v in G.BLOCK_DT.fields.items()}
    assert off == {"norm": 0, "seg_norm": 8, "seg_sumsq": 72, "seg_nonfinite": 136, "coef": 168, "nonfinite": 172,
                   "loss_nonfinite": 176, "skip": 180, "t_applied": 184, "skipped": 188, "lr": 192, "sc": 196}
    assert G.T_APPLIED_WORD == 46 and G.SKIPPED_WORD == 47


def test_guard_entry_points_reject_bad_arguments_without_gpu():
    from mzba import _lib
    L = _lib.lib()
    p, ws, blk = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(16384)
    b = lambda *v: (ctypes.c_longlong * len(v))(*v)  # noqa: E731
    chunk = 16384
    assert L.mzba_grad_stats_ws_bytes(0) == -1
    assert L.mzba_grad_stats_ws_bytes(1) == L.mzba_grad_stats_ws_bytes(chunk) == 16 + 96
    assert L.mzba_grad_stats_ws_bytes(chunk + 1) == 16 + 2 * 96
    big = 1 << 20
    assert L.mzba_grad_stats(None, 8, b(0, 8), 1, None, ws, big, None) == -1
    assert L.mzba_grad_stats(p, 0, b(0, 0), 1, None, ws, big, None) == -1
    assert L.mzba_grad_stats(p, 8, b(0, 8), 0, None, ws, big, None) == -1
    assert L.mzba_grad_stats(p, 8, b(*range(10)), 9, None, ws, big, None) == -1
    assert L.mzba_grad_stats(p, 8, b(0, 8), 1, None, ws, 16 + 96 - 1, None) == -2
    assert L.mzba_grad_stats(p, 8, b(0, 8), 1, None, ctypes.c_void_p(8200), big, None) == -2
    assert L.mzba_grad_stats(p, 8, b(0, 9), 1, None, ws, big, None) == -3
    assert L.mzba_grad_stats(p, 8, b(-1, 8), 1, None, ws, big, None) == -3
    assert L.mzba_grad_stats(p, 8, b(0, 5, 4, 8), 3, None, ws, big, None) == -3
    assert L.mzba_grad_stats_set_grid(-1) == -1

    def fin(ws=ws, n=8, nseg=1, blk=blk, max_norm=1.0, rate=1.0, steps=0, lr_dev=None, nbytes=big):
        return L.mzba_guard_finish(ws, nbytes, n, nseg, blk, max_norm, 1, 3e-4, rate, steps, lr_dev, 0.9, 0.999, 1e-8,
                                   1e-4, None)
    assert fin(ws=None) == -1 and fin(blk=None) == -1 and fin(n=0) == -1 and fin(nseg=9) == -1
    assert fin(nbytes=16 + 96 - 1) == -2 and fin(blk=ctypes.c_void_p(16388)) == -2
    assert fin(max_norm=0.0) == -3 and fin(max_norm=float("nan")) == -3 and fin(steps=-1) == -3
    assert fin(rate=0.0, steps=5) == -3 and fin(steps=5, lr_dev=p) == -3
    assert L.mzba_adam_guard(p, p, p, p, -1, blk, None) == -1
    assert L.mzba_adam_guard(p, p, p, p, 8, None, None) == -1
    assert L.mzba_adam_guard(p, p, p, p, 0, blk, None) == 0
    assert L.mzba_guard_snapshot(None, 3, None) == -1 and L.mzba_guard_snapshot(p, -1, None) == -1
    assert L.mzba_guard_snapshot(p, 0, None) == 0
    assert L.mzba_guard_restore(p, 3, None, None) == -1 and L.mzba_guard_restore(p, 0, blk, None) == 0
    f = ctypes.c_float
    assert L.mzba_replay_priority_update_g(p, p, p, 4, 16, f(1.0), f(1e-3), None, None) == -1
    assert L.mzba_replay_priority_update_g(p, p, p, 4, 0, f(1.0), f(1e-3), blk, None) == -1
    assert L.mzba_replay_priority_update_g(p, p, p, 0, 16, f(1.0), f(1e-3), blk, None) == 0
