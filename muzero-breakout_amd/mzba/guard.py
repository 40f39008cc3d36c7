"""Learner step guard: what `Learner(..., guard=StepGuard(...))` watches on the device.

`StepGuard` is configuration only. The arithmetic runs in csrc/guard.hip inside the minibatch (captured or eager):
the gradient's f64 norm per net, `clip_grad_norm_`'s coefficient, the skip of a step whose gradient or loss is not
finite, the device step counter, the learning rate of that step and Adam's seven scalars. `clip_coef`, `lr_at` and
`adam_scalars_at` restate those formulas in plain Python for the tests; nothing in the product calls them.

`BLOCK_DT` is include/mzba.h's `mzba_guard_block`; `read_block` turns the device block into a dict.
"""
import math

import numpy as np

MAX_SEG = 8
BLOCK_DT = np.dtype([("norm", "<f8"), ("seg_norm", "<f8", (MAX_SEG,)), ("seg_sumsq", "<f8", (MAX_SEG,)),
                     ("seg_nonfinite", "<i4", (MAX_SEG,)), ("coef", "<f4"), ("nonfinite", "<i4"),
                     ("loss_nonfinite", "<i4"), ("skip", "<i4"), ("t_applied", "<i4"), ("skipped", "<i4"),
                     ("lr", "<f4"), ("sc", "<f4", (7,))])
BLOCK_WORDS = BLOCK_DT.itemsize // 4  # the device block is an i32 tensor of this many words
T_APPLIED_WORD = BLOCK_DT.fields["t_applied"][1] // 4
SKIPPED_WORD = BLOCK_DT.fields["skipped"][1] // 4


class StepGuard:
    """max_norm: clip the gradient's global L2 norm to it (None: no clipping).
    skip_nonfinite: a minibatch whose gradient holds an Inf / NaN, or whose loss is one, changes nothing.
    lr_schedule: ("exp", rate, steps): lr = lr0 * rate ** ((t - 1) / steps) at optimizer step t (MuZero's decay on
    the number of steps applied before this one). lr_dev: a device f32 tensor of one element the caller owns and
    may rewrite between steps; its value is the learning rate. Not both.
    A captured minibatch holds the base rate (Learner.lr) it was captured with: to move the rate between replays by
    hand, use lr_dev."""

    def __init__(self, max_norm=None, skip_nonfinite=True, lr_schedule=None, lr_dev=None):
        if max_norm is not None:
            max_norm = float(max_norm)
            if not max_norm > 0:
                raise ValueError("StepGuard: max_norm must be > 0")
        if lr_schedule is not None:
            if lr_dev is not None:
                raise ValueError("StepGuard: give lr_schedule or lr_dev, not both")
            if len(lr_schedule) != 3 or lr_schedule[0] != "exp":
                raise ValueError('StepGuard: lr_schedule is ("exp", rate, steps)')
            _, rate, steps = lr_schedule
            if not float(rate) > 0:
                raise ValueError("StepGuard: the schedule's rate must be > 0")
            if int(steps) != steps or int(steps) < 1:
                raise ValueError("StepGuard: the schedule's steps must be an integer >= 1")
            lr_schedule = ("exp", float(rate), int(steps))
        if lr_dev is not None:
            import torch
            if not (isinstance(lr_dev, torch.Tensor) and lr_dev.dtype == torch.float32 and lr_dev.numel() == 1
                    and lr_dev.is_cuda):
                raise ValueError("StepGuard: lr_dev is a device f32 tensor of one element")
        self.max_norm, self.skip_nonfinite = max_norm, bool(skip_nonfinite)
        self.lr_schedule, self.lr_dev = lr_schedule, lr_dev


def clip_coef(norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient; None / inf: exactly 1."""
    if max_norm is None or max_norm == math.inf:
        return 1.0
    c = max_norm / (norm + 1e-6)
    return c if (c < 1.0 or c != c) else 1.0


def lr_at(lr0, schedule, t):
    """The learning rate of optimizer step t (1-based)."""
    if schedule is None:
        return lr0
    _, rate, steps = schedule
    return lr0 * rate ** ((t - 1) / steps)


def adam_scalars_at(t, lr0, schedule=None, betas=(0.9, 0.999), eps=1e-8, wd=1e-4):
    """Learner._adam_scalars(t) with the learning rate of step t."""
    b1, b2 = betas
    lr = lr_at(lr0, schedule, t)
    return [-(lr / (1 - b1 ** t)), 1 - b1, b2, 1 - b2, (1 - b2 ** t) ** 0.5, eps, wd]


def read_block(block, nseg):
    """The device stats block (i32[BLOCK_WORDS]) as a dict of Python values; one device-to-host copy."""
    r = block.cpu().numpy().view(BLOCK_DT)[0]
    return {"grad_norm": float(r["norm"]), "seg_norm": [float(x) for x in r["seg_norm"][:nseg]],
            "seg_sumsq": [float(x) for x in r["seg_sumsq"][:nseg]],
            "seg_nonfinite": [int(x) for x in r["seg_nonfinite"][:nseg]], "coef": float(r["coef"]),
            "nonfinite": int(r["nonfinite"]), "loss_nonfinite": int(r["loss_nonfinite"]), "skip": int(r["skip"]),
            "t_applied": int(r["t_applied"]), "skipped": int(r["skipped"]), "lr": float(r["lr"]),
            "adam_scalars": [float(x) for x in r["sc"]]}
