"""The error-bound idiom shared by tests/test_gpu_learner_ops.py and tests/test_gpu_acting_ops.py (their module
docstrings state it): e_k, the kernel's error against an f64 evaluation, within 4 e_w + c 2^-24 S, e_w the error of a
plain torch f32 CPU evaluation (the witness) against the same reference; and the seeded generator of a case's inputs."""
import torch

U = 2.0 ** -24   # f32 unit roundoff
BF = 2.0 ** -8   # bf16 unit roundoff (round to nearest even)


def _gen(*key):
    seed = 0
    for k in key:  # a fixed polynomial of the case's parameters: the same inputs on every interpreter
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _check(name, got, ref, wit, cS, out_bf16=False, ulps=1.0):
    """e_k <= 4 e_w + 2^-24 cS (+ ulps 2^-8 |ref| for a bf16 output), element by element; prints e_k and e_w."""
    got, ref, wit = got.detach().cpu().double(), ref.detach().double(), wit.detach().double()
    assert got.shape == ref.shape == wit.shape, (name, got.shape, ref.shape, wit.shape)
    assert torch.isfinite(got).all(), name
    e = (got - ref).abs()
    e_w = (wit - ref).abs().max().item() if ref.numel() else 0.0
    bound = torch.zeros_like(ref) + 4.0 * e_w + U * cS
    if out_bf16:
        bound = bound + ulps * BF * ref.abs()
    e_k = e.max().item() if ref.numel() else 0.0
    print(f"{name}: e_k {e_k:.3e} e_w {e_w:.3e}")
    over = (e - bound).flatten()
    i = int(over.argmax())
    assert over[i] <= 0, (name, "err", e.flatten()[i].item(), "bound", bound.flatten()[i].item(), "e_w", e_w, "at", i)
    return e_k, e_w
