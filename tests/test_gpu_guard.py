"""The learner step guard on the GPU (csrc/guard.hip, mzba/guard.py, Learner(guard=...)).

  mzba_grad_stats + mzba_guard_finish   per-segment f64 sums of squares against math.fsum of the exact squares (an f32
      square is exact in f64), within n 2^-53 relative: what any order of f64 summation over n non-negative terms can
      differ from the exact sum by. Non-finite counts exact. Bit-equal between runs, between a one-workgroup grid and
      the default one, and between the 16-byte and the scalar load paths.
  mzba_guard_finish    coef, skip, the device step counter, the learning rate and Adam's scalars against
      mzba.guard's plain-Python formulas.
  mzba_adam_guard      coef 1 / skip 0: mzba_adam's bits. coef 0.5: the f64 formula under test_adam's chain bounds
      (restated: m' = m + (1 - b1)(g - m), g = c grad + wd p: 6 operations on |m| + |g|; v' = b2 v + ((1 - b2) g) g: 8
      relative, the two of g's that the multiply by c adds enter squared: 10; denom = sqrt(v') / bc2 + eps: 8 relative;
      U = neg_step m' / denom: |neg_step| cs_m / denom + 11 |U|; p' = p + U: one more on |p| + |U|), with
      torch.optim.Adam in f32 on the CPU as the witness: e_k <= 4 e_w + 2^-24 cS.
  Learner(guard=...)   narrow nets, B = 8, f32 and bf16: identity with an unguarded twin, clipping, a poisoned step,
      a captured schedule replayed with no host input, the optimizer checkpoint.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
CH = 16384                      # csrc/guard.hip GS_CH
BIG = 1024 * CH + CH + 5        # more chunks than a default grid has workgroups: a second grid-stride pass
TS = (1, 2, 10, 1000, 100000)
LR = 3e-4


def _L():
    from mzba import _lib as L
    return L


def _G():
    from mzba import guard as G
    return G


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _close64(a, b, ulps=1):
    """Two doubles within `ulps` f64 ulps: the device's f64 sqrt against the host's."""
    return abs(a - b) <= ulps * 2.0 ** -52 * abs(b)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _block(**fields):
    """A device stats block with the given fields set (the others zero)."""
    G = _G()
    r = np.zeros(1, G.BLOCK_DT)
    for k, v in fields.items():
        r[k] = v
    return torch.from_numpy(r.view(np.int32).copy()).cuda()


def _stats(gv, bounds, loss=None, grid=0, block=None, max_norm=math.inf, skip_nonfinite=1, lr0=LR, schedule=None,
           lr_dev=None):
    """mzba_grad_stats + mzba_guard_finish on the device view gv; returns (block tensor, dict)."""
    L, G = _L(), _G()
    n, nseg = gv.numel(), len(bounds) - 1
    ws = torch.empty(int(L.lib().mzba_grad_stats_ws_bytes(n)), dtype=torch.uint8, device="cuda")
    blk = _block() if block is None else block
    b = (ctypes.c_longlong * len(bounds))(*bounds)
    rate, steps = schedule[1:] if schedule is not None else (1.0, 0)
    L.call("mzba_grad_stats_set_grid", grid)
    try:
        L.call("mzba_grad_stats", L.ptr(gv), n, b, nseg, L.ptr(loss), L.ptr(ws), ws.numel(), L.stream())
    finally:
        L.call("mzba_grad_stats_set_grid", 0)
    L.call("mzba_guard_finish", L.ptr(ws), ws.numel(), n, nseg, L.ptr(blk), max_norm, skip_nonfinite, lr0, rate,
           steps, L.ptr(lr_dev), 0.9, 0.999, 1e-8, 1e-4, L.stream())
    torch.cuda.synchronize()
    return blk, G.read_block(blk, nseg)


@functools.lru_cache(maxsize=None)
def _wide(n):
    """n f32 values of either sign with magnitudes from 1e-20 to 1e18: their squares underflow and overflow f32."""
    g = _gen(31, n)
    mag = torch.empty(n, dtype=torch.float64).uniform_(-20.0, 18.0, generator=g)
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    x = (sign * 10.0 ** mag).float()
    x[0] = 1e-20 if n > 1 else x[0]
    x[-1] = -1e18 if n > 2 else x[-1]
    assert torch.isfinite(x).all()
    return x


@functools.lru_cache(maxsize=None)
def _exact(n, bounds):
    x = _wide(n).double().numpy()
    return [math.fsum(np.square(x[lo:hi]).tolist()) for lo, hi in zip(bounds[:-1], bounds[1:])]


def _three(n):
    """Three segments whose four bounds are no multiples of 4 (and so on no chunk border)."""
    if n < 16:
        return (1, 2, 5, 7)
    last = n if n % 4 else n - 1
    return (1, (n // 3) | 1, (2 * n // 3) | 3, last)


def _place(x, misaligned):
    buf = torch.zeros(x.numel() + 8, device="cuda")
    off = 1 if misaligned else 0
    buf[off:off + x.numel()] = x.cuda()
    v = buf[off:off + x.numel()]
    assert (v.data_ptr() % 16 != 0) == misaligned
    return v


@pytest.mark.parametrize("n,misaligned", [(1, False), (7, False), (8, False), (8, True), (CH - 1, False), (CH, False),
                                          (CH + 1, False), (CH + 1, True), (BIG, False)])
def test_grad_stats_against_fsum(n, misaligned):
    x = _wide(n)
    gv = _place(x, misaligned)
    # the largest size takes the three segments only: one exact sum over its 16.8 M squares
    for bounds in ([(0, n)] if n < BIG else []) + ([_three(n)] if n >= 7 else []):
        assert len(bounds) == 2 or all(b % 4 for b in bounds)
        ref = _exact(n, bounds)
        blk, d = _stats(gv, bounds)
        for s, (got, want) in enumerate(zip(d["seg_sumsq"], ref)):
            cnt = bounds[s + 1] - bounds[s]
            rel = abs(got - want) / want
            print(f"grad_stats n {n} misaligned {int(misaligned)} seg {s} [{bounds[s]}, {bounds[s + 1]}): "
                  f"rel err {rel:.3e} bound {cnt * 2.0 ** -53:.3e}")
            assert rel <= cnt * 2.0 ** -53, (n, bounds, s, got, want)
            assert _close64(d["seg_norm"][s], math.sqrt(got))
        assert d["seg_nonfinite"] == [0] * len(ref) and d["nonfinite"] == 0 and d["skip"] == 0
        tot = 0.0
        for v in d["seg_sumsq"]:
            tot = tot + v
        assert _close64(d["grad_norm"], math.sqrt(tot))
        # two runs, and a one-workgroup grid against the default: the same bits
        again, _ = _stats(gv, bounds)
        one, _ = _stats(gv, bounds, grid=1)
        assert torch.equal(blk, again) and torch.equal(blk, one), (n, bounds)
        if n > CH:  # and an in-between grid that divides nothing
            assert torch.equal(blk, _stats(gv, bounds, grid=3)[0])


def test_grad_stats_load_paths_agree():
    """The same data behind an aligned and a misaligned pointer (16-byte loads / scalar loads): the same bits."""
    n = 3 * CH + 5
    x = _wide(n)
    a, _ = _stats(_place(x, False), (0, n))
    b, _ = _stats(_place(x, True), (0, n))
    assert torch.equal(a, b)


def test_grad_stats_counts_nonfinite():
    """n = two chunks + 7, five segments: chunk 0 holds three segment borders (scalar loads), chunk 1 lies inside one
    segment (16-byte loads), the last 7 elements are the scalar tail. +Inf in element 0, -Inf on a segment border and
    just before one, NaN in the last element, one more inside the scalar tail, one inside the 16-byte chunk; each alone,
    then all together."""
    n = 2 * CH + 7
    bounds = (0, 1001, 5002, 9003, 2 * CH + 2, n)
    inf, nan = float("inf"), float("nan")
    spots = {"+inf at 0": (0, inf), "-inf on a border": (1001, -inf), "nan last": (n - 1, nan),
             "inf in the scalar tail": (2 * CH + 3, inf), "-inf before a border": (9002, -inf),
             "nan in the 16-byte chunk": (CH + 4321, nan)}
    base = _wide(n)
    ref = _exact(n, bounds)

    def seg_of(i):
        return max(s for s in range(5) if bounds[s] <= i)

    for name, cases in list((k, [v]) for k, v in spots.items()) + [("all", list(spots.values()))]:
        x = base.clone()
        want = [0] * 5
        for i, v in cases:
            x[i] = v
            want[seg_of(i)] += 1
        _, d = _stats(_place(x, False), bounds, skip_nonfinite=1)
        assert d["seg_nonfinite"] == want and d["nonfinite"] == sum(want) and d["skip"] == 1, (name, d)
        for s in range(5):
            if want[s] == 0:
                assert abs(d["seg_sumsq"][s] - ref[s]) <= (bounds[s + 1] - bounds[s]) * 2.0 ** -53 * ref[s], (name, s)
            else:
                assert not math.isfinite(d["seg_sumsq"][s]), (name, s)
        assert not math.isfinite(d["grad_norm"])
        _, d0 = _stats(_place(x, False), bounds, skip_nonfinite=0)
        assert d0["nonfinite"] == sum(want) and d0["skip"] == 0 and d0["t_applied"] == 1


def test_grad_stats_ignores_what_lies_outside_the_segments():
    n = 64
    x = _wide(n).clone()
    x[0], x[n - 1] = float("nan"), float("inf")
    _, d = _stats(_place(x, False), (1, 30, n - 1))
    assert d["nonfinite"] == 0 and d["skip"] == 0 and math.isfinite(d["grad_norm"])


# ====================================================================== mzba_guard_finish
def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32))) if np.sign(a) == np.sign(b) else 1 << 30


def test_finish_clip_coefficient():
    """g = (3, 4): norm exactly 5. Below, at and above max_norm; +inf; norm 0."""
    G = _G()
    gv = _place(torch.tensor([3.0, 4.0]), False)
    for max_norm in (10.0, 5.0, 2.5, 1e-3, math.inf):
        _, d = _stats(gv, (0, 2), max_norm=max_norm)
        assert _close64(d["grad_norm"], 5.0) and d["seg_norm"] == [d["grad_norm"]] and d["seg_sumsq"] == [25.0]
        assert _ulps(d["coef"], G.clip_coef(5.0, max_norm)) <= 1, (max_norm, d["coef"])
    assert _stats(gv, (0, 2), max_norm=10.0)[1]["coef"] == 1.0
    assert _stats(gv, (0, 2), max_norm=math.inf)[1]["coef"] == 1.0
    assert _stats(gv, (0, 2), max_norm=5.0)[1]["coef"] < 1.0
    assert _ulps(_stats(gv, (0, 2), max_norm=2.5)[1]["coef"], 2.5 / (5.0 + 1e-6)) <= 1
    _, d = _stats(_place(torch.zeros(9), False), (0, 9), max_norm=1.0)
    assert d["grad_norm"] == 0.0 and d["coef"] == 1.0 and d["skip"] == 0


def test_finish_skip_and_step_counter():
    gv = _place(torch.tensor([3.0, 4.0, 0.5]), False)
    bad = _place(torch.tensor([3.0, float("nan"), 0.5]), False)
    ok_loss = torch.tensor([1.0, 0.5, 0.25, 0.25], device="cuda")
    blk = _block(t_applied=7, skipped=2)
    for g_, loss, sk, want_skip in ((gv, ok_loss, 1, 0), (bad, ok_loss, 1, 1), (bad, ok_loss, 0, 0), (gv, None, 1, 0)):
        before = _G().read_block(blk, 1)
        _, d = _stats(g_, (0, 3), loss=loss, block=blk, skip_nonfinite=sk)
        assert d["skip"] == want_skip
        assert d["t_applied"] == before["t_applied"] + (1 - want_skip)
        assert d["skipped"] == before["skipped"] + want_skip
    for i, v in enumerate((float("nan"), float("inf"), -float("inf"), float("nan"))):
        loss = ok_loss.clone()
        loss[i] = v
        before = _G().read_block(blk, 1)
        _, d = _stats(gv, (0, 3), loss=loss, block=blk, skip_nonfinite=1)
        assert d["skip"] == 1 and d["loss_nonfinite"] == 1 and d["nonfinite"] == 0
        assert d["t_applied"] == before["t_applied"] and d["skipped"] == before["skipped"] + 1
        _, d = _stats(gv, (0, 3), loss=loss, block=blk, skip_nonfinite=0)
        assert d["skip"] == 0 and d["loss_nonfinite"] == 1 and d["t_applied"] == before["t_applied"] + 1


@pytest.mark.parametrize("schedule", [None, ("exp", 0.1, 350000), ("exp", 0.5, 2)])
def test_finish_scalars(schedule):
    """Adam's seven scalars and the learning rate for t in TS (the counter seeded with t - 1) within one f32 ulp of
    adam_scalars_at / lr_at: a double chain with relative error <= 1e-13 rounds to another f32 only at a midpoint."""
    G = _G()
    gv = _place(torch.tensor([3.0, 4.0]), False)
    for lr0 in (LR, 0.05):
        for t in TS:
            if schedule == ("exp", 0.5, 2) and t > 100:
                continue  # 0.5 ** 500 and below: f32 denormals and zero, where "one ulp" is no relative statement
            _, d = _stats(gv, (0, 2), block=_block(t_applied=t - 1), lr0=lr0, schedule=schedule)
            assert d["t_applied"] == t
            want = G.adam_scalars_at(t, lr0, schedule)
            for i, (a, b) in enumerate(zip(d["adam_scalars"], want)):
                assert _ulps(a, b) <= 1, (t, lr0, i, a, b)
            assert _ulps(d["lr"], G.lr_at(lr0, schedule, t)) <= 1


def test_finish_first_steps_equal_the_host_scalars():
    """t = 1, 2, 3 at lr 3e-4: the device scalars are the f32 roundings of Learner._adam_scalars — the learner
    identity test rests on this."""
    import types
    from mzba.learner import Learner
    gv = _place(torch.tensor([3.0, 4.0]), False)
    blk = _block()
    for t in (1, 2, 3):
        _, d = _stats(gv, (0, 2), block=blk, lr0=LR)
        want = np.asarray(Learner._adam_scalars(types.SimpleNamespace(lr=LR), t), np.float32)
        got = np.asarray(d["adam_scalars"], np.float32)
        assert d["t_applied"] == t and np.array_equal(got.view(np.int32), want.view(np.int32)), (t, got, want)
        assert np.float32(d["lr"]) == np.float32(LR)


def test_finish_device_learning_rate():
    G = _G()
    gv = _place(torch.tensor([3.0, 4.0]), False)
    lr_dev = torch.tensor([0.0125], device="cuda")
    blk = _block(t_applied=4)
    _, d = _stats(gv, (0, 2), block=blk, lr_dev=lr_dev)
    want = G.adam_scalars_at(5, float(np.float32(0.0125)))
    assert d["lr"] == float(np.float32(0.0125)) and _ulps(d["adam_scalars"][0], want[0]) <= 1
    lr_dev.fill_(0.5)
    _, d = _stats(gv, (0, 2), block=blk, lr_dev=lr_dev)
    assert d["lr"] == 0.5 and d["t_applied"] == 6 and _ulps(d["adam_scalars"][0], G.adam_scalars_at(6, 0.5)[0]) <= 1


# ====================================================================== mzba_adam_guard
def _check(name, got, ref, wit, cS):
    """e_k <= 4 e_w + 2^-24 cS, element by element; prints e_k and e_w."""
    got, ref, wit = got.detach().cpu().double(), ref.detach().double(), wit.detach().double()
    assert got.shape == ref.shape == wit.shape and torch.isfinite(got).all(), name
    e = (got - ref).abs()
    e_w = (wit - ref).abs().max().item()
    over = (e - (4.0 * e_w + U * cS)).flatten()
    i = int(over.argmax())
    print(f"{name}: e_k {e.max().item():.3e} e_w {e_w:.3e}")
    assert over[i] <= 0, (name, "err", e.flatten()[i].item(), "e_w", e_w, "at", i)


def _adam_reference(p0, grad, m0, v0, sc, coef, lr, t):
    """The guarded update in f64 from the f32 scalars sc and coefficient coef, its chain bounds (module docstring),
    and torch.optim.Adam in f32 on the CPU on the scaled gradient as the witness."""
    ns_, omb1, b2, omb2, bc, eps, wd = [float(np.float32(s)) for s in sc]
    c = float(np.float32(coef))
    p64, g64, m64, v64 = p0.double(), grad.double(), m0.double(), v0.double()
    gg = c * g64 + wd * p64
    m1 = m64 + omb1 * (gg - m64)
    v1 = v64 * b2 + (omb2 * gg) * gg
    den = v1.sqrt() / bc + eps
    upd = (ns_ * m1) / den
    p1 = p64 + upd
    cs_m = 6 * (m64.abs() + gg.abs())
    cs_v = 10 * v1
    cs_p = abs(ns_) * cs_m / den + 11 * upd.abs() + (p64.abs() + upd.abs())
    pw = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([pw], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4)
    opt.state[pw] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    pw.grad = grad * c  # c is an f32 value: one f32 multiply per element, as the kernel's
    opt.step()
    return (p1, m1, v1), (cs_p, cs_m, cs_v), (pw.detach(), opt.state[pw]["exp_avg"], opt.state[pw]["exp_avg_sq"])


@functools.lru_cache(maxsize=None)
def _adam_data(n):
    g = _gen(20, n)
    return (torch.randn(n, generator=g), 0.1 * torch.randn(n, generator=g), 0.01 * torch.randn(n, generator=g),
            1e-3 * torch.rand(n, generator=g))


def _adam_buffers(n, misaligned, fill=0.0):
    off = 1 if misaligned else 0
    bufs = []
    for src in _adam_data(n):
        b = torch.full((n + 4,), fill, device="cuda")
        b[off:off + n] = src.cuda()
        bufs.append(b)
    views = [b[off:off + n] for b in bufs]
    assert all((v.data_ptr() % 16 != 0) == misaligned for v in views)
    return bufs, views, off


@pytest.mark.parametrize("n,misaligned", [(7, False), (8, False), (8, True), (4 * 16384 * 256 + 4, False)])
@pytest.mark.parametrize("t", [1, 1000])
def test_adam_guard(n, misaligned, t):
    L, G = _L(), _G()
    sc = G.adam_scalars_at(t, LR)
    p0, grad, m0, v0 = _adam_data(n)
    # coef 1, skip 0: mzba_adam's bits
    _, plain, _ = _adam_buffers(n, misaligned)
    L.call("mzba_adam", *[L.ptr(v) for v in plain], n, *sc, L.stream())
    bufs, views, off = _adam_buffers(n, misaligned)
    L.call("mzba_adam_guard", *[L.ptr(v) for v in views], n, L.ptr(_block(coef=1.0, skip=0, sc=sc)), L.stream())
    torch.cuda.synchronize()
    for a, b in zip(plain, views):
        assert _same(a, b)
    for b in bufs:
        assert (b[:off] == 0).all() and (b[off + n:] == 0).all()
    # coef 0.5: the f64 formula on the scaled gradient
    bufs, views, off = _adam_buffers(n, misaligned)
    L.call("mzba_adam_guard", *[L.ptr(v) for v in views], n, L.ptr(_block(coef=0.5, skip=0, sc=sc)), L.stream())
    torch.cuda.synchronize()
    ref, cs, wit = _adam_reference(p0, grad, m0, v0, sc, 0.5, LR, t)
    pk, gk, mk, vk = [v.cpu() for v in views]
    assert torch.equal(gk, grad)
    tag = f"adam_guard coef 0.5 n {n} misaligned {int(misaligned)} t {t}"
    for name, got, r, c, w in zip("pmv", (pk, mk, vk), ref, cs, wit):
        _check(f"{tag} {name}", got, r, w, c)
    assert not _same(pk, plain[0].cpu())
    # skip 1: nothing is stored, the words around the arrays included
    bufs, views, off = _adam_buffers(n, misaligned, fill=float("nan"))
    before = [b.clone() for b in bufs]
    L.call("mzba_adam_guard", *[L.ptr(v) for v in views], n, L.ptr(_block(coef=0.5, skip=1, sc=sc)), L.stream())
    torch.cuda.synchronize()
    for a, b in zip(before, bufs):
        assert _same(a, b)


def test_guarded_priority_update_and_restore_follow_skip():
    """mzba_replay_priority_update_g and mzba_guard_restore act on skip alone; mzba_guard_snapshot always copies."""
    L = _L()
    cap, n = 40, 6
    slots = torch.tensor([3, 39, 0, 17, -1, 40], dtype=torch.int32, device="cuda")
    td = torch.rand(n, generator=_gen(5)).cuda()
    outs = {}
    for skip in (0, 1):
        q = torch.full((cap,), 0.25, device="cuda")
        L.call("mzba_replay_priority_update_g", L.ptr(q), L.ptr(slots), L.ptr(td), n, cap, 0.6, 1e-3,
               L.ptr(_block(skip=skip)), L.stream())
        outs[skip] = q
    q = torch.full((cap,), 0.25, device="cuda")
    L.call("mzba_replay_priority_update", L.ptr(q), L.ptr(slots), L.ptr(td), n, cap, 0.6, 1e-3, L.stream())
    torch.cuda.synchronize()
    assert _same(outs[0], q) and (outs[1] == 0.25).all() and not _same(outs[0], outs[1])
    # table of three tensors (sizes below, at and above one workgroup's 256 threads)
    live = [torch.rand(k, generator=_gen(6, k)).cuda() for k in (5, 256, 700)]
    snap = [torch.full((k + 2,), -1.0, device="cuda") for k in (5, 256, 700)]
    rec = np.zeros(3, np.dtype([("live", "<u8"), ("snap", "<u8"), ("n", "<i4"), ("pad", "<i4")]))
    for r, a, b in zip(rec, live, snap):
        r["live"], r["snap"], r["n"] = a.data_ptr(), b.data_ptr() + 4, a.numel()
    tab = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    orig = [a.clone() for a in live]
    L.call("mzba_guard_snapshot", L.ptr(tab), 3, L.stream())
    for a in live:
        a.mul_(2.0)
    L.call("mzba_guard_restore", L.ptr(tab), 3, L.ptr(_block(skip=0)), L.stream())
    torch.cuda.synchronize()
    for a, o, b in zip(live, orig, snap):
        assert torch.equal(a, o * 2) and torch.equal(b[1:-1], o) and b[0] == -1 and b[-1] == -1
    L.call("mzba_guard_restore", L.ptr(tab), 3, L.ptr(_block(skip=1)), L.stream())
    torch.cuda.synchronize()
    for a, o in zip(live, orig):
        assert _same(a, o)


# ====================================================================== the learner
B = 8
POISON = "pred_net.value_head.2.bias"


def _minibatch_arrays(n, seed):
    g = np.random.default_rng(seed)
    lut = np.array([0, 0.3, 0.6, 1.0], np.float32)
    mb = dict(states=lut[g.integers(0, 4, (n, 4, 16, 20)) * (g.random((n, 4, 16, 20)) < 0.3)],
              past_actions=g.integers(0, 3, (n, 4)), future_actions=g.integers(0, 3, (n, 5)),
              rewards=g.choice(np.array([-1, 0, 1], np.float32), (n, 5)),
              targets=(g.normal(size=(n, 5)) * 2).astype(np.float32),
              counts=g.multinomial(50, [0.3, 0.3, 0.4], (n, 5)).astype(np.float32))
    values = (mb["targets"] + g.normal(size=(n, 5)) * 0.5).astype(np.float32)
    return mb, values


def _ring(n=64, seed=4):
    """A DeviceReplayBuffer(prioritized=True) of n explicit windows, priorities by the ingest rule."""
    from mzba.learner import MinibatchRing
    from mzba.replay import DeviceReplayBuffer
    mb, values = _minibatch_arrays(n, seed)
    src = MinibatchRing(mb)
    buf = DeviceReplayBuffer(4, 5, n, 0.997, 8, prioritized=True, alpha=0.6, beta=0.4, prio_eps=1e-3)
    for k, t in src._ring.items():
        buf._ring[k].copy_(t)
    buf._ring["values"].copy_(torch.from_numpy(values))
    buf.start, buf.length = 0, n
    buf._init_priorities(0, n)
    return buf


def _learner(dtype, guard, seed=6):
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    lm = learner_model_cfg()
    return Learner(lm, init_state_dict(lm, seed), K=5, dtype=dtype, lr=LR, guard=guard)


def _running(lrn):
    return [t.clone() for k in lrn.bn_keys for t in lrn.run[k]]


def _state(lrn):
    return [lrn.P.clone(), lrn.M1.clone(), lrn.M2.clone()] + _running(lrn)


def _slots(i):
    return torch.arange(3 + 8 * i, 3 + 8 * i + B, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("captured", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_default_guard_is_the_unguarded_step(dtype, captured):
    """StepGuard() (no clip, no schedule) over three minibatches: losses, P, M1, M2 and the running statistics bit-equal
    to an unguarded twin's; eager, and one eager minibatch followed by two replays of the captured one."""
    G = _G()
    ring = _ring()
    out = []
    for guard in (None, G.StepGuard()):
        lrn = _learner(dtype, guard)
        losses = [lrn.train_minibatch(ring, _slots(0)).clone()]
        if captured:
            lrn.capture(ring, B)
        for i in (1, 2):
            losses.append(lrn.train_minibatch(ring, _slots(i)).clone())
        assert lrn.step_count == 3 and lrn.applied_steps() == 3
        out.append((losses, _state(lrn), lrn))
    for a, b in zip(out[0][0], out[1][0]):
        assert _same(a, b)
    for i, (a, b) in enumerate(zip(out[0][1], out[1][1])):
        assert _same(a, b), i
    d = out[1][2].guard_stats()
    assert d["coef"] == 1.0 and d["skip"] == 0 and d["skipped"] == 0 and d["t_applied"] == 3 and d["nonfinite"] == 0
    assert d["segments"] == ["rep_net", "dyn_net", "pred_net"] and all(v > 0 for v in d["seg_norm"])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_clipped_step(dtype):
    """max_norm = half the first minibatch's norm: P after the step is the f64 Adam formula on coef G within the
    chain bounds; the block's norm is that of learner.G (fsum, n 2^-53); the per-net norms square-sum to it."""
    G = _G()
    ring = _ring()
    probe = _learner(dtype, G.StepGuard())
    probe.train_minibatch(ring, _slots(0))
    norm = probe.guard_stats()["grad_norm"]
    lrn = _learner(dtype, G.StepGuard(max_norm=0.5 * norm))
    p0 = lrn.P.clone().cpu()
    lrn.train_minibatch(ring, _slots(0))
    d = lrn.guard_stats()
    g = lrn.G.cpu()
    assert _same(g, probe.G.cpu()) and d["grad_norm"] == norm
    n = g.numel()
    x = g.double().numpy()
    exact = math.fsum(np.square(x).tolist())
    total = 0.0
    for v in d["seg_sumsq"]:
        total = total + v
    print(f"clipped step {dtype}: n {n} norm {norm:.9e} rel err of the sum {abs(total - exact) / exact:.3e}")
    assert abs(total - exact) <= n * 2.0 ** -53 * exact and _close64(d["grad_norm"], math.sqrt(total))
    for (lo, hi), got in zip(zip(lrn.guard_bounds[:-1], lrn.guard_bounds[1:]), d["seg_sumsq"]):
        want = math.fsum(np.square(x[lo:hi]).tolist())
        assert abs(got - want) <= (hi - lo) * 2.0 ** -53 * want
    sq = math.fsum(v * v for v in d["seg_norm"])
    assert abs(sq - norm * norm) <= 16 * 2.0 ** -53 * norm * norm
    assert _ulps(d["coef"], G.clip_coef(norm, 0.5 * norm)) <= 1 and 0.4 < d["coef"] < 0.5
    z = torch.zeros(n)
    ref, cs, wit = _adam_reference(p0, g, z, z, d["adam_scalars"], d["coef"], LR, 1)
    for name, got, r, c, w in zip("pmv", (lrn.P, lrn.M1, lrn.M2), ref, cs, wit):
        _check(f"clipped step {dtype} {name}", got, r, w, c)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_poisoned_step_is_skipped(dtype):
    """NaN in one element of the value head's bias: the guarded prioritized step changes nothing but the skip count;
    repaired, the next one applies as step t + 1 and rewrites the sampled slots' priorities only. The unguarded twin
    ends with NaN in P and in q."""
    G = _G()
    guarded, plain = _learner(dtype, G.StepGuard()), _learner(dtype, None)
    rg, rp = _ring(), _ring()
    for lrn, ring in ((guarded, rg), (plain, rp)):
        lrn.prioritized_step(ring, B, seed=7)
    assert _same(guarded.P, plain.P) and _same(rg._q, rp._q) and guarded.applied_steps() == 1
    off = guarded.params[POISON].off
    good = guarded.P[off].clone()
    for lrn in (guarded, plain):
        lrn.P[off] = float("nan")
    before, q0 = _state(guarded), rg._q.clone()
    loss = guarded.prioritized_step(rg, B, seed=7)
    assert not torch.isfinite(loss).all() and not torch.isfinite(guarded.last_td).all()
    for i, (a, b) in enumerate(zip(before, _state(guarded))):
        assert _same(a, b), i
    assert _same(q0, rg._q)
    d = guarded.guard_stats()
    assert guarded.applied_steps() == 1 and d["skip"] == 1 and d["skipped"] == 1 and d["t_applied"] == 1
    assert d["nonfinite"] > 0 and d["loss_nonfinite"] > 0 and guarded.step_count == 2
    # the running statistics did move during the step: the restore is what put them back
    plain.prioritized_step(rp, B, seed=7)
    assert any(not _same(a, b) for a, b in zip(before[3:], _running(plain)))
    assert torch.isnan(plain.P).sum() > 1 and torch.isnan(rp._q).any()
    # repaired: the next step applies
    guarded.P[off] = good
    guarded.prioritized_step(rg, B, seed=7)
    d = guarded.guard_stats()
    assert guarded.applied_steps() == 2 and d["skip"] == 0 and d["skipped"] == 1 and d["nonfinite"] == 0
    assert torch.isfinite(guarded.P).all() and not _same(before[0], guarded.P)
    touched = torch.zeros(len(rg), dtype=torch.bool)
    touched[guarded.last_slots.long().cpu()] = True
    q1 = rg._q.cpu()
    assert torch.equal(q1[~touched], q0.cpu()[~touched]) and not torch.equal(q1[touched], q0.cpu()[touched])
    assert torch.isfinite(q1).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_captured_schedule_replays_without_the_host(dtype):
    """lr_schedule ("exp", 0.5, 2): three bare replays of the captured prioritized step (graph.replay() and nothing
    else) against three eager guarded steps of a twin, bit for bit; the block's lr is lr_at(t)."""
    G = _G()
    sched = ("exp", 0.5, 2)
    a, b = _learner(dtype, G.StepGuard(lr_schedule=sched)), _learner(dtype, G.StepGuard(lr_schedule=sched))
    ra, rb = _ring(), _ring()
    a.prioritized_step(ra, B, seed=7)
    b.prioritized_step(rb, B, seed=7)
    a.capture(ra, B, prioritized=True, seed=7)
    for _ in range(3):
        a._graph.replay()
        b.prioritized_step(rb, B, seed=7)
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(_state(a), _state(b))):
        assert _same(x, y), i
    assert torch.equal(a.guard_block, b.guard_block) and _same(ra._q, rb._q)
    assert int(a._g_step.item()) == b.per_step == 4
    d = a.guard_stats()
    assert d["t_applied"] == 4 and _ulps(d["lr"], G.lr_at(LR, sched, 4)) <= 1
    assert abs(d["lr"] / LR - 0.5 ** 1.5) < 1e-6
    for i, (x, y) in enumerate(zip(d["adam_scalars"], G.adam_scalars_at(4, LR, sched))):
        assert _ulps(x, y) <= 1, i


def test_optimizer_state_round_trip_after_a_skipped_step():
    G = _G()
    ring = _ring()
    lrn = _learner("f32", G.StepGuard())
    lrn.train_minibatch(ring, _slots(0))
    off = lrn.params[POISON].off
    good = lrn.P[off].clone()
    lrn.P[off] = float("nan")
    lrn.train_minibatch(ring, _slots(1))
    lrn.P[off] = good
    assert lrn.step_count == 2 and lrn.applied_steps() == 1 and lrn.guard_stats()["skipped"] == 1
    osd, sd = lrn.optimizer_state_dict(), lrn.state_dict()
    assert float(osd["state"][0]["step"]) == 1.0 and osd["param_groups"][0]["lr"] == LR
    twin = _learner("f32", G.StepGuard(), seed=9)
    twin.load_state_dict(sd)
    assert twin.applied_steps() == 0
    twin.load_optimizer_state_dict(osd)
    assert twin.applied_steps() == 1 and _same(twin.M1, lrn.M1) and _same(twin.M2, lrn.M2)
    la, lb = lrn.train_minibatch(ring, _slots(2)), twin.train_minibatch(ring, _slots(2))
    d = twin.guard_stats()
    assert d["t_applied"] == 2 and _same(la, lb) and _same(twin.P, lrn.P)
    for i, (x, y) in enumerate(zip(d["adam_scalars"], G.adam_scalars_at(2, LR))):
        assert np.float32(x) == np.float32(y), i


def test_snapshot_table_follows_load_state_dict():
    """load_state_dict replaces the running-statistics tensors: the next guarded minibatch snapshots and restores the
    new ones (the pointer table is rebuilt, as RefreshTable.stale())."""
    G = _G()
    ring = _ring()
    lrn = _learner("f32", G.StepGuard())
    lrn.train_minibatch(ring, _slots(0))
    old = [t for k in lrn.bn_keys for t in lrn.run[k]]  # the tensors themselves, kept alive
    lrn.load_state_dict(lrn.state_dict())
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip([t for k in lrn.bn_keys for t in lrn.run[k]], old))
    lrn.P[lrn.params[POISON].off] = float("nan")
    before = _state(lrn)
    lrn.train_minibatch(ring, _slots(1))
    assert lrn.guard_stats()["skip"] == 1 and lrn.applied_steps() == 0
    for i, (a, b) in enumerate(zip(before, _state(lrn))):
        assert _same(a, b), i


def test_guard_needs_one_run_per_net():
    """The segment bounds come from the key prefixes; a layout that splits a net is refused."""
    from collections import OrderedDict
    G = _G()
    lrn = _learner("f32", G.StepGuard())
    assert lrn.guard_bounds[0] == 0 and lrn.guard_bounds[-1] == lrn.n_flat
    assert lrn.guard_bounds == sorted(lrn.guard_bounds) and len(lrn.guard_bounds) == 4
    keys = list(lrn.params)
    keys.append(keys.pop(0))  # the first rep_net parameter after pred_net's
    lrn.params = OrderedDict((k, lrn.params[k]) for k in keys)
    with pytest.raises(ValueError):
        lrn._guard_init()
