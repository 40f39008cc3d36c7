"""Prioritized replay on the device (csrc/replay_prio.hip, mzba_learner_loss_w, DeviceReplayBuffer / Learner):
the sampler against the f64 / longdouble restatement of tests/per_reference.py, the priority arithmetic and the
weighted loss against f64 evaluations, and the Python layer end to end.

Bounds. A sampled slot i of sample j is accepted iff C[i-1] - tol <= t_j <= C[i] + tol with tol = (cap + 8) 2^-52 S
(C, t_j in longdouble): any order of f64 summation over cap terms, plus the two roundings of t_j. f32 outputs follow
the idiom of tests/test_gpu_learner_ops.py, e_k <= 4 e_w + c 2^-24 S against an f32 torch-CPU witness, with c counted
from the kernel and stated at each test. Every test prints its e_k and e_w (pytest -s).
"""
import os

import numpy as np
import pytest
import torch

import per_reference as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SMIN, SMAX = -5.0, 5.0


def _lib():
    from mzba import _lib as L
    return L


def _check(name, got, ref, wit, cS):
    """e_k <= 4 e_w + 2^-24 cS, element by element; prints e_k and e_w."""
    got, ref, wit = got.detach().cpu().double(), ref.detach().double(), wit.detach().double()
    assert got.shape == ref.shape == wit.shape, (name, got.shape, ref.shape, wit.shape)
    assert torch.isfinite(got).all(), name
    e = (got - ref).abs()
    e_w = (wit - ref).abs().max().item() if ref.numel() else 0.0
    bound = torch.zeros_like(ref) + 4.0 * e_w + U * cS
    e_k = e.max().item() if ref.numel() else 0.0
    print(f"{name}: e_k {e_k:.3e} e_w {e_w:.3e}")
    over = (e - bound).flatten()
    i = int(over.argmax())
    assert over[i] <= 0, (name, "err", e.flatten()[i].item(), "bound", bound.flatten()[i].item(), "e_w", e_w, "at", i)


def _t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ====================================================================== the sampler
def _random_q(cap, seed):
    g = np.random.default_rng(seed)
    return np.exp(g.uniform(np.log(1e-3), np.log(1e3), cap)).astype(np.float32)


def _make_q(cap, kind):
    """f32[cap] priorities in slot space. random: log-uniform over 1e-3 ... 1e3; equal: all 0.37; wrap: the 40 % of
    the ring that is live wraps its end (start > 0), dead slots in the middle; middle: the live run lies inside, so
    the ring begins and ends with runs of zeros; single: one live slot, the last (cap > 1024: in the block whose tail
    is loaded element by element); holes: random with single dead slots, a dead 16-slot lane and a dead 1024-slot
    block inside."""
    q = _random_q(cap, cap + 17)
    if kind == "equal":
        q[:] = np.float32(0.37)
    elif kind == "wrap":
        live = cap * 2 // 5
        q[live // 2:cap - (live - live // 2)] = 0.0
    elif kind == "middle":
        q[:cap * 3 // 10] = 0.0
        q[cap * 7 // 10:] = 0.0
    elif kind == "single":
        q[:] = 0.0
        q[cap - 1] = np.float32(2.5)
    elif kind == "holes":
        q[np.random.default_rng(3).random(cap) < 0.3] = 0.0
        q[32:48] = 0.0
        q[1024:2048] = 0.0
    else:
        assert kind == "random"
    return q


def _run_sampler(q_dev, n, beta, n_live, seed=0, step=0, step_dev=None, u=None):
    L = _lib()
    cap = q_dev.numel()
    slots = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    prob = torch.full((n,), float("nan"), device="cuda")
    weight = torch.full((n,), float("nan"), device="cuda")
    ws = torch.empty(L.lib().mzba_replay_sample_ws_bytes(cap, n), dtype=torch.uint8, device="cuda")
    L.call("mzba_replay_sample", L.ptr(q_dev), cap, n, beta, n_live, seed, step, L.ptr(step_dev), L.ptr(u),
           L.ptr(slots), L.ptr(prob), L.ptr(weight), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return slots.cpu(), prob.cpu(), weight.cpu()


def _accept(tag, q, n, beta, n_live, u, slots, prob, weight):
    """Every sample of the call: a live slot inside the acceptance interval; prob and weight at the returned slots.

    prob = f32(f64(q_i) / S): the f64 sum and quotient are exact to 2^-53 relative, one f32 rounding: c = 2 on q_i / S.
    weight = f32(raw / max raw), raw = pow(n_live prob, -beta) in f64: one f32 rounding, c = 2 on the weight."""
    cap = len(q)
    C = R.prefix(q)
    S = C[-1]
    t = R.targets(q, n, u)
    tol = np.longdouble(cap + 8) * np.longdouble(2.0) ** -52 * S
    i = slots.numpy().astype(np.int64)
    assert ((i >= 0) & (i < cap)).all(), tag
    assert (q[i] > 0).all(), (tag, "a slot with q == 0 was returned")
    lo = np.where(i > 0, C[np.maximum(i - 1, 0)], np.longdouble(0))
    bad = ~((lo - tol <= t) & (t <= C[i] + tol))
    assert not bad.any(), (tag, "sample", int(np.nonzero(bad)[0][0]), "of", n)
    p_ref = (q[i].astype(np.longdouble) / S).astype(np.float64)
    qt = torch.from_numpy(q)
    p_wit = qt[i] / qt.sum()
    _check(tag + " prob", prob, _t64(p_ref), p_wit, 2 * _t64(p_ref))
    raw = (np.float64(n_live) * p_ref) ** (-np.float64(np.float32(beta)))
    w_ref = raw / raw.max()
    raw_w = (float(n_live) * p_wit) ** (-beta)
    _check(tag + " weight", weight, _t64(w_ref), raw_w / raw_w.max(), 2 * _t64(w_ref))
    assert (weight > 0).all() and (weight <= 1).all() and weight.max() == 1.0, tag


SAMPLER_CASES = [(cap, kind) for cap in (1, 63, 1023, 1024, 1025, 3000) for kind in ("random", "equal")] + \
    [(3000, "wrap"), (3000, "middle"), (3000, "single"), (1025, "single"), (3000, "holes")]


@pytest.mark.parametrize("cap,kind", SAMPLER_CASES)
def test_sampler(cap, kind):
    """mzba_replay_sample at n = 1, 7 and 512, with the Philox draws (oracle.rng.uniform(j, 4, step, 0, seed)) and
    with injected draws of all 0.0 and all 1 - 2^-24: every sample accepted, no dead slot, prob and weight within
    their bounds; a second call with equal arguments and a call that reads the step from the device give the same
    bits; beta = 0 gives weights of exactly 1."""
    q = _make_q(cap, kind)
    qd = torch.from_numpy(q).cuda()
    n_live = int((q > 0).sum())
    seed, step, beta = 1234567 + cap, 41, 0.6
    for n in (1, 7, 512):
        tag = f"sampler cap {cap} {kind} n {n}"
        out = _run_sampler(qd, n, beta, n_live, seed, step)
        _accept(tag + " philox", q, n, beta, n_live, R.draws(n, step, seed), *out)
        again = _run_sampler(qd, n, beta, n_live, seed, step)
        sdev = torch.tensor([step], dtype=torch.int32, device="cuda")
        from_dev = _run_sampler(qd, n, beta, n_live, seed, step + 1000, step_dev=sdev)  # step_dev overrides step
        for a, b, c in zip(out, again, from_dev):
            assert torch.equal(a, b) and torch.equal(a, c), tag
        for name, val in (("u=0", 0.0), ("u=1-2^-24", 1.0 - 2.0 ** -24)):
            u = torch.full((n,), val, dtype=torch.float32)
            assert float(u[0]) == val
            got = _run_sampler(qd, n, beta, n_live, seed, step, u=u.cuda())
            _accept(f"{tag} {name}", q, n, beta, n_live, u.numpy(), *got)
        s0, p0, w0 = _run_sampler(qd, n, 0.0, n_live, seed, step)
        assert torch.equal(s0, out[0]) and torch.equal(p0, out[1]) and (w0 == 1.0).all(), tag
        if n > 1 and kind == "random" and cap > 1:
            other = _run_sampler(qd, n, beta, n_live, seed, step + 1)
            assert not torch.equal(other[0], out[0]) or cap < 64, (tag, "another step drew the same slots")


def test_sampler_rejects_an_empty_buffer():
    """n_live = 0 (S == 0) is an argument error, not a launch; so are a short workspace and cap > 2^20."""
    L = _lib()
    q = torch.zeros(64, device="cuda")
    o = torch.zeros(8, device="cuda")
    oi = torch.zeros(8, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.lib().mzba_replay_sample_ws_bytes(64, 8), dtype=torch.uint8, device="cuda")
    f = L.lib().mzba_replay_sample
    args = lambda cap, n_live, nbytes: (L.ptr(q), cap, 8, 1.0, n_live, 0, 0, None, None, L.ptr(oi), L.ptr(o),  # noqa: E731
                                        L.ptr(o), L.ptr(ws), nbytes, L.stream())
    assert f(*args(64, 0, ws.numel())) == -3
    assert f(*args(64, 64, ws.numel() - 1)) == -2
    assert f(*args((1 << 20) + 1, 64, ws.numel())) == -1


# ====================================================================== priorities
def _fixture_trajectories():
    from replay_buffer import ObservationTrajectory
    d = np.load(os.path.join(GOLDEN, "replay.npz"))
    h = int(d["hist"])
    out = []
    for i, Lr in enumerate(d["lengths"]):
        f0 = torch.from_numpy(d["frame0"][i].reshape(1, 16, 20))
        t = ObservationTrajectory([0] * h, [f0] * (h - 1), [0] * h, [torch.zeros(3)] * h, [0.0] * h, 0, 0)
        for s in range(Lr):
            t.add_observation(int(d["actions"][i, s]), torch.from_numpy(d["frames"][i, s].reshape(1, 16, 20)),
                              float(d["rewards"][i, s]), torch.from_numpy(d["counts"][i, s]), float(d["values"][i, s]))
        out.append(t)
    return d, out


def _fixture_buffer(max_length, **kw):
    from mzba.replay import DeviceReplayBuffer
    d, trajs = _fixture_trajectories()
    buf = DeviceReplayBuffer(int(d["hist"]), int(d["K"]), max_length, float(d["discount"]),
                             int(d["num_rewards_to_sum"]), **kw)
    return buf, trajs


def _ingest_rule(buf, alpha, eps):
    """(|searched value - n-step target| at the root step + eps) ** alpha from the device getters: f64 and f32."""
    idx = torch.arange(len(buf))
    v, z = buf.get_values(idx)[:, 0].cpu(), buf.get_batched_values(idx)[:, 0].cpu()
    ref = _t64(R.priority((v.double() - z.double()).abs().numpy(), eps, alpha))
    wit = ((v - z).abs() + eps) ** alpha
    return ref, wit


@pytest.mark.parametrize("alpha", [1.0, 0.6])
@pytest.mark.parametrize("max_length", [100000, 60])
def test_ingest_sets_priorities(max_length, alpha):
    """save_observation_trajectory on the host trajectories of tests/golden/replay.npz (74 windows; 60 evicts): after
    every trajectory priorities() follows the ingest rule, every slot without a window holds exactly 0, and
    empty_buffer() zeroes everything.

    Chain: v - z, + eps (f32), pow in double, one rounding to f32: c = 4 on q (alpha <= 1 does not amplify)."""
    eps = 1e-3
    buf, trajs = _fixture_buffer(max_length, prioritized=True, alpha=alpha, prio_eps=eps)
    assert buf._q.shape == (max_length,) and not buf._q.any() and "q" not in buf._ring
    total = 0
    for t in trajs:
        buf.save_observation_trajectory(t)
        total += max(t.length - buf.K + 1, 0) if t.length >= buf.K else 0
        assert len(buf) == min(total, max_length)
        if len(buf) == 0:
            continue
        ref, wit = _ingest_rule(buf, alpha, eps)
        pri = buf.priorities()
        assert pri.dtype == torch.float32 and pri.shape == (len(buf),)
        _check(f"ingest cap {max_length} alpha {alpha} at {len(buf)}", pri, ref, wit, 4 * ref)
        assert (pri > 0).all()
        live = (torch.arange(len(buf), device="cuda") + buf.start) % max_length
        dead = torch.ones(max_length, dtype=torch.bool, device="cuda")
        dead[live] = False
        assert dead.sum().item() == max_length - len(buf) and not buf._q[dead].any()
    assert total == 74 and (len(buf) == 60) == (max_length == 60) and (buf.start > 0) == (max_length == 60)
    buf.empty_buffer()
    assert len(buf) == 0 and not buf._q.any()


@pytest.mark.parametrize("alpha", [1.0, 0.6])
def test_priority_update(alpha):
    """mzba_replay_priority_update over n = 512 slots of a 3000-slot ring, duplicates carrying equal td: q[slot] =
    (td + eps) ** alpha at the touched slots (c = 3: the f32 add, the pow in double, the rounding), every other slot
    bit-equal."""
    L = _lib()
    cap, n, eps = 3000, 512, 1e-3
    g = torch.Generator().manual_seed(5)
    q0 = torch.rand(cap, generator=g) + 0.1
    table = torch.rand(cap, generator=g) * 4.0
    table[::7] = 0.0  # a perfect prediction: the priority is eps ** alpha
    slots = torch.randint(0, cap, (n,), generator=g).to(torch.int32)
    assert slots.unique().numel() < n, "the case needs duplicates"
    td = table[slots.long()]
    q, slots_d, td_d = q0.clone().cuda(), slots.cuda(), td.cuda()
    L.call("mzba_replay_priority_update", L.ptr(q), L.ptr(slots_d), L.ptr(td_d), n, cap, alpha, eps, L.stream())
    torch.cuda.synchronize()
    # a slot outside [0, cap) is skipped, not written
    wild = torch.tensor([-1, cap, 2 ** 30, 5], dtype=torch.int32, device="cuda")
    q2, td2 = q0.clone().cuda(), torch.ones(4, device="cuda")
    L.call("mzba_replay_priority_update", L.ptr(q2), L.ptr(wild), L.ptr(td2), 4, cap, 1.0, 0.0, L.stream())
    torch.cuda.synchronize()
    assert q2[5].item() == 1.0 and torch.equal(q2.cpu()[torch.arange(cap) != 5], q0[torch.arange(cap) != 5])
    touched = torch.zeros(cap, dtype=torch.bool)
    touched[slots.long()] = True
    assert torch.equal(q.cpu()[~touched], q0[~touched])
    ref = _t64(R.priority(table.double().numpy(), eps, alpha))
    wit = (table + eps) ** alpha
    _check(f"priority_update alpha {alpha}", q.cpu()[touched], ref[touched], wit[touched], 3 * ref[touched])


def test_prioritized_api_is_opt_in():
    """A buffer built with prioritized=False has no priority array, raises from the three calls, and lists exactly
    the reference's checkpoint keys."""
    from mzba.checkpoint import REPLAY_KEYS
    buf, trajs = _fixture_buffer(100)
    buf.save_observation_trajectory(trajs[1])
    assert buf._q is None and len(buf) > 0
    for call in (lambda: buf.sample(4, 0), lambda: buf.priorities(),
                 lambda: buf.update_priorities(torch.zeros(1, dtype=torch.int32, device="cuda"),
                                               torch.zeros(1, device="cuda"))):
        with pytest.raises(RuntimeError):
            call()
    assert set(buf.to_reference_lists()) == set(REPLAY_KEYS)
    pb, _ = _fixture_buffer(100, prioritized=True)
    with pytest.raises(ValueError):
        pb.sample(4, 0)  # empty


def test_checkpoint_round_trip(tmp_path):
    """to_reference_lists() / load_reference_lists through torch.save and torch.load(weights_only=True): with the
    "priorities" entry the learned priorities come back bit for bit; without it the ingest rule is applied; the
    reference-format entries are those of a non-prioritized buffer either way."""
    from mzba.checkpoint import REPLAY_KEYS
    kw = dict(prioritized=True, alpha=0.6, prio_eps=1e-3)
    buf, trajs = _fixture_buffer(60, **kw)
    plain, _ = _fixture_buffer(60)
    for t in trajs:
        buf.save_observation_trajectory(t)
        plain.save_observation_trajectory(t)
    at_ingest = buf.priorities().clone()
    slots, _, _ = buf.sample(16, step=0, seed=3)
    buf.update_priorities(slots, torch.linspace(0.0, 3.0, 16, device="cuda")[slots.long() % 16])
    learned = buf.priorities().clone()
    assert not torch.equal(learned, at_ingest)
    d = buf.to_reference_lists()
    assert set(d) == set(REPLAY_KEYS) | {"priorities"}
    dp = plain.to_reference_lists()
    for k in REPLAY_KEYS:
        a, b = d[k], dp[k]
        same = all(torch.equal(torch.as_tensor(x), torch.as_tensor(y)) for x, y in zip(a, b)) and len(a) == len(b) \
            if isinstance(a, list) else a == b
        assert same, k
    p = str(tmp_path / "replay.pth")
    torch.save(d, p)
    back = torch.load(p, weights_only=True)
    b2, _ = _fixture_buffer(60, **kw)
    b2.load_reference_lists(back)
    assert len(b2) == len(buf) and torch.equal(b2.priorities(), learned)
    idx = torch.arange(len(buf))
    assert torch.equal(b2.get_batched_values(idx), buf.get_batched_values(idx))
    del back["priorities"]
    b3, _ = _fixture_buffer(97, **kw)  # a larger ring: the slots past the loaded windows stay 0
    b3.load_reference_lists(back)
    assert torch.equal(b3.priorities(), at_ingest) and not b3._q[len(b3):].any()
    b4, _ = _fixture_buffer(60)
    b4.load_reference_lists(d)  # a non-prioritized buffer reads a prioritized checkpoint: the entry is ignored
    assert b4._q is None and len(b4) == len(buf)


# ====================================================================== the weighted loss
def _compact64(x):
    return np.sign(x) * (np.sqrt(np.abs(x) + 1.0) - 1.0 + 0.001 * x)


def _weighted_loss(lr, lv, lp, rw, tg, ct, w, K, ns, na, tdt):
    """loss_fn with row (b, k)'s KL terms times w[b], in dtype tdt (two-hot targets from oracle.learner's
    supports_representation); gradients by autograd of the total. -> (total, r, v, p), grads, targets."""
    from oracle.learner import supports_representation
    z = [t.detach().to(tdt).clone().requires_grad_() for t in (lr, lv, lp)]
    tr = supports_representation(rw.to(tdt), SMIN, SMAX, ns)
    tv = supports_representation(tg.to(tdt), SMIN, SMAX, ns)
    c = ct.to(tdt)
    tp = c / c.sum(-1, keepdim=True)
    B = rw.shape[0]
    parts = []
    for zz, tt in zip(z, (tr, tv, tp)):
        logp = torch.log_softmax(zz.permute(1, 0, 2), -1)
        kl = torch.where(tt > 0, tt * (tt.clamp_min(1e-30).log() - logp), torch.zeros_like(logp)).sum(-1)  # [B][K]
        parts.append((kl * w.to(tdt)[:, None]).sum() / (B * K))
    total = (1 / K) * (parts[0] + parts[1] + parts[2])
    total.backward()
    return torch.stack([total] + parts).detach(), [zz.grad for zz in z], (tr, tv, tp)


def _loss_bounds(z, t, comp, K, step, w):
    """c S of one head's weighted mean KL and of its logit gradients (tests/test_gpu_learner_ops.py's _loss_bounds
    with one more operation, the multiply by w[b] <= 1, and every row's terms scaled by w[b]). kl_row: max, n
    exp-adds, log, and per entry two subtracts, log t, a subtract and a multiply: c = n + 11 on sum t (|ln t| +
    |logp|) + max |logp|. A two-hot target carries the f32 transform's and supports' rounding, dt = 12 2^-24
    (|compact| + 1) / step, which moves t ln t by up to dt (1 + |ln dt| + max |logp|) per entry. Gradient entry:
    (n + 11) 2^-24 (1 + |z - max| + |log sum|) softmax + dt + 3 2^-24 (softmax + t), times w / (K B K)."""
    n = z.shape[-1]
    zz = z.permute(1, 0, 2)
    lp = torch.log_softmax(zz, -1)
    soft = lp.exp()
    tl = torch.where(t > 0, t * t.clamp_min(1e-300).log().abs(), torch.zeros_like(t))
    lpmax = lp.abs().max(-1)[0]
    c = n + 11 + (0 if comp is not None else n + 1)
    row = c * ((tl + t * lp.abs()).sum(-1) + lpmax)
    if comp is not None:
        dt = 12 * U * (comp.abs() + 1) / step
        row = row + 2 * dt * (1 + dt.log().abs() + lpmax) / U
        dte = (dt / U).unsqueeze(-1).expand_as(t)
    else:
        dte = (n + 1) * t
    zmax = zz.max(-1, keepdim=True)[0]
    ls = (zz - zmax).exp().sum(-1, keepdim=True).log().abs()
    gr = (c * (1 + (zz - zmax).abs() + ls) * soft + dte + 3 * (soft + t)) / (K * zz.shape[0] * K)
    wd = w.double()
    return (row * wd[:, None]).mean(), (gr * wd[:, None, None]).permute(1, 0, 2)


@pytest.mark.parametrize("B,K", [(3, 2), (64, 5), (512, 5)])
def test_weighted_loss(B, K):
    """mzba_learner_loss_w on gathered slots. weights NULL and weights all 1.0f: loss and the three gradients are the
    bits of mzba_learner_loss_ws. Random weights in (0, 1]: loss, gradients and td against f64.

    td[b] = |decode(logit_v[0][b]) - target[slot][0]|. decode_support: x = sum softmax_i sup_i carries (n + 8 + max
    |z - max|) roundings of max |sup| (the exp argument's rounding is a relative error |z - max| 2^-24 of that term;
    n adds, a divide, a multiply per term, the supports' own rounding), amplified by d/dx (|x| + 0.999)^2 = 2 t; then
    + 0.999, the square, - 1, - target: 4 roundings of t^2 + 1 + |target|."""
    from oracle.nets import inverted_softmax_expectation
    L = _lib()
    ns, na = 11, 3
    g = torch.Generator().manual_seed(100 * B + K)
    cap = B + 4
    slots = torch.randperm(cap, generator=g)[:B].to(torch.int32)
    sel = slots.long()
    lr, lv = torch.randn(K, B, ns, generator=g) * 3, torch.randn(K, B, ns, generator=g) * 3
    lp = torch.randn(K, B, na, generator=g)
    rewards = torch.randint(-1, 2, (cap, K), generator=g).float()
    targets = torch.randn(cap, K, generator=g) * 4
    targets[sel[0], 0] = 0.0
    counts = torch.randint(0, 51, (cap, K, na), generator=g).float()
    counts[..., 0] += 1
    w = 1.0 - torch.rand(B, generator=g)  # (0, 1]
    w[0] = 1.0
    assert (w > 0).all() and (w <= 1).all()
    dev = [t.cuda() for t in (lr, lv, lp, rewards, targets, counts)]
    sd = slots.cuda()
    ws = torch.empty(L.lib().mzba_learner_loss_ws_bytes(B, K), dtype=torch.uint8, device="cuda")

    def run(entry, *extra):
        d = [torch.full_like(t, float("nan")) for t in dev[:3]]
        loss = torch.full((4,), float("nan"), device="cuda")
        L.call(entry, *[L.ptr(t) for t in dev], L.ptr(sd), B, K, ns, na, SMIN, SMAX, *[L.ptr(t) for t in d],
               L.ptr(loss), L.ptr(ws), ws.numel(), *extra, L.stream())
        torch.cuda.synchronize()
        return [loss] + d

    plain = run("mzba_learner_loss_ws")
    td1 = torch.full((B,), float("nan"), device="cuda")
    ones = torch.ones(B, device="cuda")
    for name, got in (("NULL", run("mzba_learner_loss_w", None, None)),
                      ("ones", run("mzba_learner_loss_w", L.ptr(ones), L.ptr(td1)))):
        for a, b in zip(plain, got):
            assert torch.equal(a, b), (name, B, K)
    rw, tg, ct = rewards[sel], targets[sel], counts[sel]
    ref, rgrad, tt = _weighted_loss(lr, lv, lp, rw, tg, ct, w, K, ns, na, torch.float64)
    wit, wgrad, _ = _weighted_loss(lr, lv, lp, rw, tg, ct, w, K, ns, na, torch.float32)
    step = (SMAX - SMIN) / (ns - 1)
    comps = (torch.from_numpy(_compact64(rw.double().numpy())), torch.from_numpy(_compact64(tg.double().numpy())), None)
    rows, gbs = zip(*[_loss_bounds(z.double(), t, c, K, step, w) for z, t, c in zip((lr, lv, lp), tt, comps)])
    cs_parts = [r + 2 * p.abs() for r, p in zip(rows, ref[1:])]
    cs_loss = torch.stack([(1 / K) * sum(cs_parts) + 3 * ref[0].abs()] + cs_parts)
    td = torch.full((B,), float("nan"), device="cuda")
    w_d = w.cuda()
    got = run("mzba_learner_loss_w", L.ptr(w_d), L.ptr(td))
    tag = f"loss_w B {B} K {K}"
    _check(tag + " loss", got[0], ref, wit, cs_loss)
    for name, a, r, w_, c in zip(("dlogit_r", "dlogit_v", "dlogit_p"), got[1:], rgrad, wgrad, gbs):
        _check(f"{tag} {name}", a, r, w_, c)
    assert torch.equal(td, td1), "td does not depend on the weights"
    z0 = lv[0].double().numpy()
    dec = inverted_softmax_expectation(z0, SMIN, SMAX)
    td_ref = np.abs(dec - tg[:, 0].double().numpy())
    td_wit = np.abs(inverted_softmax_expectation(lv[0].numpy(), SMIN, SMAX) - tg[:, 0].numpy())
    soft = torch.softmax(lv[0].double(), -1)
    x = (soft * torch.linspace(SMIN, SMAX, ns, dtype=torch.float64)).sum(-1)
    t_ = x.abs() + 0.999
    spread = (lv[0].double().max(-1)[0] - lv[0].double().min(-1)[0])
    cs_td = (ns + 8 + spread) * max(abs(SMIN), abs(SMAX)) * 2 * t_ + 4 * (t_ * t_ + 1 + tg[:, 0].double().abs())
    _check(tag + " td", td, _t64(td_ref), torch.from_numpy(np.asarray(td_wit, np.float32)), cs_td)


# ====================================================================== the learner, end to end
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


def _per_ring(n=64, seed=4, **kw):
    """A DeviceReplayBuffer(prioritized=True) of n explicit windows (the rows of a MinibatchRing), priorities by
    the ingest rule."""
    from mzba.learner import MinibatchRing
    from mzba.replay import DeviceReplayBuffer
    mb, values = _minibatch_arrays(n, seed)
    src = MinibatchRing(mb)
    kw = {**dict(prioritized=True, alpha=0.6, beta=0.4, prio_eps=1e-3), **kw}
    buf = DeviceReplayBuffer(4, 5, n, 0.997, 8, **kw)
    for k, t in src._ring.items():
        buf._ring[k].copy_(t)
    buf._ring["values"].copy_(torch.from_numpy(values))
    buf.start, buf.length = 0, n
    if buf.prioritized:
        buf._init_priorities(0, n)
    return buf


def _learner(seed=6):
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    lm = learner_model_cfg()
    return Learner(lm, init_state_dict(lm, seed), K=5)


def test_unit_weights_leave_the_minibatch_unchanged():
    """train_minibatch(weights=ones) leaves the parameters and the loss bit-equal to train_minibatch() from the
    same start, and leaves last_td."""
    ring = _per_ring()
    slots = torch.arange(3, 19, dtype=torch.int32, device="cuda")
    a, b = _learner(), _learner()
    la = a.train_minibatch(ring, slots)
    lb = b.train_minibatch(ring, slots, weights=torch.ones(16, device="cuda"))
    assert torch.equal(la, lb) and torch.equal(a.P, b.P)
    assert a.last_td is None and b.last_td.shape == (16,) and torch.isfinite(b.last_td).all()
    half = b.train_minibatch(ring, slots, weights=torch.full((16,), 0.5, device="cuda"))
    assert not torch.equal(half, a.train_minibatch(ring, slots))


def test_captured_prioritized_step_equals_eager():
    """Three eager prioritized steps and three replays of capture(..., prioritized=True), each after one eager
    step from the same start: slots, weights, losses, parameters and final priorities bit for bit. After each eager
    step exactly the sampled slots' priorities are (last_td + eps) ** alpha (c = 3, as test_priority_update)."""
    B = 16
    runs = []
    for captured in (False, True):
        ring, lrn = _per_ring(), _learner()
        lrn.prioritized_step(ring, B, seed=7)
        if captured:
            lrn.capture(ring, B, prioritized=True, seed=7)
        rec = []
        for _ in range(3):
            before = ring._q.clone()
            loss = lrn.prioritized_step(ring, B, seed=7)
            rec.append((lrn.last_slots.clone(), lrn.last_weights.clone(), loss.clone()))
            touched = torch.zeros(len(ring), dtype=torch.bool)
            touched[lrn.last_slots.long().cpu()] = True
            after = ring._q.cpu()
            assert torch.equal(after[~touched], before.cpu()[~touched])
            s = lrn.last_slots.long().cpu()
            td = lrn.last_td.cpu()
            ref = _t64(R.priority(td.double().numpy(), ring.prio_eps, ring.alpha))
            _check(f"step priorities captured {captured}", after[s], ref, (td + ring.prio_eps) ** ring.alpha, 3 * ref)
        assert lrn.per_step == 4 and lrn.step_count == 4
        runs.append((rec, lrn.P.clone(), ring.priorities().clone()))
    (ra, pa, qa), (rb, pb, qb) = runs
    for i, (x, y) in enumerate(zip(ra, rb)):
        for name, u, v in zip(("slots", "weights", "loss"), x, y):
            assert torch.equal(u, v), (i, name)
    assert torch.equal(pa, pb) and torch.equal(qa, qb)
    assert len({tuple(r[0].tolist()) for r in ra}) == 3, "every step draws afresh"


def test_training_stage_uniform_path_is_untouched():
    """training_stage(prioritized=False) on a fixed generator: the losses of a hand-written randperm loop over
    train_minibatch (the parent's loop), on a prioritized ring whose priorities it leaves alone. prioritized=True:
    the losses of the same number of prioritized_step()s."""
    ring = _per_ring()
    q0 = ring._q.clone()
    a, b = _learner(), _learner()
    got = a.training_stage(ring, 3, 16, generator=torch.Generator().manual_seed(12))
    perm = torch.randperm(len(ring), generator=torch.Generator().manual_seed(12))
    want = []
    for i in range(3):
        slots = (perm[i * 16:(i + 1) * 16].to("cuda") + ring.start) % ring.max_length
        want.append(float(b.train_minibatch(ring, slots)[0]))
    assert got == want and len(got) == 3 and torch.equal(a.P, b.P)
    assert torch.equal(ring._q, q0) and a.per_step == 0
    ring2 = _per_ring()
    got_p = a.training_stage(ring, 2, 16, prioritized=True, seed=5)
    want_p = [float(b.prioritized_step(ring2, 16, seed=5)[0]) for _ in range(2)]
    assert got_p == want_p and torch.equal(a.P, b.P) and torch.equal(ring._q, ring2._q)
    assert not torch.equal(ring._q, q0)
