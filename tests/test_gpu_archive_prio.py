"""Prioritized replay over the sink archive on the GPU (csrc/archive_prio.hip, mzba.archive.SinkArchive(prioritized=True);
DESIGN.md §19), against the numpy restatement of tests/archive_prio_cases.py.

Bounds. A sampled row i of sample j is accepted iff q[i] > 0 and C[i-1] - tol <= t_j <= C[i] + tol with tol = (n_rows +
8) 2^-52 S (C, t_j in longdouble): any order of f64 summation over n_rows terms plus the roundings of t_j; prob and
weight are held to test_gpu_per._accept's bounds (that function is the one called). With q in {0, 1} every partial sum
is an exact integer, so the rows are compared exactly. Priorities at alpha = 1 are compared bit for bit, at alpha = 0.6
within test_ingest_sets_priorities' bound (c = 4 on q).
"""
import ctypes

import numpy as np
import pytest
import torch

import archive_cases as AC
import archive_prio_cases as APC
import per_reference as PR
import stream_cases as SC
from stream_cases import K, HIST, DISCOUNT
from test_gpu_archive import _by_slab, _bytes, _dev, _i32, _is_poison, _one_stage, _poison
from test_gpu_per import _accept, _check, _t64

pytestmark = pytest.mark.gpu

EPS = 1e-3
U_TOP = 1.0 - 2.0 ** -53


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def _L():
    from mzba import _lib as L
    return L


# ====================================================================== 1. the sampler alone
ROWS = [1, 1023, 1024, 1025, 3000, 2 ** 20 - 1, 2 ** 20, 2 ** 20 + 1, 2 ** 20 + 1025, 3 * 2 ** 20 + 77]
KINDS = ["random", "equal", "single", "holes"]


def _make_q(n_rows, kind):
    """f32[n_rows]. random: log-uniform over 1e-3 ... 1e3; equal: all 0.37; single: one live row, the last; holes:
    random with 30 % single dead rows, a dead 16-row lane, a dead 1024-row block and (beyond 2^20 rows) a dead
    super-block, the second."""
    g = np.random.default_rng(n_rows + 17)
    q = np.exp(g.uniform(np.log(1e-3), np.log(1e3), n_rows)).astype(np.float32)
    if kind == "equal":
        q[:] = np.float32(0.37)
    elif kind == "single":
        q[:] = 0.0
        q[n_rows - 1] = np.float32(2.5)
    elif kind == "holes":
        q[g.random(n_rows) < 0.3] = 0.0
        q[32:48] = 0.0
        q[1024:2048] = 0.0
        q[2 ** 20:2 ** 21] = 0.0
        if not q.any():
            q[0] = np.float32(1.5)
    else:
        assert kind == "random"
    return q


def _run_sampler(q_dev, n, beta, n_live, seed=0, step=0, step_dev=None, u=None):
    """The plain row sampler (no table) -> rows, prob, weight on the host."""
    L = _L()
    n_rows = q_dev.numel()
    rows = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    prob = torch.full((n,), float("nan"), device="cuda")
    weight = torch.full((n,), float("nan"), device="cuda")
    ws = torch.empty(L.lib().mzba_archive_sample_ws_bytes(n_rows, n), dtype=torch.uint8, device="cuda")
    L.call("mzba_archive_sample", L.ptr(q_dev), n_rows, n, beta, n_live, None, 0, None, None, 0, 0, seed, step,
           L.ptr(step_dev), L.ptr(u), L.ptr(rows), None, L.ptr(prob), L.ptr(weight), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return rows.cpu(), prob.cpu(), weight.cpu()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n_rows", ROWS)
def test_sampler(n_rows, kind):
    """mzba_archive_sample without a table at n = 1, 7 and 512, with the 53-bit Philox draws and with injected draws of
    all 0.0 and all 1 - 2^-53: every sample accepted, no dead row, prob and weight within their bounds; equal arguments
    and a step read from the device give equal bits; beta = 0 gives weights of exactly 1; with the same rows at
    priority 1 (q in {0, 1}) the rows are exactly the floor(t_j)-th live rows."""
    q = _make_q(n_rows, kind)
    qd = torch.from_numpy(q).cuda()
    q01 = (q > 0).astype(np.float32)
    q01d = torch.from_numpy(q01).cuda()
    n_live = int((q > 0).sum())
    if kind == "holes" and n_rows > 2 ** 20:
        assert not q[2 ** 20:2 ** 21].any() and q[:2 ** 20].any()
    seed, step, beta = 1234567 + n_rows, 41, 0.6
    for n in (1, 7, 512):
        tag = f"rows {n_rows} {kind} n {n}"
        draws = APC.draws53(n, step, seed)
        out = _run_sampler(qd, n, beta, n_live, seed, step)
        _accept(tag + " philox", q, n, beta, n_live, draws, *out)
        again = _run_sampler(qd, n, beta, n_live, seed, step)
        sdev = torch.tensor([step], dtype=torch.int32, device="cuda")
        from_dev = _run_sampler(qd, n, beta, n_live, seed, step + 1000, step_dev=sdev)  # step_dev overrides step
        for a, b, c in zip(out, again, from_dev):
            assert torch.equal(_bytes(a), _bytes(b)) and torch.equal(_bytes(a), _bytes(c)), tag
        r01 = _run_sampler(q01d, n, beta, n_live, seed, step)[0]
        assert np.array_equal(r01.numpy(), APC.live_rank_rows(q01, n, draws)), tag
        for name, val in (("u=0", 0.0), ("u=1-2^-53", U_TOP)):
            u = torch.full((n,), val, dtype=torch.float64)
            assert float(u[0]) == val and val < 1.0
            got = _run_sampler(qd, n, beta, n_live, seed, step, u=u.cuda())
            _accept(f"{tag} {name}", q, n, beta, n_live, u.numpy(), *got)
            r01 = _run_sampler(q01d, n, beta, n_live, seed, step, u=u.cuda())[0]
            assert np.array_equal(r01.numpy(), APC.live_rank_rows(q01, n, u.numpy())), (tag, name)
        r0, p0, w0 = _run_sampler(qd, n, 0.0, n_live, seed, step)
        assert torch.equal(r0, out[0]) and torch.equal(p0, out[1]) and (w0 == 1.0).all(), tag
        if n > 1 and kind == "random" and n_rows > 64:
            other = _run_sampler(qd, n, beta, n_live, seed, step + 1)
            assert not torch.equal(other[0], out[0]), (tag, "another step drew the same rows")


# ====================================================================== archives
def _archive(slabs, T, B, seq_len=HIST, **kw):
    from mzba.archive import SinkArchive
    return SinkArchive(slabs, T, B, K, seq_len, DISCOUNT, episode_cap=SC.CAP_SYN, **kw)


def _append(arc, host, stage, T):
    spec, tail, rec, done, hlen = stage
    drec, ddone, dhlen = _dev(rec, done, hlen)
    slab = arc.append(drec, T, ddone, dhlen, tail=tail)
    assert slab == host.append(rec, done, hlen, tail)
    return slab


def _mixed(n_stages, **kw):
    """The 3-slab B = 67, T = 24 mixed-tail archive after n_stages appends -> (arc, host, stages)."""
    B, T, S = 67, 24, 3
    stages = AC.mixed_stages(B, T, 100, ("keep", "drop", "keep", "drop"))
    arc, host = _archive(S, T, B, **kw), AC.HostArchive(S, T, B)
    for stage in stages[:n_stages]:
        _append(arc, host, stage, T)
    return arc, host, stages


def _one_slab(B, **kw):
    T = 24
    spec = [([(12, 12), (11, 11)], False)] if B == 1 else SC.random_spec(B, T, seed=B, empty_runs=((2, 4),))
    stage = _one_stage(spec, T, "keep", seed=B + 1)
    arc, host = _archive(1, T, B, **kw), AC.HostArchive(1, T, B)
    _append(arc, host, stage, T)
    return arc, host, stage


def _cases(**kw):
    yield ("mixed", *_mixed(3, **kw)[:2])
    for B in (1, 5, 257):
        yield (f"one slab B {B}", *_one_slab(B, **kw)[:2])


def _lookup(arc, rows):
    L = _L()
    rows = _i32(rows)
    out = torch.full((rows.numel(),), -7, dtype=torch.int32, device="cuda")
    L.call("mzba_archive_row_windows", L.ptr(arc._table), arc.nmax, L.ptr(arc._offs), L.ptr(arc._totals), arc.B, K,
           arc.T * arc.B, L.ptr(rows), rows.numel(), L.ptr(out), L.stream())
    return out.cpu().numpy().astype(np.int64)


# ====================================================================== 2. the lookup
def test_lookup_every_row():
    """mzba_archive_row_windows over every (row, env), and the rows -1, T B and 2^31 - 1, against the numpy lookup;
    an archive without a kept segment answers -1 everywhere."""
    for name, arc, host in _cases():
        segs = host.plan()
        n_rows = arc.T * arc.B
        rows = np.concatenate([np.arange(n_rows), [-1, n_rows, 2 ** 31 - 1]])
        got = _lookup(arc, rows)
        want = APC.lookup(segs, arc.B, K, n_rows, rows)
        assert np.array_equal(got, want), name
        assert (got[n_rows:] == -1).all() and (got >= 0).sum() == arc.windows == AC.windows_of(segs) > 0, name
        assert np.array_equal(arc.root_rows().cpu().numpy(), APC.root_rows(segs, arc.B, K)), name
    empty = _archive(2, 24, 9)
    assert (_lookup(empty, np.arange(-1, 2 * 24 * 9 + 1)) == -1).all()


# ====================================================================== 3. the init rule
def _gathered(arc):
    """(values[j][0], targets[j][0]) f32 on the host, of a gather of all windows."""
    N = arc.windows
    staged, _, idx_out = arc.gather(N, idx=_i32(np.arange(N)))
    assert idx_out.tolist() == list(range(N))
    return staged._ring["values"][:, 0].cpu(), staged._ring["targets"][:, 0].cpu()


def _check_init(tag, arc, segs, alpha, rows=None):
    """q at the roots against the priority formula on the gathered windows, 0.0 at every non-root; restricted to the
    sink rows [rows) where given."""
    v, z = _gathered(arc)
    roots = APC.root_rows(segs, arc.B, K)
    q = arc._q.cpu()
    sel = np.ones(len(roots), bool) if rows is None else (roots >= rows[0]) & (roots < rows[1])
    assert sel.any(), tag
    pri = q[torch.from_numpy(roots[sel])]
    v, z = v[torch.from_numpy(sel)], z[torch.from_numpy(sel)]
    wit = ((v - z).abs() + EPS) ** alpha
    if alpha == 1.0:
        assert torch.equal(_bytes(pri), _bytes((v - z).abs() + np.float32(EPS))), tag
    else:
        ref = _t64(PR.priority((v.double() - z.double()).abs().numpy(), EPS, alpha))
        _check(tag, pri, ref, wit, 4 * ref)
    assert (pri > 0).all(), tag
    dead = torch.ones(q.numel(), dtype=torch.bool)
    dead[torch.from_numpy(roots)] = False
    if rows is not None:
        dead[:rows[0]] = False
        dead[rows[1]:] = False
    assert dead.any() and not q[dead].any(), (tag, "a non-root row holds a priority")
    assert torch.equal(_bytes(arc.priorities().cpu()), _bytes(q[torch.from_numpy(roots)])), tag


@pytest.mark.parametrize("alpha", [1.0, 0.6])
def test_append_sets_priorities(alpha):
    """After the appends, q at window j's root is the priority formula on values[j][0] and targets[j][0] of a gather of
    all windows (alpha = 1 bit for bit, the numpy n-step target too), 0.0 on every non-root, and in window order
    bit-equal to the priorities of prioritized rings that ingest the same stages and evict nothing."""
    from mzba.replay import DeviceReplayBuffer
    kw = dict(prioritized=True, alpha=alpha, prio_eps=EPS)
    arc, host, stages = _mixed(3, **kw)
    cases = [("mixed", arc, host, stages[:3])]
    for B in (1, 5, 257):
        a, h, st = _one_slab(B, **kw)
        cases.append((f"one slab B {B}", a, h, [st]))
    for name, arc, host, sts in cases:
        segs = host.plan()
        T = arc.steps
        _check_init(f"init {name} alpha {alpha}", arc, segs, alpha)
        _, z = _gathered(arc)
        _, z_np = APC.init_reference(host.rec, segs, K, DISCOUNT, EPS, alpha)
        assert np.array_equal(z.numpy().view(np.uint32), z_np.view(np.uint32)), name
        pri = arc.priorities()
        slab, widx = _by_slab(segs, T)
        for j, (spec, tail, rec, done, hlen) in enumerate(sts):
            n = AC.windows_of(SC.kept_segments(spec, tail))
            ring = DeviceReplayBuffer(HIST, K, n + 3, DISCOUNT, 64, **kw)
            drec, ddone, dhlen = _dev(rec, done, hlen)
            assert ring.ingest_stream(drec, T, ddone, dhlen, tail=tail, episode_cap=SC.CAP_SYN) == n
            sel = np.flatnonzero(slab == j)
            assert len(sel) == n and np.array_equal(widx[sel], np.arange(n))
            assert torch.equal(_bytes(pri[torch.as_tensor(sel).cuda()]), _bytes(ring.priorities())), (name, j)
    zero = _one_slab(5, prioritized=True, alpha=0.0, prio_eps=EPS)[0]  # alpha = 0: q in {0, 1}
    assert set(zero._q.unique().tolist()) == {0.0, 1.0} and int(zero._q.sum().item()) == zero.windows


# ====================================================================== 4. update and overwrite
def test_update_then_an_append_over_slab_0():
    """Priorities of some roots of slabs 1 and 2 are rewritten; a fourth stage then lands on slab 0: slab 0's q is a
    fresh init (that of a one-slab archive holding that stage), slabs 1 and 2 keep their bits."""
    alpha = 0.6
    kw = dict(prioritized=True, alpha=alpha, prio_eps=EPS)
    arc, host, stages = _mixed(3, **kw)
    B, T = arc.B, arc.steps
    slab_rows = T * B
    roots = APC.root_rows(host.plan(), B, K)
    late = roots[roots >= slab_rows]
    g = np.random.default_rng(8)
    pick = g.choice(late, 64, replace=False)
    assert (pick // slab_rows == 1).any() and (pick // slab_rows == 2).any()
    rows = np.concatenate([pick, pick[:5], [-1]])  # duplicates carry equal td; -1 is skipped
    td_of = g.random(arc.T * B).astype(np.float32) * 3
    td = np.concatenate([td_of[pick], td_of[pick[:5]], [9.0]]).astype(np.float32)
    q0 = arc._q.clone()
    arc.update_priorities(_i32(rows), torch.from_numpy(td).cuda())
    q1 = arc._q.clone()
    touched = torch.zeros(arc.T * B, dtype=torch.bool)
    touched[torch.from_numpy(pick)] = True
    assert torch.equal(_bytes(q1.cpu()[~touched]), _bytes(q0.cpu()[~touched]))
    t = torch.from_numpy(td_of[pick])
    ref = _t64(PR.priority(t.double().numpy(), EPS, alpha))
    _check("update", q1.cpu()[torch.from_numpy(pick)], ref, (t + EPS) ** alpha, 3 * ref)
    assert _append(arc, host, stages[3], T) == 0
    fresh = _archive(1, T, B, **kw)
    spec, tail, rec, done, hlen = stages[3]
    drec, ddone, dhlen = _dev(rec, done, hlen)
    fresh.append(drec, T, ddone, dhlen, tail=tail)
    assert fresh.windows > 0
    assert torch.equal(_bytes(arc._q[:slab_rows]), _bytes(fresh._q))
    assert not torch.equal(_bytes(arc._q[:slab_rows]), _bytes(q1[:slab_rows]))
    assert torch.equal(_bytes(arc._q[slab_rows:]), _bytes(q1[slab_rows:]))
    _check_init("slab 0 after the overwrite", arc, host.plan(), alpha, rows=(0, slab_rows))
    arc.reprioritize(2)  # the public form: slab 2 back to the init rule, slab 1 as it is
    assert torch.equal(_bytes(arc._q[2 * slab_rows:]), _bytes(q0[2 * slab_rows:]))
    assert torch.equal(_bytes(arc._q[slab_rows:2 * slab_rows]), _bytes(q1[slab_rows:2 * slab_rows]))


# ====================================================================== 5. containment
def _table_sample(arc, q, n, step=0, seed=0, u=None, beta=None):
    """mzba_archive_sample with the archive's table on a given q -> rows, idx, prob, weight on the host."""
    L = _L()
    rows = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    idx = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    prob = torch.full((n,), float("nan"), device="cuda")
    weight = torch.full((n,), float("nan"), device="cuda")
    ws = arc._sample_workspace(n)
    L.call("mzba_archive_sample", L.ptr(q), arc.T * arc.B, n, arc.beta if beta is None else beta, 0, L.ptr(arc._table),
           arc.nmax, L.ptr(arc._offs), L.ptr(arc._totals), arc.B, K, seed, step, None, L.ptr(u), L.ptr(rows), L.ptr(idx),
           L.ptr(prob), L.ptr(weight), L.ptr(ws), ws.numel(), L.stream())
    torch.cuda.synchronize()
    return rows.cpu(), idx.cpu(), prob.cpu(), weight.cpu()


def test_containment():
    """A hand-set q > 0 on a non-root: rows = idx = -1, weight 0, the staged row untouched by the gather, the other
    weights normalised over the valid samples. All-zero q: -1 everywhere. Argument errors write nothing."""
    L = _L()
    T, B, n, beta = 24, 9, 32, 0.7  # 32 strata of 10 / 32: every live row's interval holds a whole one
    spec = SC.random_spec(B, T, seed=21)
    stage = _one_stage(spec, T, "keep", 22)
    arc, host = _archive(2, T, B, prioritized=True, beta=beta, prio_eps=EPS), AC.HostArchive(2, T, B)
    _append(arc, host, stage, T)
    segs = host.plan()
    n_rows, N = arc.T * B, arc.windows
    brute = APC.lookup_brute(segs, B, K, n_rows)
    roots = np.flatnonzero(brute >= 0)
    b0, t0, L0 = segs[0]
    bad = [(t0 + L0 - 1) * B + b0, (T + 3) * B + 4]  # a segment's last record; a row of the unfilled slab
    assert (brute[bad] == -1).all()
    r1, r2 = int(roots[3]), int(roots[-2])
    q = np.zeros(n_rows, np.float32)
    q[[r1, r2]] = [1.0, 4.0]
    q[bad] = [3.0, 2.0]
    arc._q.copy_(torch.from_numpy(q))
    rows, idx, prob, weight = _table_sample(arc, arc._q, n, step=3, seed=5)
    drawn = APC.sample_rows(q, n, APC.draws53(n, 3, 5))
    valid = brute[drawn] >= 0
    assert valid.any() and (~valid).any() and set(drawn[valid]) == {r1, r2}
    assert np.array_equal(rows.numpy(), np.where(valid, drawn, -1))
    assert np.array_equal(idx.numpy(), np.where(valid, brute[drawn], -1))
    assert (weight[torch.from_numpy(~valid)] == 0).all() and (prob[torch.from_numpy(~valid)] == 0).all()
    raw = (N * q[drawn].astype(np.float64) / 10.0) ** -np.float64(np.float32(beta))
    want = np.where(valid, raw / raw[valid].max(), 0.0)
    assert np.abs(weight.double().numpy() - want).max() <= 2.0 ** -22 and weight.max() == 1.0
    # through the view: the staged rows of the unusable draws are left as they were
    view = arc.prioritized_view(n)
    _poison(view.staged)
    slots, w, p = view.sample(n, 3, seed=5)
    assert slots.tolist() == list(range(n)) and torch.equal(w.cpu(), weight) and torch.equal(view.rows.cpu(), rows)
    assert _is_poison(view.staged, torch.from_numpy(np.flatnonzero(~valid)).cuda())
    ref, _, _ = arc.gather(int(valid.sum()), idx=_i32(brute[drawn][valid]))
    for k, t in view.staged._ring.items():
        assert torch.equal(_bytes(t[torch.from_numpy(np.flatnonzero(valid)).cuda()]), _bytes(ref._ring[k])), k
    # update through the view: the unusable draws write nowhere
    view.update_priorities(slots, torch.full((n,), 6.0, device="cuda"))
    q2 = arc._q.cpu().numpy()
    assert q2[r1] == q2[r2] == np.float32(6.0) + np.float32(EPS) and np.array_equal(q2[bad], q[bad])
    assert (q2 != q).sum() == 2
    # no priority mass
    arc._q.zero_()
    for u in (None, torch.zeros(n, dtype=torch.float64, device="cuda")):
        rows, idx, prob, weight = _table_sample(arc, arc._q, n, u=u)
        assert (rows == -1).all() and (idx == -1).all() and (weight == 0).all() and (prob == 0).all()
    # a table without a kept segment: every live row is unusable
    empty = _archive(2, T, B, prioritized=True)
    one = torch.ones(n_rows, device="cuda")
    rows, idx, prob, weight = _table_sample(empty, one, n)
    assert (rows == -1).all() and (idx == -1).all() and (weight == 0).all()
    # argument errors: a negative code, no launch
    f = L.lib().mzba_archive_sample
    qd = torch.ones(n_rows + 4, device="cuda")
    outs = [torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2)] + \
        [torch.full((n,), -7.0, device="cuda") for _ in range(2)]
    ws = arc._sample_workspace(n)
    ok = dict(q=L.ptr(qd), n_rows=n_rows, n=n, beta=1.0, n_live=0, table=L.ptr(arc._table), offs=L.ptr(arc._offs),
              totals=L.ptr(arc._totals), B=B, K=K, rows=L.ptr(outs[0]), idx=L.ptr(outs[1]), ws=L.ptr(ws),
              nbytes=ws.numel())
    bad_calls = {"NULL q": (dict(q=None), -1), "n = 0": (dict(n=0), -1), "n > 2^20": (dict(n=2 ** 20 + 1), -1),
                 "beta < 0": (dict(beta=-1.0), -1), "n_rows = 0": (dict(n_rows=0), -1),
                 "table without idx": (dict(idx=None), -1), "table without offs": (dict(offs=None), -1),
                 "K = 0": (dict(K=0), -1), "rows not whole": (dict(n_rows=n_rows + 1), -1),
                 "no table, nothing live": (dict(table=None), -3), "short workspace": (dict(nbytes=ws.numel() - 1), -2),
                 "misaligned q": (dict(q=ctypes.c_void_p(qd.data_ptr() + 4)), -2), "NULL ws": (dict(ws=None), -1)}
    for name, (kw, code) in bad_calls.items():
        a = {**ok, **kw}
        assert f(a["q"], a["n_rows"], a["n"], a["beta"], a["n_live"], a["table"], arc.nmax, a["offs"], a["totals"],
                 a["B"], a["K"], 0, 0, None, None, a["rows"], a["idx"], L.ptr(outs[2]), L.ptr(outs[3]), a["ws"],
                 a["nbytes"], L.stream()) == code, name
    assert L.lib().mzba_archive_sample_ws_bytes(0, 8) == -1 and L.lib().mzba_archive_sample_ws_bytes(8, 0) == -1
    assert L.lib().mzba_archive_sample_ws_bytes(2 ** 31 - 1, 512) % 16 == 0
    g = L.lib().mzba_archive_priority_init
    init = lambda row0, nrows, table: g(ctypes.byref(arc._sink), table, arc.nmax, L.ptr(arc._offs),  # noqa: E731
                                        L.ptr(arc._totals), L.ptr(outs[2]), row0, nrows, K, L.ptr(arc._dpow), 1.0, EPS,
                                        L.stream())
    assert init(arc.T - 1, 2, L.ptr(arc._table)) == -1 and init(-1, 1, L.ptr(arc._table)) == -1
    assert init(0, 1, None) == -1
    h = L.lib().mzba_archive_row_windows
    assert h(None, arc.nmax, L.ptr(arc._offs), L.ptr(arc._totals), B, K, n_rows, L.ptr(outs[0]), n, L.ptr(outs[1]),
             L.stream()) == -1
    assert h(L.ptr(arc._table), arc.nmax, L.ptr(arc._offs), L.ptr(arc._totals), 0, K, n_rows, L.ptr(outs[0]), n,
             L.ptr(outs[1]), L.stream()) == -1
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in outs)


# ====================================================================== 6. acted stages: reanalyse and the learner
class _Acted:
    """Three streamed stages of the tiny nets (B = 8, T = 64, S = 20; test_gpu_archive's end-to-end case), their sinks
    cloned so that any number of archives can be filled with the same rows."""

    def __init__(self):
        from mzba.agent import MuZeroAgent
        from mzba.config import small_model_cfg
        from mzba.stream import StreamingStage
        from mzba.weights import init_state_dict
        self.B, self.T, self.cap, self.seed = SC.STAGE_B, SC.STAGE_T, SC.STAGE_CAP_SHORT, SC.STAGE_SEED
        cfg = SC.default_config()
        cfg["model"] = small_model_cfg(cfg)
        cfg["num_simulations"], cfg["n_parallel"] = SC.STAGE_S, self.B
        self.cfg, self.Lh, self.disc = cfg, cfg["model"]["state_history_length"], cfg["discount_factor"]
        self.agent = MuZeroAgent(cfg["model"], dtype="f32")
        self.agent.load_state_dict(init_state_dict(cfg["model"], SC.STAGE_SD_SEED))
        st = StreamingStage(cfg, self.agent, steps=self.T, episode_cap=self.cap, seed=self.seed)
        self.sinks = []
        for _ in range(3):
            st.run()
            loop = st.loop
            rec = {k: loop.rec[k][:self.T].clone() for k in ("action", "reward", "mask", "counts", "values", "frame",
                                                             "start")}
            self.sinks.append((rec, loop.env.done.clone(), loop.env.hist_len.clone(), st.last_search_id0))

    def archive(self, stages, slabs=3, **kw):
        from mzba.archive import SinkArchive
        arc = SinkArchive(slabs, self.T, self.B, K, self.Lh, self.disc, episode_cap=self.cap, **kw)
        for s in stages:
            self.append(arc, s)
        return arc

    def append(self, arc, s):
        rec, done, hlen, sid = self.sinks[s]
        return arc.append(rec, self.T, done, hlen, tail="drop", search_id0=sid)


@pytest.fixture(scope="module")
def acted():
    return _Acted()


def _host_segs(arc):
    host = AC.HostArchive(arc.slabs, arc.steps, arc.B, cap=arc.episode_cap)
    for k in ("mask", "start"):
        host.rec[k] = arc.rec[k].cpu().numpy().view(host.rec[k].dtype)
    return host.plan()


def test_refresh_writes_the_slabs_priorities(acted):
    """refresh(slab 1) with another net: slab 1's q is the init rule on the refreshed values (bit for bit against a
    gather), slab 0's learned priorities keep their bits."""
    from mzba.reanalyse import Reanalyser
    from mzba.weights import init_state_dict
    arc = acted.archive([0, 1], slabs=2, prioritized=True, prio_eps=EPS)
    segs = _host_segs(arc)
    slab_rows = acted.T * acted.B
    roots = APC.root_rows(segs, acted.B, K)
    assert (roots < slab_rows).any() and (roots >= slab_rows).any() and len(roots) == arc.windows
    _check_init("acted stages", arc, segs, 1.0)
    some = roots[roots < slab_rows][::3]
    arc.update_priorities(_i32(some), torch.linspace(0.5, 2.0, len(some), device="cuda"))
    q0 = arc._q.clone()
    acted.agent.load_state_dict(init_state_dict(acted.cfg["model"], 6))
    try:
        assert arc.refresh(Reanalyser(acted.cfg, acted.agent, acted.B, seed=acted.seed), 1) == acted.T
    finally:
        acted.agent.load_state_dict(init_state_dict(acted.cfg["model"], SC.STAGE_SD_SEED))
    assert _host_segs(arc) == segs
    assert torch.equal(_bytes(arc._q[:slab_rows]), _bytes(q0[:slab_rows]))
    assert not torch.equal(_bytes(arc._q[slab_rows:]), _bytes(q0[slab_rows:]))
    _check_init("refreshed slab 1", arc, segs, 1.0, rows=(slab_rows, 2 * slab_rows))


def _learner(guard=None, seed=6):
    from mzba.config import learner_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    lm = learner_model_cfg()
    assert lm["state_history_length"] == 4
    return Learner(lm, init_state_dict(lm, seed), K=K, guard=guard)


def test_learner_runs_the_prioritized_step_from_the_archive(acted):
    """Three prioritized steps of B = 8 with an append before the third, three ways: through prioritized_view, eager;
    the first eager, then captured and replayed twice (the device step moves on by itself, the append is followed
    without a recapture); spelled out by hand. Losses, parameters and q agree bit for bit."""
    n, seed = 8, 11
    kw = dict(prioritized=True, alpha=0.6, beta=0.4, prio_eps=EPS)
    runs = []
    for how in ("eager", "captured", "by hand"):
        arc = acted.archive([0, 1], **kw)
        lrn = _learner()
        losses = []
        view = arc.prioritized_view(n)
        assert view is arc.prioritized_view(n) and view._ring is arc.staged(n)._ring and view._abi is arc.staged(n)._abi
        for i in range(3):
            if i == 2:
                acted.append(arc, 2)
            if how == "by hand":
                rows, idx, w, _ = arc.sample(n, i, seed=seed)
                st, slots, idx_out = arc.gather(n, idx=idx, out=arc.staged(n))
                assert torch.equal(idx_out, idx) and (idx >= 0).all() and (rows >= 0).all()
                assert torch.equal(arc.root_rows()[idx.long()], rows.long())
                assert (w > 0).all() and w.max() == 1.0
                losses.append(lrn.train_minibatch(st, slots, weights=w).clone())
                arc.update_priorities(rows, lrn.last_td)
            else:
                if how == "captured" and i == 1:
                    lrn.capture(view, n, prioritized=True, seed=seed)
                losses.append(lrn.prioritized_step(view, n, seed).clone())
                assert (lrn._graph is not None) == (how == "captured" and i >= 1)
        torch.cuda.synchronize()
        assert lrn.step_count == 3 and all(torch.isfinite(x).all() for x in losses)
        runs.append((losses, lrn.P.clone(), arc._q.clone(), arc))
    for losses, P, q, arc in runs[1:]:
        for i, (a, b) in enumerate(zip(runs[0][0], losses)):
            assert torch.equal(_bytes(a), _bytes(b)), i
        assert torch.equal(_bytes(P), _bytes(runs[0][1])) and torch.equal(_bytes(q), _bytes(runs[0][2]))
    # the steps moved priorities, and only at roots
    arc = runs[0][3]
    fresh = acted.archive([0, 1, 2], **kw)
    assert not torch.equal(_bytes(fresh._q), _bytes(arc._q)) and torch.equal(fresh._q == 0, arc._q == 0)
    # training_stage(prioritized=True) is num_batches such steps
    a, b = acted.archive([0, 1], **kw), acted.archive([0, 1], **kw)
    la, lb = _learner(), _learner()
    got = a.training_stage(la, 2, n, seed=seed, prioritized=True)
    want = [float(lb.prioritized_step(b.prioritized_view(n), n, seed)[0]) for _ in range(2)]
    assert got == want and la.per_step == 2 and torch.equal(_bytes(a._q), _bytes(b._q))
    assert la.training_stage(a.prioritized_view(n), 1, n, prioritized=True, seed=seed) is not None and la.per_step == 3


def test_a_skipped_step_leaves_the_priorities(acted):
    """NaN in one element of the value head's bias under a guarded learner: the prioritized step from the archive is
    skipped and q keeps its bits; repaired, the next step rewrites the sampled rows."""
    from mzba import guard as G
    n = 8
    arc = acted.archive([0, 1], prioritized=True, alpha=0.6, beta=0.4, prio_eps=EPS)
    view = arc.prioritized_view(n)
    lrn = _learner(G.StepGuard())
    lrn.prioritized_step(view, n, seed=7)
    off = lrn.params["pred_net.value_head.2.bias"].off
    good = lrn.P[off].clone()
    lrn.P[off] = float("nan")
    q0 = arc._q.clone()
    loss = lrn.prioritized_step(view, n, seed=7)
    assert not torch.isfinite(loss).all() and lrn.guard_stats()["skip"] == 1
    assert torch.equal(_bytes(arc._q), _bytes(q0))
    lrn.P[off] = good
    lrn.prioritized_step(view, n, seed=7)
    assert lrn.guard_stats()["skip"] == 0 and torch.isfinite(arc._q).all()
    changed = (arc._q != q0).nonzero().flatten().cpu()
    assert 0 < changed.numel() <= n and set(changed.tolist()) <= set(view.rows.tolist())


def test_an_archive_without_priorities(acted):
    """prioritized=False: every PER method raises, no q is kept, and the uniform stage gives the bits of a prioritized
    archive's uniform stage (the draws of stream 6, untouched by the priorities)."""
    plain, prio = acted.archive([0, 1]), acted.archive([0, 1], prioritized=True)
    assert plain._q is None and not plain.prioritized
    t = torch.zeros(4, dtype=torch.int32, device="cuda")
    for call in (lambda: plain.sample(4, 0), lambda: plain.update_priorities(t, t.float()), plain.priorities,
                 lambda: plain.prioritized_view(4), lambda: plain.reprioritize(0), lambda: plain._sample_workspace(4),
                 lambda: plain.training_stage(_learner(), 1, 4, prioritized=True)):
        with pytest.raises(RuntimeError, match="prioritized=False"):
            call()
    la, lb = _learner(), _learner()
    assert plain.training_stage(la, 2, 8, seed=3) == prio.training_stage(lb, 2, 8, seed=3)
    assert torch.equal(_bytes(la.P), _bytes(lb.P)) and plain.draw_step == prio.draw_step == 1
    for k in plain.staged(16)._ring:
        assert torch.equal(_bytes(plain.staged(16)._ring[k]), _bytes(prio.staged(16)._ring[k])), k
