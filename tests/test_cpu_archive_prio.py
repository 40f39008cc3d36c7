"""Prioritized replay over the sink archive, its definition without a GPU (tests/archive_prio_cases.py).

1. The row -> window lookup by binary search per env against the list of every window's root row: 3 slabs, B = 67,
   T = 24, all 8 tail combinations, after every append (unfilled slabs, an overwritten slab 0 and middle slab).
2. Every window has exactly one root row, the rows are distinct, and rows outside the sink map to no window.
3. The 53-bit draw: below 1, on the 2^-53 grid, exact in f64, both ends reached.
4. With q in {0, 1} sample j is the floor(t_j)-th live row.
"""
import itertools

import numpy as np
import pytest

import archive_cases as AC
import archive_prio_cases as APC
import stream_cases as SC

B, T, SLABS, K = 67, 24, 3, SC.K


@pytest.mark.parametrize("tails", list(itertools.product(("drop", "keep"), repeat=3)), ids="-".join)
def test_lookup_against_brute_force(tails):
    stages = AC.mixed_stages(B, T, 100, tails + ("keep", "drop"))
    arc = AC.HostArchive(SLABS, T, B)
    slabs = [None] * SLABS
    n_rows = SLABS * T * B
    rows = np.concatenate([np.arange(n_rows), [-1, -B, n_rows, n_rows + B, 2 ** 31 - 1]])
    for spec, tail, rec, done, hlen in stages:
        slabs[arc.append(rec, done, hlen, tail)] = (spec, tail)
        segs = AC.expected_segments(slabs, T)
        assert segs == arc.plan()
        N = AC.windows_of(segs)
        brute = APC.lookup_brute(segs, B, K, n_rows)
        got = APC.lookup(segs, B, K, n_rows, rows)
        assert np.array_equal(got[:n_rows], brute) and (got[n_rows:] == -1).all()
        # every window has exactly one root row
        roots = APC.root_rows(segs, B, K)
        assert len(roots) == N == len(np.unique(roots)) and np.array_equal(np.sort(brute[brute >= 0]), np.arange(N))
        assert np.array_equal(brute[roots], np.arange(N))
        # a root is a masked row of its env; the last K - 1 records of a segment are no roots
        assert arc.rec["mask"].reshape(-1)[roots].all()
        for b, t0, L in segs[:: max(len(segs) // 9, 1)]:
            tail_rows = (t0 + np.arange(L - K + 1, L)) * B + b
            assert (brute[tail_rows] == -1).all() and brute[(t0 + L - K) * B + b] >= 0
        # rows of unfilled slabs
        for j, st in enumerate(slabs):
            if st is None:
                assert (brute[j * T * B:(j + 1) * T * B] == -1).all()


def test_lookup_on_an_empty_plan():
    assert (APC.lookup([], 5, K, 120, np.arange(-2, 125)) == -1).all()
    assert len(APC.root_rows([], 5, K)) == 0


def test_draw_formula_53_bits():
    # the formula on python integers: exact in f64, below 1, on the 2^-53 grid
    for x0, x1 in ((0, 0), (2 ** 32 - 1, 2 ** 32 - 1), (1, 2047), (0, 2048), (123456789, 987654321)):
        u = float(APC.u_of_words(np.uint32(x0), np.uint32(x1)))
        k = x0 * 2 ** 21 + (x1 >> 11)
        assert u == k / 2 ** 53 and 0.0 <= u < 1.0 and (u * 2 ** 53).is_integer()
    assert float(APC.u_of_words(np.uint32(2 ** 32 - 1), np.uint32(2 ** 32 - 1))) == 1.0 - 2.0 ** -53
    assert float(APC.u_of_words(np.uint32(0), np.uint32(2 ** 11))) == 2.0 ** -53
    for step, seed in ((0, 0), (5, 0x1234_5678_9ABC_DEF0), (2 ** 32 - 1, 7)):
        u = APC.draws53(4096, step, seed)
        assert u.dtype == np.float64 and (u >= 0).all() and (u < 1).all()
        assert len(np.unique(u)) == 4096 and (np.abs(u.mean() - 0.5) < 0.03)
        # finer than 24 bits: the draws do not sit on the 2^-24 grid
        assert ((u * 2.0 ** 24) % 1 != 0).mean() > 0.99
        x0, x1, _, _ = APC.rng.philox4x32(3, APC.STREAM_ARCHIVE_PRIO, step, 0, seed)
        assert float(u[3]) == (int(x0) * 2 ** 21 + (int(x1) >> 11)) / 2 ** 53
    assert (APC.draws53(512, 1, 0) != APC.draws53(512, 2, 0)).all()


@pytest.mark.parametrize("n_rows", [1, 1025, 3000, 2 ** 20 + 1025])
def test_with_unit_priorities_sample_j_is_the_floor_t_th_live_row(n_rows):
    g = np.random.default_rng(n_rows)
    q = (g.random(n_rows) < 0.4).astype(np.float32)
    q[n_rows // 2] = 1.0
    live = np.flatnonzero(q)
    for n in (1, 7, 512):
        for u in (APC.draws53(n, 3, 9), np.zeros(n), np.full(n, 1.0 - 2.0 ** -53)):
            rows = APC.live_rank_rows(q, n, u)
            assert (q[rows] == 1).all() and (np.diff(rows) >= 0).all()
            # the longdouble restatement agrees except where the f64 target rounds onto an integer (u = 1 - 2^-53)
            ld = APC.sample_rows(q, n, u)
            rank = np.searchsorted(live, rows)
            assert (np.abs(np.searchsorted(live, ld) - rank) <= 1).all()
            if u[0] == 0.0:  # t_j = j S / n
                t = APC.targets_f64(n, u, len(live))
                assert np.array_equal(rank, np.minimum(np.floor(t), len(live) - 1))
