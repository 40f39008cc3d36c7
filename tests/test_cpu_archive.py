"""The sink archive's definition without a GPU (tests/archive_cases.py; mzba.archive).

1. Appending with the tail rule and planning the whole archive with every last segment closed plans exactly the union
   of stream_cases.kept_segments(spec_j, tail_j) of the stages now in the slabs, start rows shifted by j * steps, in
   (env, archive row) order: 3 slabs, B = 67, T = 24, all 8 tail combinations, envs without a segment in a slab, a
   kept open tail followed by a slab in which that env has no start word, slab 0 and a middle slab overwritten.
2. The gather's draw ((u64)x * N) >> 32 over the full Philox word stays in [0, N) and reaches beyond 2^24.
"""
import itertools

import numpy as np
import pytest

import archive_cases as AC
import stream_cases as SC

B, T, SLABS = 67, 24, 3


@pytest.mark.parametrize("tails", list(itertools.product(("drop", "keep"), repeat=3)), ids="-".join)
def test_archive_plans_the_union_of_the_slabs_kept_segments(tails):
    stages = AC.mixed_stages(B, T, 100, tails + ("keep", "drop"))
    arc = AC.HostArchive(SLABS, T, B)
    assert arc.plan() == []
    slabs = [None] * SLABS
    seen_tail_then_no_start = False
    for i, (spec, tail, rec, done, hlen) in enumerate(stages):
        slab = arc.append(rec, done, hlen, tail)
        assert slab == i % SLABS  # the fourth stage overwrites slab 0, the fifth the middle slab
        slabs[slab] = (spec, tail)
        want = AC.expected_segments(slabs, T)
        assert arc.plan() == want, (i, tails)
        assert len(want) > 0 and len({b for b, _, _ in want}) < B  # envs without a kept segment exist
        # no segment crosses a slab: its records end in the slab they start in
        assert all(t0 // T == (t0 + L - 1) // T for _, t0, L in want)
        # env 1: an open tail of 14 records in the even stages, no start word in the odd ones
        for j in range(SLABS - 1):
            if slabs[j] and slabs[j + 1] and slabs[j][1] == "keep" and slabs[j][0][1] == ([(14, 14)], False) \
                    and slabs[j + 1][0][1] == ([], True):
                assert (1, j * T, 14) in want and not arc.rec["start"][(j + 1) * T:(j + 2) * T, 1].any()
                seen_tail_then_no_start = True
    assert seen_tail_then_no_start == (tails[0] == "keep")  # stage 0's tail, then stage 1 in the next slab
    # min_len = -1 keeps segments of length K
    want = AC.expected_segments(slabs, T, min_len=-1)
    assert arc.plan(min_len=-1) == want and SC.K in {L for _, _, L in want}


def test_tail_rule_clears_only_the_open_last_segment():
    spec = [([(8, 8), (9, 9)], False), ([(8, 8), (9, 9)], True), ([], True), ([(24, 24)], True), ([(10, 14), (7, 7)], False)]
    rec, done, hlen = SC.make_stream_sink(spec, T, seed=3)
    for tail in ("drop", "keep"):
        arc = AC.HostArchive(2, T, len(spec))
        arc.append(rec, done, hlen, tail)
        m = arc.rec["mask"][:T]
        if tail == "keep":
            assert np.array_equal(m, rec["mask"])
        else:
            assert not m[8:, 0].any() and m[:8, 0].all() and not m[14:, 4].any() and m[:10, 4].all()
            assert np.array_equal(m[:, 1:4], rec["mask"][:, 1:4])
        assert arc.plan() == AC.expected_segments([(spec, tail), None], T)
        assert not arc.rec["mask"][T:].any() and not arc.rec["start"][T:].any()


@pytest.mark.parametrize("N", [1, 7, 2 ** 24 + 3, 2 ** 31 - 1])
def test_draw_formula(N):
    i = np.arange(4096)
    for step, seed in ((0, 0), (5, 0x1234_5678_9ABC_DEF0), (2 ** 32 - 1, 7)):
        j = AC.draw(i, step, seed, N)
        assert j.dtype == np.int64 and (j >= 0).all() and (j < N).all()
        if N > 2 ** 24:
            assert len(np.unique(j)) > 4000
        if N == 2 ** 31 - 1:  # (for N = 2^24 + 3 only three windows lie above 2^24: see the words below)
            assert (j > 2 ** 24).any()
        if N == 1:
            assert not j.any()
    # the formula itself, on python integers
    x = AC.R.philox4x32(3, AC.STREAM_ARCHIVE, 9, 0, 11)[0]
    assert int(AC.draw(3, 9, 11, N)) == (int(x) * N) >> 32
    # the first and the last window are reached, and every window is: consecutive words move j by at most one
    assert AC.window_of_word(np.uint32(0), N) == 0 and AC.window_of_word(np.uint32(2 ** 32 - 1), N) == N - 1
    w = np.arange(2 ** 32 - 4096, 2 ** 32, dtype=np.uint64).astype(np.uint32)
    assert set(np.diff(AC.window_of_word(w, N))) <= {0, 1}
    # other steps give other draws
    if N > 1000:
        assert (AC.draw(i, 1, 0, N) != AC.draw(i, 2, 0, N)).mean() > 0.99
