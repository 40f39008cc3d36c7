"""The episode-statistics cases are not vacuous (no GPU): the synthetic sinks of tests/test_gpu_episode_stats.py hold
capped episodes, open tails, envs with no episode, one-record episodes, envs that first_n cuts and the 0.3 reward; the
oracle's return is the sequential f32 sum; the histogram clamps at both ends; the binding's struct mirrors agree."""
import math

import numpy as np

import episode_stats_cases as EC
import stream_cases as SC

T = 96
CASES = [(1, 11), (5, 12), (257, 13)]  # (B, seed) of the GPU test's synthetic sinks


def _sink(B, seed):
    spec = SC.random_spec(B, T, seed)
    rec, done, hlen = SC.make_stream_sink(spec, T, seed=seed)
    return spec, rec, done, hlen


def test_synthetic_sinks_hold_every_kind_of_segment():
    seen = dict(capped=0, open_tail=0, no_episode=0, one_record=0, cut1=0, cut3=0, reward03=0)
    for B, seed in CASES:
        spec, rec, done, hlen = _sink(B, seed)
        eps = EC.episodes_of(rec, T, done, hlen, SC.CAP_SYN)
        per_env = np.bincount([b for b, _, _, _ in eps], minlength=B)
        seen["capped"] += sum(L >= SC.CAP_SYN for _, _, _, L in eps)
        seen["one_record"] += sum(L == 1 for _, _, _, L in eps)
        seen["open_tail"] += sum(not closed for _, _, _, closed in SC.segments_of(rec["start"], T, done, hlen, SC.CAP_SYN))
        seen["no_episode"] += int((per_env == 0).sum())
        seen["cut1"] += int((per_env > 1).sum())
        seen["cut3"] += int((per_env > 3).sum())
        seen["reward03"] += sum(bool((rec["reward"][t0:t0 + L, b] == np.float32(0.3)).any()) for b, _, t0, L in eps)
        if B == 257:  # every kind within the one sink that spans two blocks of envs
            assert all(v > 0 for v in seen.values()), seen
    assert all(v > 0 for v in seen.values()), seen


def test_first_n_cuts_and_lists():
    B, seed = 5, 12
    _, rec, done, hlen = _sink(B, seed)
    full = EC.stats_oracle(rec, T, done, hlen, SC.CAP_SYN, ep_n=4)
    one = EC.stats_oracle(rec, T, done, hlen, SC.CAP_SYN, first_n=1, ep_n=4)
    three = EC.stats_oracle(rec, T, done, hlen, SC.CAP_SYN, first_n=3, ep_n=4)
    assert one["episodes"] < three["episodes"] < full["episodes"]
    assert one["episodes"] == int((full["ep_len"][:, 0] > 0).sum())
    assert np.array_equal(one["ep_len"][:, 0], full["ep_len"][:, 0]) and not one["ep_len"][:, 1:].any()
    assert np.array_equal(three["ep_len"][:, :3], full["ep_len"][:, :3]) and not three["ep_len"][:, 3:].any()
    assert sum(full["hist"]) == full["episodes"] and full["rows"] == sum(
        L for _, _, _, L in EC.episodes_of(rec, T, done, hlen, SC.CAP_SYN))


def test_return_is_the_sequential_f32_sum_and_no_integer():
    B, seed = 257, 13
    _, rec, done, hlen = _sink(B, seed)
    o = EC.stats_oracle(rec, T, done, hlen, SC.CAP_SYN, ep_n=4)
    frac = 0
    for b, i, t0, L in EC.episodes_of(rec, T, done, hlen, SC.CAP_SYN):
        s = np.float32(0)
        for t in range(t0, t0 + L):
            s = np.float32(s + rec["reward"][t, b])
        if i < 4:
            assert o["ep_ret"][b, i].view(np.uint32) == s.view(np.uint32) and o["ep_len"][b, i] == L
        frac += float(s) != round(float(s))
    assert frac > 0
    # the f32 sum is not the f64 one: the test would see a kernel that sums in double
    assert any(float(EC.f32_sum(rec["reward"][t0:t0 + L, b])) != math.fsum(float(x) for x in rec["reward"][t0:t0 + L, b])
               for b, _, t0, L in EC.episodes_of(rec, T, done, hlen, SC.CAP_SYN))
    assert not math.isnan(o["verr_sum"]) and not math.isnan(o["entropy_sum"]) and o["verr_rows"] < o["rows"]
    assert 0 < o["entropy_sum"] < o["rows"] * math.log(3) + 1e-9


def test_histogram_edge_bins_clamp():
    assert EC.hist_bin(np.float32(-100), -8.0, 1.0) == 0 and EC.hist_bin(np.float32(1000), -8.0, 1.0) == 31
    assert EC.hist_bin(np.float32(-8), -8.0, 1.0) == 0 and EC.hist_bin(np.float32(-7.5), -8.0, 1.0) == 0
    assert EC.hist_bin(np.float32(-7), -8.0, 1.0) == 1 and EC.hist_bin(np.float32(22.99), -8.0, 1.0) == 30
    assert EC.hist_bin(np.float32(23), -8.0, 1.0) == 31 and EC.hist_bin(np.float32(0.3), 0.0, 0.25) == 1
    # with a narrow histogram both edge bins of the synthetic sink are in use
    _, rec, done, hlen = _sink(257, 13)
    o = EC.stats_oracle(rec, T, done, hlen, SC.CAP_SYN, hist_lo=2.0, hist_step=0.25)
    assert o["hist"][0] > 0 and o["hist"][31] > 0 and sum(o["hist"]) == o["episodes"]


def test_combine_adds_two_sinks():
    _, r1, d1, h1 = _sink(5, 12)
    _, r2, d2, h2 = _sink(5, 14)
    a, b = EC.stats_oracle(r1, T, d1, h1, SC.CAP_SYN), EC.stats_oracle(r2, T, d2, h2, SC.CAP_SYN)
    c = EC.combine(a, b)
    assert c["episodes"] == a["episodes"] + b["episodes"] and c["len_max"] == max(a["len_max"], b["len_max"])
    assert c["ret_min"] == min(a["ret_min"], b["ret_min"]) and c["n_terms"]["verr_sq"] == a["verr_rows"] + b["verr_rows"]


def test_block_mirrors_agree():
    import ctypes
    from mzba import _lib, stats
    assert ctypes.sizeof(_lib.EpisodeStats) == stats.BLOCK_BYTES == 360
    for name, _ in _lib.EpisodeStats._fields_:
        assert getattr(_lib.EpisodeStats, name).offset == stats.BLOCK_DT.fields[name][1], name
    L = _lib.lib()
    assert L.mzba_struct_bytes(b"mzba_episode_stats") == 360
    assert L.mzba_stream_episode_stats_ws_bytes(7) >= 7 * 45 * 8 and L.mzba_stream_episode_stats_ws_bytes(0) == -1
