"""The episode statistics (include/mzba.h mzba_episode_stats) restated in numpy / python f64 over the
host arrays of a streamed sink, for tests/test_cpu_episode_stats.py, tests/test_gpu_episode_stats.py and
tests/test_gpu_trainer.py. Nothing here calls the library.

* `episodes_of`: every episode (closed segment with L >= 1) of a sink, by env then row, with its per-env number.
* `stats_oracle`: the block's fields for one sink, the per-env lists, and for every f64 field its number of terms and
  the sum of their magnitudes: a sum of n terms added in another order differs by at most n 2^-52 sum|term|.
* `combine`: the oracle of two sinks added in turn. `check_block`: a device block against an oracle.
"""
import math

import numpy as np

from stream_cases import DISCOUNT, segments_of

INT_FIELDS = ("episodes", "capped", "rows", "verr_rows")
F64_FIELDS = ("ret_sum", "ret_sq", "verr_sum", "verr_abs", "verr_sq", "value_sum", "entropy_sum")
NBINS = 32


def f32_sum(x):
    """Sequential f32 sum from 0, in order."""
    s = np.float32(0)
    for r in x:
        s = np.float32(s + np.float32(r))
    return s


def episodes_of(rec, T, done, hlen, cap):
    """[(env, number within the env, t0, L)] of the closed segments with L >= 1 masked rows."""
    out, num = [], {}
    for b, t0, t1, closed in segments_of(rec["start"], T, done, hlen, cap):
        L = int(rec["mask"][t0:t1, b].astype(bool).sum())
        assert rec["mask"][t0:t0 + L, b].all()  # the records are a prefix
        if closed and L >= 1:
            out.append((b, num.get(b, 0), t0, L))
            num[b] = num.get(b, 0) + 1
    return out


def hist_bin(R, lo, step):
    x = math.floor((float(R) - lo) / step)
    return min(max(x, 0), NBINS - 1)


def row_entropy(c):
    n = int(c.sum())
    if n <= 0:
        return 0.0
    h = 0.0
    for x in c:
        if x > 0:
            p = float(x) / float(n)
            h = h - p * math.log(p)
    return h


def stats_oracle(rec, T, done, hlen, cap, first_n=0, ep_n=0, hist_lo=-8.0, hist_step=1.0, gamma=DISCOUNT):
    B = rec["start"].shape[1]
    o = {k: 0 for k in INT_FIELDS}
    o["hist"] = [0] * NBINS
    terms = {k: [] for k in F64_FIELDS}
    rets, lens = [], []
    ep_ret, ep_len = np.zeros((B, ep_n), np.float32), np.zeros((B, ep_n), np.int32)
    for b, i, t0, L in episodes_of(rec, T, done, hlen, cap):
        if first_n and i >= first_n:
            continue
        s = slice(t0, t0 + L)
        R = f32_sum(rec["reward"][s, b])
        rets.append(R)
        lens.append(L)
        o["episodes"] += 1
        o["rows"] += L
        o["capped"] += int(L >= cap)
        o["hist"][hist_bin(R, hist_lo, hist_step)] += 1
        terms["ret_sum"].append(float(R))
        terms["ret_sq"].append(float(R) * float(R))
        if i < ep_n:
            ep_ret[b, i], ep_len[b, i] = R, L
        v = rec["values"][s, b].astype(np.float64)
        terms["value_sum"] += [float(x) for x in v]
        terms["entropy_sum"] += [row_entropy(c) for c in rec["counts"][s, b]]
        if L < cap:
            o["verr_rows"] += L
            G = 0.0
            for k in range(L - 1, -1, -1):
                G = float(rec["reward"][t0 + k, b]) + gamma * G
                e = float(v[k]) - G
                terms["verr_sum"].append(e)
                terms["verr_abs"].append(abs(e))
                terms["verr_sq"].append(e * e)
    for k in F64_FIELDS:
        o[k] = math.fsum(terms[k])
    o["n_terms"] = {k: len(terms[k]) for k in F64_FIELDS}
    o["abs_terms"] = {k: math.fsum(abs(x) for x in terms[k]) for k in F64_FIELDS}
    o["ret_min"] = np.float32(min(rets)) if rets else None
    o["ret_max"] = np.float32(max(rets)) if rets else None
    o["len_min"] = min(lens) if lens else None
    o["len_max"] = max(lens) if lens else None
    o["ep_ret"], o["ep_len"] = ep_ret, ep_len
    return o


def combine(a, b):
    """The oracle of sink a, then sink b, added to one block (the per-env lists are the last sink's)."""
    o = {k: a[k] + b[k] for k in INT_FIELDS + F64_FIELDS}
    o["hist"] = [x + y for x, y in zip(a["hist"], b["hist"])]
    o["n_terms"] = {k: a["n_terms"][k] + b["n_terms"][k] for k in F64_FIELDS}
    o["abs_terms"] = {k: a["abs_terms"][k] + b["abs_terms"][k] for k in F64_FIELDS}
    pick = lambda f, x, y: x if y is None else y if x is None else f(x, y)  # noqa: E731
    o["ret_min"], o["ret_max"] = pick(min, a["ret_min"], b["ret_min"]), pick(max, a["ret_max"], b["ret_max"])
    o["len_min"], o["len_max"] = pick(min, a["len_min"], b["len_min"]), pick(max, a["len_max"], b["len_max"])
    o["ep_ret"], o["ep_len"] = b["ep_ret"], b["ep_len"]
    return o


def f64_bound(o, k):
    """Worst case of a reordered f64 sum of the field's terms."""
    return o["n_terms"][k] * 2.0 ** -52 * o["abs_terms"][k]


def check_block(d, o, what=""):
    """d: the device block as a dict of python values (mzba.stats.block_dict / EpisodeStats.read) against oracle o:
    integers, extremes and the histogram exactly, the f64 sums within the reordering bound, no NaN anywhere."""
    for k in INT_FIELDS:
        assert d[k] == o[k], (what, k, d[k], o[k])
    assert list(d["hist"]) == list(o["hist"]), (what, d["hist"], o["hist"])
    assert sum(d["hist"]) == d["episodes"]
    for k in F64_FIELDS:
        assert not math.isnan(d[k]), (what, k, "NaN: a poisoned row was read")
        assert abs(d[k] - o[k]) <= f64_bound(o, k), (what, k, d[k], o[k], f64_bound(o, k))
    if o["episodes"]:
        for k in ("ret_min", "ret_max"):
            assert np.float32(d[k]).view(np.uint32) == np.float32(o[k]).view(np.uint32), (what, k, d[k], o[k])
        for k in ("len_min", "len_max"):
            assert d[k] == o[k], (what, k, d[k], o[k])
    else:
        assert not math.isnan(d["ret_min"]) and not math.isnan(d["ret_max"])


def check_lists(d, o, what=""):
    """The per-env lists of EpisodeStats.read(): returns as bits, lengths exactly."""
    assert np.array_equal(d["ep_ret"].view(np.uint32), o["ep_ret"].view(np.uint32)), what
    assert np.array_equal(d["ep_len"], o["ep_len"]), what
