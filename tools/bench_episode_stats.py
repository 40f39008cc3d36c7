"""The cost of the episode statistics beside the streamed plan.

  timeout 300 python tools/bench_episode_stats.py [--out profiles/r16/train/episode_stats.json]

A synthetic streamed sink of --envs x --rows rows on the device (episodes of 20 .. 261 records back to back, no
frames): `EpisodeStats.add` and `mzba_replay_stream_plan` on the same sink in one process, HIP events around every
launch, --launches timed after --warmup. The plan walks the same columns reading 9 bytes a row; the statistics walk them
twice, 9 bytes forward and 37 backward. Prints one JSON line and writes it to --out. Needs a GPU."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "muzero-breakout_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def synthetic_sink(B, T, cap, seed):
    g = np.random.default_rng(seed)
    start = np.zeros((T, B), np.int32)
    for b in range(B):
        t = 0
        while t < T:
            start[t, b] = -2 ** 31 + 1  # flag bit and a non-zero body
            t += int(g.integers(20, cap + 1))
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(seed)
    rec = {
        "action": torch.randint(0, 3, (T, B), device=dev, generator=gen, dtype=torch.uint8),
        "reward": torch.randint(-1, 2, (T, B), device=dev, generator=gen).float(),
        "mask": torch.ones(T, B, dtype=torch.uint8, device=dev),
        "counts": torch.randint(0, 30, (T, B, 3), device=dev, generator=gen),
        "values": torch.randn(T, B, device=dev, generator=gen),
        "frame": None,
        "start": torch.from_numpy(start).to(dev),
    }
    done = torch.zeros(B, dtype=torch.uint8, device=dev)
    hlen = torch.zeros(B, dtype=torch.int32, device=dev)
    return rec, done, hlen


def timed(fn, n):
    ev = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def _summary(v):
    a = np.asarray(v, np.float64)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)),
            "p90_ms": float(np.percentile(a, 90)), "n": int(a.size)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=1044)
    ap.add_argument("--cap", type=int, default=261)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--stage-seconds", type=float, default=131.0, help="the acting stage the cost is set beside")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from mzba import _lib as L
    from mzba.stats import EpisodeStats
    B, T, K, min_len = a.envs, a.rows, 5, 6
    rec, done, hlen = synthetic_sink(B, T, a.cap, 0)
    st = EpisodeStats(B)
    sink = L.sink(rec, T, 0)
    nmax = B * (T // max(min_len + 1, K))
    cnt = torch.zeros(B, 2, dtype=torch.int32, device="cuda")
    offs = torch.zeros(B + 1, 2, dtype=torch.int32, device="cuda")
    table = torch.zeros(6, nmax + 1, dtype=torch.int32, device="cuda")

    def stats():
        st.add(rec, T, done, hlen, a.cap)

    def plan():
        L.call("mzba_replay_stream_plan", ctypes.byref(sink), L.ptr(done), L.ptr(hlen), K, min_len, a.cap, 0,
               L.ptr(cnt), L.ptr(offs), L.ptr(table), nmax, L.stream())

    res = {}
    for name, fn in (("plan", plan), ("stats", stats), ("plan_again", plan), ("stats_again", stats)):
        timed(fn, a.warmup)
        res[name] = _summary(timed(fn, a.launches))
    d = st.read()
    rows = B * T
    out = {"envs": B, "rows": T, "cap": a.cap, "episodes_per_add": d["episodes"] // (2 * (a.warmup + a.launches)),
           **res, "ratio_stats_over_plan": res["stats"]["median_ms"] / res["plan"]["median_ms"],
           "stats_gb_per_s_at_46_bytes_a_row": rows * 46 / res["stats"]["median_ms"] / 1e6,
           "plan_gb_per_s_at_18_bytes_a_row": rows * 18 / res["plan"]["median_ms"] / 1e6,
           "share_of_stage": res["stats"]["median_ms"] / 1e3 / a.stage_seconds, "stage_seconds": a.stage_seconds}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
