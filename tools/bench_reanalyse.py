"""Cost of a reanalysed row against an acting step, and of the sink gather against the ring gather.

  timeout 600 python tools/bench_reanalyse.py [--out profiles/r12/reanalyse/bench_reanalyse.json]

bf16 full-width nets, 4096 envs, S = 50, bench.py's random-init agent, one process. An `ActingLoop` first records
--record steps into its sink; a snapshot of those rows is what the `Reanalyser` (same agent) refreshes.

(a) row against step: the loop's captured step and the reanalyser's captured row alternate in rounds of --steps, HIP
    events around every step / row (the row's events include its 12-byte context copy); round 0 is dropped. A row runs
    the step's launches minus the action sampling and the env step, with mzba_sink_rep_input in place of
    mzba_build_rep_input, so it is expected within the step's median plus the step's own p10 - p90 spread.
(b) the gather alone: mzba_sink_rep_input (row --record - 1: every source row is a sink row) against
    mzba_build_rep_input on the loop's env at the same shape and dtype, alternating launch by launch, HIP events
    around each launch; round 0 dropped. Per kernel: median, p10, p90, the algorithmic bytes (the output once, each
    source frame row once) and their rate as a fraction of the 8 TB/s HBM peak.

--stream measures the same two things on a streamed sink:

  timeout 600 python tools/bench_reanalyse.py --stream [--out profiles/r13/reanalyse_stream/bench_reanalyse_stream.json]

A `StreamingStage`'s loop (episode cap --cap, so that at the last recorded row segments of every age up to the cap are
present; the record's `ages_at_gather_row` says what was there) records --record rows; (a) is the streamed acting step
(restart kernel included) against `begin_stream`'s captured row; (b) is mzba_sink_rep_input_stream on the snapshot
(its origin table filled beforehand by mzba_sink_origin, timed apart as `origin_table_fill`: once per sink, not per
row) against mzba_sink_rep_input on the same snapshot (the yardstick: the parent's kernel, the same bytes moved; at row
--record - 1 >= L it reads no g(s0), so any frame0 serves).

Prints one JSON line and writes it, with the command, to --out. Needs a GPU; there is no fallback."""
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

HBM_PEAK = 8.0e12


def _stats(v):
    a = np.asarray(v, np.float64)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)),
            "p90_ms": float(np.percentile(a, 90)), "n": int(a.size)}


def timed(fn, n):
    ev = []
    for i in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--record", type=int, default=40, help="acting steps recorded before the timed rounds")
    ap.add_argument("--steps", type=int, default=10, help="steps / rows per mode and round")
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds (one more is run first and dropped)")
    ap.add_argument("--launches", type=int, default=50, help="(b): launches per kernel and round")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--stream", action="store_true", help="a streamed stage and the streamed entry points (§17)")
    ap.add_argument("--cap", type=int, default=40, help="--stream: the stage's episode cap")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reanalyse.py needs a GPU")
    from mzba import _lib as L
    from mzba.acting import ActingLoop
    from mzba.agent import MuZeroAgent
    from mzba.config import default_config
    from mzba.reanalyse import Reanalyser
    from mzba.weights import init_state_dict

    cfg = default_config()
    cfg["n_parallel"], cfg["num_simulations"] = args.envs, args.sims
    B, T0 = args.envs, args.record
    agent = MuZeroAgent(cfg["model"], dtype=args.dtype)
    agent.load_state_dict(init_state_dict(cfg["model"], args.seed))
    rows_total = T0 + args.steps * (args.rounds + 1) + 1
    if args.stream:
        from mzba.stream import StreamingStage
        stage = StreamingStage(cfg, agent, steps=rows_total, episode_cap=args.cap, seed=args.seed, use_graph=False)
        loop = stage.loop
        stage.blk.copy_(torch.tensor([0, args.cap], dtype=torch.int32))  # StreamingStage.run's set-up, row by row here
    else:
        loop = ActingLoop(cfg, agent, B, seed=args.seed, max_steps=rows_total)
    loop.reset(0)
    loop.act()  # the first step eager, then every step replays the captured graph
    loop.capture()
    for _ in range(T0 - 1):
        loop.act()
    rean = Reanalyser(cfg, agent, B, seed=args.seed, paddle_width=loop.env.pw, brick_rows=loop.env.brick_rows)
    if args.stream:
        rec, _, _ = Reanalyser.snapshot_stream(loop.rec, T0, loop.env.done, loop.env.hist_len)
        frame0 = loop.frame0.clone()
        run = rean.begin_stream(rec, T0, 0)  # captures the row
    else:
        rec, frame0 = Reanalyser.snapshot(loop.rec, loop.frame0, T0)
        run = rean.begin(rec, frame0, T0, 0)  # captures the row
    torch.cuda.synchronize()
    res = {"command": "python tools/bench_reanalyse.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "envs": B, "sims": args.sims, "dtype": args.dtype, "recorded_rows": T0, "steps_per_round": args.steps,
           "rounds": args.rounds, "live_envs_at_last_recorded_row": int(rec["mask"][T0 - 1].sum())}
    if args.stream:  # t - t0 of every env at the row the gather is timed at
        rows = torch.arange(T0, device=rec["start"].device)[:, None].expand(T0, B)
        t0 = torch.where(rec["start"] != 0, rows, torch.zeros_like(rows)).max(0).values
        age = np.bincount((T0 - 1 - t0).cpu().numpy(), minlength=T0)
        res.update(streamed=True, episode_cap=args.cap,
                   ages_at_gather_row={"distinct": int((age > 0).sum()), "min": int(np.flatnonzero(age)[0]),
                                       "max": int(np.flatnonzero(age)[-1]), "distinct_below_L": int((age[:loop.Lh] > 0).sum()),
                                       "envs_younger_than_L": int(age[:loop.Lh].sum()),
                                       "restarts_recorded": int((rec["start"][1:] != 0).sum())})

    # (a) one reanalysed row against one acting step
    acc = {"acting_step": [], "reanalysed_row": []}
    nrow = 0
    for r in range(args.rounds + 1):
        ms_a = timed(lambda i: loop.act(), args.steps)
        ms_r = timed(lambda i: run.row((nrow + i) % T0), args.steps)
        nrow += args.steps
        print(f"round {r}: step {np.median(ms_a):.3f} ms, row {np.median(ms_r):.3f} ms", file=sys.stderr, flush=True)
        if r:
            acc["acting_step"] += ms_a
            acc["reanalysed_row"] += ms_r
    a, w = _stats(acc["acting_step"]), _stats(acc["reanalysed_row"])
    bound = a["median_ms"] + (a["p90_ms"] - a["p10_ms"])
    res["row_vs_step"] = {"acting_step": a, "reanalysed_row": w, "row_minus_step_ms": w["median_ms"] - a["median_ms"],
                          "bound_ms": bound, "within_bound": bool(w["median_ms"] <= bound)}

    # (b) the gather alone
    H, W, Lh, cs = loop.H, loop.W, loop.Lh, loop.cs
    HW, bf16 = H * W, 1 if args.dtype == "bf16" else 0
    out = torch.empty_like(loop.rep_in)
    sink = L.sink(rec, T0, HW)
    sk = ctypes.byref(sink)
    lockstep = lambda i: L.call("mzba_sink_rep_input", sk, L.ptr(frame0), Lh, 0, T0 - 1, None, L.ptr(out), bf16, cs,  # noqa: E731
                                L.stream())
    if args.stream:
        if T0 - 1 < Lh:
            raise SystemExit("--stream: --record must exceed L, so that the yardstick reads sink rows only")
        new, yard = "mzba_sink_rep_input_stream", "mzba_sink_rep_input"
        origin = torch.empty(T0, B, dtype=torch.int32, device=out.device)
        fill = lambda i: L.call("mzba_sink_origin", sk, L.ptr(origin), L.stream())  # noqa: E731
        res["origin_table_fill"] = _stats(timed(fill, 21)[1:])  # once per sink; the first launch dropped
        kernels = {
            new: lambda i: L.call(new, sk, L.ptr(origin), H, W, rean.paddle_width, rean.brick_rows, Lh, 0, T0 - 1, None,
                                  L.ptr(out), bf16, cs, L.stream()),
            yard: lockstep,
        }
    else:
        new, yard = "mzba_sink_rep_input", "mzba_build_rep_input"
        kernels = {new: lockstep, yard: lambda i: loop.env.build_rep_input(out, cs, bool(bf16))}
    acc = {k: [] for k in kernels}
    for r in range(args.rounds + 1):
        per = {k: [] for k in kernels}
        for i in range(args.launches):
            for k, fn in kernels.items():
                per[k] += timed(fn, 1)
        if r:
            for k in kernels:
                acc[k] += per[k]
    nbytes = B * HW * cs * out.element_size() + Lh * B * HW  # the output once, L source frame rows once
    res["gather"] = {"shape": {"B": B, "H": H, "W": W, "L": Lh, "Cs": cs}, "algorithmic_bytes": nbytes,
                     "hbm_peak_bytes_per_s": HBM_PEAK}
    for k, v in acc.items():
        s = _stats(v)
        s["bytes_per_s"] = nbytes / (s["median_ms"] * 1e-3)
        s["fraction_of_hbm_peak"] = s["bytes_per_s"] / HBM_PEAK
        res["gather"][k] = s
    g = res["gather"]
    y = g[yard]
    g["yardstick"], g["bound_ms"] = yard, y["median_ms"] + (y["p90_ms"] - y["p10_ms"])
    g["within_bound"] = bool(g[new]["median_ms"] <= g["bound_ms"])
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
