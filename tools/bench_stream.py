"""Streaming acting against the lockstep stage: what reaches the replay buffer per second (DESIGN.md "Streaming acting").

  python tools/bench_stream.py [--out profiles/r09/stream/bench_stream.json]

bf16 full-width nets, 4096 envs x 50 simulations, bench.py's random-init agent. In one process, alternating in rounds:
one lockstep episode (`ActingStage.run_episode` into a `DeviceReplayBuffer`: every env searched until the last one is
done or 261 steps have passed) and one streamed stage (`StreamingStage(steps=1044).run`: finished envs restart in
place, the sink is ingested by episode). Both replay their captured step graph. HIP events around every acting step
(no synchronisation is added: the lockstep loop reads its done flag per step as it always does, the streamed stage
reads nothing until its ingest); the ingest by the host clock between two synchronisations.

Per mode: steps played, (step, env) rows recorded into kept trajectories and their share of steps x envs, windows
ingested, step time (median, p10, p90), ingest time, and recorded env-steps per second = kept rows / (acting + ingest
wall time). Round 0 (graph capture) is dropped. Prints one JSON line and writes it, with the command, to --out.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "muzero-breakout_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _stats(v):
    a = np.asarray(v, np.float64)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)),
            "p90_ms": float(np.percentile(a, 90)), "n": int(a.size)}


class StepTimer:
    """HIP events around every loop.act() of one stage run."""

    def __init__(self, loop):
        self.events = []
        act = loop.act

        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            act(*a, **k)
            e1.record()
            self.events.append((e0, e1))
        loop.act = timed

    def take(self):
        ms = [a.elapsed_time(b) for a, b in self.events]
        self.events = []
        return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=1044, help="rows of a streamed stage")
    ap.add_argument("--rounds", type=int, default=2, help="timed rounds (one more is run first and dropped)")
    ap.add_argument("--tail", default="drop", choices=["drop", "keep"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream.py needs a GPU")
    from mzba.acting import ActingStage
    from mzba.agent import MuZeroAgent
    from mzba.config import default_config
    from mzba.replay import DeviceReplayBuffer
    from mzba.stream import StreamingStage
    from mzba.weights import init_state_dict

    cfg = default_config()
    cfg["num_simulations"], cfg["n_parallel"] = args.sims, args.envs
    mcfg = cfg["model"]
    K, Lh, B = cfg["num_unroll_steps"], mcfg["state_history_length"], args.envs
    agent = MuZeroAgent(mcfg, dtype=args.dtype)
    agent.load_state_dict(init_state_dict(mcfg, args.seed))
    stages = {"lockstep": ActingStage(cfg, agent, seed=args.seed), "streaming": StreamingStage(cfg, agent, steps=args.steps, seed=args.seed)}
    bufs = {k: DeviceReplayBuffer(Lh, K, cfg["replay_buffer_max"], cfg["discount_factor"], 64) for k in stages}
    timers = {k: StepTimer(s.loop) for k, s in stages.items()}
    acc = {k: {"step_ms": [], "ingest_ms": [], "wall_s": [], "steps": [], "rows": [], "windows": []} for k in stages}

    def ingest_lockstep(buf, loop):
        n = buf.ingest_records(loop.rec, loop.frame0.reshape(-1, loop.H * loop.W), loop.t)
        # kept rows: a trajectory of L records gives L - K + 1 windows
        lens = loop.rec["mask"][:loop.t].sum(0)
        kept = lens[lens > K + 1]
        return n, int(kept.sum().item())

    for r in range(args.rounds + 1):
        for kind, st in stages.items():
            buf, loop = bufs[kind], st.loop
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            # the stage without its ingest, which is timed on its own
            if kind == "lockstep":
                st.run_episode(None, trajectories=False)
            else:
                st.run(None)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if kind == "lockstep":
                n, rows = ingest_lockstep(buf, loop)
            else:
                n = buf.ingest_stream(loop.rec, st.steps, loop.env.done, loop.env.hist_len, tail=args.tail,
                                      episode_cap=st.episode_cap)
                rows = n + buf.last_stream["segments"] * (K - 1)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            ms = timers[kind].take()
            print(f"round {r} {kind}: {len(ms)} steps, {rows} rows kept, {n} windows, acting {t1 - t0:.1f} s, "
                  f"ingest {(t2 - t1) * 1e3:.1f} ms", file=sys.stderr, flush=True)
            if r == 0:
                continue
            a = acc[kind]
            a["step_ms"] += ms
            a["ingest_ms"].append((t2 - t1) * 1e3)
            a["wall_s"].append(t2 - t0)
            a["steps"].append(len(ms))
            a["rows"].append(rows)
            a["windows"].append(n)
    res = {"command": "python tools/bench_stream.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "envs": B, "sims": args.sims, "dtype": args.dtype, "rounds": args.rounds, "tail": args.tail,
           "replay_max": cfg["replay_buffer_max"]}
    for kind, a in acc.items():
        steps, rows = sum(a["steps"]), sum(a["rows"])
        res[kind] = {"steps_played": a["steps"], "rows_kept": a["rows"], "windows": a["windows"],
                     "live_share": rows / (steps * B), "step": _stats(a["step_ms"]),
                     "ingest_ms": a["ingest_ms"], "wall_s": a["wall_s"],
                     "searched_env_steps_per_s": steps * B / sum(a["wall_s"]),
                     "recorded_env_steps_per_s": rows / sum(a["wall_s"])}
    res["recorded_gain"] = res["streaming"]["recorded_env_steps_per_s"] / res["lockstep"]["recorded_env_steps_per_s"]
    lo, hi = res["lockstep"]["step"]["p10_ms"], res["lockstep"]["step"]["p90_ms"]
    res["streaming_median_inside_lockstep_p10_p90"] = bool(lo <= res["streaming"]["step"]["median_ms"] <= hi)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
