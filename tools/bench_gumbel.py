"""Step cost of the Gumbel search against the PUCT search at the same number of simulations.

  python tools/bench_gumbel.py [--out profiles/r11/gumbel/bench_gumbel.json]

bf16 full-width nets, 4096 envs, bench.py's random-init agent, one process. For each S in --sims (8, 16, 50): one
`ActingLoop` per mode over the same envs and seed, each replaying its captured step graph. The modes alternate in
rounds of --steps acting steps with HIP events around every step (no synchronisation is added inside a round); round 0
(the first eager step and the graph capture) is dropped. PUCT is the search as it was before the Gumbel mode (the fused
prediction launch backs up and selects); the Gumbel step runs the same dynamics and prediction launches without a tree
plus one tree launch per simulation.

Per S and mode: step time median, p10, p90. Per S: overhead = Gumbel median - PUCT median, and the bound it is held to,
the PUCT step's own p10-p90 spread plus S x 12 us (the top of the 4-12 us DESIGN §3 records for the tree kernels).
Prints one JSON line and writes it, with the command, to --out. Needs a GPU; there is no fallback."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "muzero-breakout_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

LAUNCH_US = 12.0


def _stats(v):
    a = np.asarray(v, np.float64)
    return {"median_ms": float(np.median(a)), "p10_ms": float(np.percentile(a, 10)),
            "p90_ms": float(np.percentile(a, 90)), "n": int(a.size)}


def timed_steps(loop, n):
    ev = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loop.act()
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, nargs="+", default=[8, 16, 50])
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=20, help="acting steps per mode and round")
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds (one more is run first and dropped)")
    ap.add_argument("--max-considered", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gumbel.py needs a GPU")
    from mzba.acting import ActingLoop
    from mzba.agent import MuZeroAgent
    from mzba.config import default_config
    from mzba.weights import init_state_dict

    base = default_config()
    base["n_parallel"] = args.envs
    agent = MuZeroAgent(base["model"], dtype=args.dtype)
    agent.load_state_dict(init_state_dict(base["model"], args.seed))
    res = {"command": "python tools/bench_gumbel.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "envs": args.envs, "dtype": args.dtype, "steps_per_round": args.steps, "rounds": args.rounds,
           "max_considered": args.max_considered, "launch_allowance_us": LAUNCH_US, "sims": {}}
    total = args.steps * (args.rounds + 1) + 1
    for S in args.sims:
        loops = {}
        for kind in ("puct", "gumbel"):
            cfg = copy.deepcopy(base)
            cfg["num_simulations"] = S
            if kind == "gumbel":
                cfg["search"]["kind"] = "gumbel"
                cfg["search"]["gumbel"] = {"max_considered": args.max_considered}
            loops[kind] = loop = ActingLoop(cfg, agent, args.envs, seed=args.seed, max_steps=total)
            loop.reset(0)
            loop.act()  # the first step eager, then every step replays the captured graph
            loop.capture()
        acc = {k: [] for k in loops}
        for r in range(args.rounds + 1):
            for kind, loop in loops.items():
                ms = timed_steps(loop, args.steps)
                print(f"S {S} round {r} {kind}: median {np.median(ms):.3f} ms", file=sys.stderr, flush=True)
                if r:
                    acc[kind] += ms
        p, g = _stats(acc["puct"]), _stats(acc["gumbel"])
        over = g["median_ms"] - p["median_ms"]
        bound = (p["p90_ms"] - p["p10_ms"]) + S * LAUNCH_US * 1e-3
        res["sims"][str(S)] = {"puct": p, "gumbel": g, "overhead_ms": over, "overhead_us_per_sim": over * 1e3 / S,
                               "bound_ms": bound, "within_bound": bool(over <= bound)}
        del loops, loop
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
