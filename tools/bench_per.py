"""Prioritized replay: what the device sampler and a whole prioritized step cost on the GPU.

  python tools/bench_per.py [--out profiles/r07/per/bench_per.json]

1. `sample` + `update_priorities` at n = 512 on rings of 60 000 (config.yaml's replay_buffer_max) and 600 000
   slots, every slot live with log-uniform priorities: HIP events around each pair, median and spread over
   --iters pairs after --warmup; the sample alone as well.
2. In the same process, alternating in rounds: the captured bf16 full-width minibatch with uniform slots (the
   parent commit's step: `Learner.capture(ring, B)`) and the captured prioritized step
   (`capture(ring, B, prioritized=True)`: sample -> weighted minibatch -> priority update -> step counter) on the
   same 60 000-window ring; HIP events around every replay, median per kind, and their ratio.
Prints one JSON line and writes it, with the command, to --out. Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "muzero-breakout_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _events(n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def _stats(ms):
    a = np.asarray(ms, np.float64) * 1e3
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
            "p90_us": float(np.percentile(a, 90)), "n": int(a.size)}


def time_sampler(cap, n, warmup, iters, seed):
    from mzba.replay import DeviceReplayBuffer
    buf = DeviceReplayBuffer(1, 5, cap, 0.997, 8, height=1, width=16, prioritized=True, alpha=0.6, beta=0.4)
    g = torch.Generator(device="cuda").manual_seed(seed)
    buf._q.copy_(torch.exp(torch.empty(cap, device="cuda").uniform_(np.log(1e-3), np.log(1e3), generator=g)))
    buf.start, buf.length = 0, cap
    td = torch.rand(cap, device="cuda", generator=g)
    out = {}
    for what in ("sample", "sample+update"):
        ev = _events(iters)
        for i in range(warmup + iters):
            k = i - warmup
            if k >= 0:
                ev[k][0].record()
            slots, _, _ = buf.sample(n, step=i, seed=seed)
            if what != "sample":
                buf.update_priorities(slots, td[:n])
            if k >= 0:
                ev[k][1].record()
        torch.cuda.synchronize()
        out[what] = _stats([a.elapsed_time(b) for a, b in ev])
    out["bytes_scanned"] = 2 * 4 * cap  # the block sums, then the sampled blocks' 4 KB each (<= n of them)
    return out


def _fill_ring(buf, seed):
    """Synthetic windows as bench.py's learner workload builds them, in chunks; priorities by the ingest rule."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r, cap, K = buf._ring, buf.max_length, buf.K
    for lo in range(0, cap, 4096):
        hi = min(lo + 4096, cap)
        m = hi - lo
        shape = (m,) + tuple(r["states"].shape[1:])
        r["states"][lo:hi] = (torch.randint(0, 8, shape, device="cuda", generator=g, dtype=torch.uint8) *
                              (torch.rand(shape, device="cuda", generator=g) < 0.3))
        r["past_actions"][lo:hi] = torch.randint(0, 3, (m, r["past_actions"].shape[1]), device="cuda", generator=g)
        r["future_actions"][lo:hi] = torch.randint(0, 3, (m, K), device="cuda", generator=g)
        r["rewards"][lo:hi] = torch.randint(-1, 2, (m, K), device="cuda", generator=g).float()
        r["targets"][lo:hi] = torch.randn(m, K, device="cuda", generator=g) * 2
        r["values"][lo:hi] = r["targets"][lo:hi] + torch.randn(m, K, device="cuda", generator=g) * 0.5
        r["counts"][lo:hi] = torch.randint(0, 51, (m, K, 3), device="cuda", generator=g).float() + 1
    buf.start, buf.length = 0, cap
    buf._init_priorities(0, cap)


def time_steps(cap, B, warmup, steps, rounds, seed):
    from mzba.config import default_config
    from mzba.learner import Learner
    from mzba.replay import DeviceReplayBuffer
    from mzba.weights import init_state_dict
    mcfg = default_config()["model"]
    K, Lh = 5, mcfg["state_history_length"]
    buf = DeviceReplayBuffer(Lh, K, cap, 0.997, 8, prioritized=True, alpha=0.6, beta=0.4)
    _fill_ring(buf, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    learners = {}
    for kind in ("uniform", "prioritized"):
        ln = Learner(mcfg, init_state_dict(mcfg, seed), K=K, dtype="bf16", streams=2)
        if kind == "uniform":
            ln.train_minibatch(buf, torch.randperm(cap, device="cuda", generator=g)[:B].to(torch.int32))
            ln.capture(buf, B)
        else:
            ln.prioritized_step(buf, B, seed=seed)
            ln.capture(buf, B, prioritized=True, seed=seed)
        learners[kind] = ln
    times = {"uniform": [], "prioritized": []}
    for r in range(rounds + 1):  # round 0 warms both graphs up and is dropped
        for kind, ln in learners.items():
            n = warmup if r == 0 else steps
            slots = [torch.randperm(cap, device="cuda", generator=g)[:B].to(torch.int32) for _ in range(n)]
            ev = _events(n)
            for i in range(n):
                ev[i][0].record()
                if kind == "uniform":
                    ln.train_minibatch(buf, slots[i])
                else:
                    ln.prioritized_step(buf, B, seed=seed)
                ev[i][1].record()
            torch.cuda.synchronize()
            if r:
                times[kind] += [a.elapsed_time(b) for a, b in ev]
    out = {k: {"median_ms": float(np.median(v)), "p10_ms": float(np.percentile(v, 10)),
               "p90_ms": float(np.percentile(v, 90)), "n": len(v)} for k, v in times.items()}
    out["prioritized_over_uniform"] = out["prioritized"]["median_ms"] / out["uniform"]["median_ms"]
    out["extra_ms"] = out["prioritized"]["median_ms"] - out["uniform"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--caps", type=int, nargs="+", default=[60000, 600000])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--minibatch", type=int, default=512)
    ap.add_argument("--ring", type=int, default=60000)
    ap.add_argument("--steps", type=int, default=10, help="timed replays per kind and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-steps", action="store_true", help="sampler timings only")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_per.py needs a GPU")
    res = {"command": "python tools/bench_per.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "n": args.n, "sampler": {str(c): time_sampler(c, args.n, args.warmup, args.iters, args.seed)
                                    for c in args.caps}}
    if not args.no_steps:
        res["captured_step_bf16"] = {"minibatch": args.minibatch, "ring": args.ring,
                                     **time_steps(args.ring, args.minibatch, 3, args.steps, args.rounds, args.seed)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
