"""Weight hand-off from the learner to an acting agent: the host path against the device path, on the GPU.

  python tools/bench_refresh.py [--out profiles/r07/refresh/bench_refresh.json]

Full-width default model, bf16 pack, one bf16 `Learner` and one `MuZeroAgent` in one process; the paths alternate in
rounds (round 0 warms everything up and is dropped):
  host      agent.load_state_dict(learner.state_dict()): what every refresh did before the device path (per-parameter
            D2H copies, the f64 numpy fold and packings, the upload, the in-place copy); host clock around the call
            and a device synchronise;
  eager     agent.refresh_from_learner(learner): the two pack_fold launches plus the device snapshot of the learner's
            state (for the agent's state_dict contract); HIP events around every call, and a host clock around the
            round's calls and one synchronise;
  captured  the same call as a torch.cuda.graph, replayed; the same two clocks;
  pack      PackedNets.refresh_from_learner alone, captured: the two launches without the snapshot copy. Its bytes
            (source weights read once per destination tensor, destination bytes written) over its time is the figure
            to put next to the measured HBM copy rate (MI355X: 6.29 TB/s for a float4 copy).
Every refreshed pack is compared with the host path's, bit for bit, at the size timed. Prints one JSON line and
writes it, with the command, to --out. Needs a GPU; there is no fallback.
"""
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


def _stats(us):
    a = np.asarray(us, np.float64)
    return {"median_us": float(np.median(a)), "p10_us": float(np.percentile(a, 10)),
            "p90_us": float(np.percentile(a, 90)), "n": int(a.size)}


def _timed(fn, n):
    """n calls of fn: per-call HIP event times (us) and the host clock over all of them to a synchronise (us / call)."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e6 / n
    return [a.elapsed_time(b) * 1e3 for a, b in ev], wall


def _same_bits(p, q):
    v = {4: torch.int32, 2: torch.int16}
    return all(torch.equal(a.view(v[a.element_size()]), b.view(v[b.element_size()]))
               for a, b in zip(p.device_tensors(), q.device_tensors()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50, help="device-path calls per kind and round")
    ap.add_argument("--dyn-dtype", default=None, choices=[None, "fp16"])
    ap.add_argument("--small", action="store_true", help="small_model_cfg() (a rehearsal, not a measurement)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refresh.py needs a GPU")
    from mzba.agent import MuZeroAgent, PackedNets
    from mzba.config import default_config, small_model_cfg
    from mzba.learner import Learner
    from mzba.weights import init_state_dict
    mcfg = small_model_cfg() if args.small else default_config()["model"]
    learner = Learner(mcfg, init_state_dict(mcfg, args.seed), dtype="bf16")
    g = torch.Generator(device="cuda").manual_seed(args.seed + 1)

    def move_learner():  # a trained-looking state: every weight and statistic moves between rounds
        learner.G.copy_(torch.randn(learner.G.shape, generator=g, device="cuda") * 0.01)
        learner.adam_step()
        for m, v in learner.run.values():
            m.add_(torch.randn(m.shape, generator=g, device="cuda") * 0.1)
            v.mul_(torch.rand(v.shape, generator=g, device="cuda") + 0.5)

    agent = MuZeroAgent(mcfg, dtype="bf16", dyn_dtype=args.dyn_dtype)
    agent.packed
    move_learner()
    agent.refresh_from_learner(learner)  # job table, snapshot buffers
    table = agent.packed._refresh_table[1]
    graph, pack_graph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        agent.refresh_from_learner(learner)
    with torch.cuda.graph(pack_graph):
        agent.packed.refresh_from_learner(learner)
    kinds = {"eager": lambda: agent.refresh_from_learner(learner), "captured": graph.replay, "pack": pack_graph.replay}
    ev = {k: [] for k in kinds}
    wall = {k: [] for k in kinds}
    host, checks = [], 0
    for r in range(args.rounds + 1):
        move_learner()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agent.load_state_dict(learner.state_dict())
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e6
        print(f"round {r}: host path {dt / 1e3:.1f} ms", file=sys.stderr, flush=True)
        if r:
            host.append(dt)
        want = PackedNets(learner.state_dict(), mcfg, "bf16", "cuda", args.dyn_dtype) if r == args.rounds else None
        for k, fn in kinds.items():
            if want is not None:  # last round: each kind starts from another state's pack and must end bit-equal
                for t in agent.packed.device_tensors():
                    t.zero_()
            e, w = _timed(fn, args.iters)
            if r:
                ev[k] += e
                wall[k].append(w)
            if want is not None:
                if not _same_bits(agent.packed, want):
                    raise SystemExit(f"bench_refresh.py: the {k} path's pack differs from the host path's")
                checks += 1
    n_flat = learner.P.numel()
    snap = 2 * 4 * (n_flat + sum(m.numel() + v.numel() for m, v in learner.run.values()))
    res = {"command": "python tools/bench_refresh.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "model": "small" if args.small else "default", "dyn_dtype": args.dyn_dtype, "parameters_flat": n_flat,
           "jobs": table.njobs, "bn_records": table.nbn, "workgroups": table.job_blocks,
           "host": {"median_ms": float(np.median(host)) / 1e3, "min_ms": min(host) / 1e3, "max_ms": max(host) / 1e3,
                    "n": len(host)},
           "bytes": {"pack_read": table.bytes_read, "pack_written": table.bytes_written, "snapshot_read_write": snap},
           "bit_equal_checks": checks}
    for k in kinds:
        res[k] = {"events": _stats(ev[k]), "wall_us_per_call": [round(w, 2) for w in wall[k]]}
    pack_us = res["pack"]["events"]["median_us"]
    res["pack"]["bytes_per_s"] = (table.bytes_read + table.bytes_written) / (pack_us * 1e-6)
    res["captured"]["bytes_per_s"] = (table.bytes_read + table.bytes_written + snap) / (
        res["captured"]["events"]["median_us"] * 1e-6)
    res["host_over_eager"] = res["host"]["median_ms"] * 1e3 / float(np.median(wall["eager"]))
    res["host_over_captured"] = res["host"]["median_ms"] * 1e3 / float(np.median(wall["captured"]))
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
