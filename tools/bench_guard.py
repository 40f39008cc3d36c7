"""Learner step guard: what it costs on the GPU.

  python tools/bench_guard.py [--out profiles/r08/guard/bench_guard.json]

1. Whole step. In one process, alternating in rounds: the captured bf16 full-width minibatch of an unguarded
   learner (`Learner.capture(ring, B)`, the parent commit's step) and of a guarded one (`guard=StepGuard(max_norm,
   lr_schedule)`: snapshot, grad_stats, guard_finish, adam_guard, guard_restore in place of mzba_adam_dev). HIP events
   around every replay; median, p10 and p90 per kind, and their ratio.
2. Replay without the upload. The same replays by the host clock: time until `train_minibatch` returns (the host's
   share) and until a synchronise after it, per kind.
3. The reduction alone. `mzba_grad_stats` over the learner's flat gradient (its real n and segments) against a
   device-to-device `copy_` of the same n floats, alternating in one process; the achieved read bandwidth; then
   `mzba_guard_finish`, `mzba_adam_guard` and `mzba_adam_dev` the same way.
--unguarded-only skips everything that needs the guard's entry points, so that the same script times the unguarded
step on an older build of the library (MZBA_LIB=..., MZBA_LIB_PARTIAL=1).
Prints one JSON line and writes it, with the command, to --out. Needs a GPU; there is no fallback.
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


def _events(n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def _stats(v, scale=1.0, unit="ms"):
    a = np.asarray(v, np.float64) * scale
    return {f"median_{unit}": float(np.median(a)), f"p10_{unit}": float(np.percentile(a, 10)),
            f"p90_{unit}": float(np.percentile(a, 90)), "n": int(a.size)}


def _fill_ring(buf, seed):
    """Synthetic windows as bench.py's learner workload builds them."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    r, cap, K = buf._ring, buf.max_length, buf.K
    shape = tuple(r["states"].shape)
    r["states"].copy_(torch.randint(0, 8, shape, device="cuda", generator=g, dtype=torch.uint8) *
                      (torch.rand(shape, device="cuda", generator=g) < 0.3))
    r["past_actions"].copy_(torch.randint(0, 3, tuple(r["past_actions"].shape), device="cuda", generator=g))
    r["future_actions"].copy_(torch.randint(0, 3, (cap, K), device="cuda", generator=g))
    r["rewards"].copy_(torch.randint(-1, 2, (cap, K), device="cuda", generator=g).float())
    r["targets"].copy_(torch.randn(cap, K, device="cuda", generator=g) * 2)
    r["counts"].copy_(torch.randint(0, 51, (cap, K, 3), device="cuda", generator=g).float() + 1)
    buf.start, buf.length = 0, cap


def time_steps(cap, B, warmup, steps, rounds, seed, kinds):
    from mzba.config import default_config
    from mzba.guard import StepGuard
    from mzba.learner import Learner
    from mzba.replay import DeviceReplayBuffer
    from mzba.weights import init_state_dict
    mcfg = default_config()["model"]
    K, Lh = 5, mcfg["state_history_length"]
    buf = DeviceReplayBuffer(Lh, K, cap, 0.997, 8)
    _fill_ring(buf, seed)
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    draw = lambda: torch.randperm(cap, device="cuda", generator=g)[:B].to(torch.int32)  # noqa: E731
    learners = {}
    for kind in kinds:
        kw = {"guard": StepGuard(max_norm=10.0, lr_schedule=("exp", 0.1, 350000))} if kind == "guarded" else {}
        ln = Learner(mcfg, init_state_dict(mcfg, seed), K=K, dtype="bf16", streams=2, **kw)
        ln.train_minibatch(buf, draw())
        ln.capture(buf, B)
        learners[kind] = ln
    dev, host, wall = ({k: [] for k in kinds} for _ in range(3))
    for r in range(rounds + 1):  # round 0 warms the graphs up and is dropped
        for kind, ln in learners.items():
            n = warmup if r == 0 else steps
            slots = [draw() for _ in range(n)]
            ev = _events(n)
            torch.cuda.synchronize()
            for i in range(n):
                t0 = time.perf_counter()
                ev[i][0].record()
                ln.train_minibatch(buf, slots[i])
                ev[i][1].record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                if r:
                    host[kind].append(t1 - t0)
                    wall[kind].append(t2 - t0)
            if r:
                dev[kind] += [a.elapsed_time(b) for a, b in ev]
    out = {k: {"device": _stats(dev[k]), "host_call": _stats(host[k], 1e6, "us"), "host_to_sync": _stats(wall[k], 1e3)}
           for k in kinds}
    if len(kinds) == 2:
        a, b = out["guarded"]["device"]["median_ms"], out["unguarded"]["device"]["median_ms"]
        out["guarded_over_unguarded"], out["extra_ms"] = a / b, a - b
        out["host_call_saved_us"] = (out["unguarded"]["host_call"]["median_us"] -
                                     out["guarded"]["host_call"]["median_us"])
    if "guarded" in learners:
        d = learners["guarded"].guard_stats()
        out["last_block"] = {k: d[k] for k in ("grad_norm", "seg_norm", "coef", "skip", "t_applied", "skipped", "lr")}
    return out, learners.get("guarded")


def time_kernels(ln, warmup, iters):
    """grad_stats against copy_ on the learner's own gradient buffer, then the other guard launches."""
    from mzba import _lib as L
    from mzba.learner import ADAM_EPS, BETAS, WEIGHT_DECAY
    n, nseg = ln.n_flat, len(ln.guard_segments)
    dst = torch.empty_like(ln.G)
    loss = torch.ones(4, device="cuda")
    s = L.stream()
    sc = torch.tensor(ln._adam_scalars(10), dtype=torch.float32, device="cuda")
    calls = {
        "copy_": lambda: dst.copy_(ln.G),
        "grad_stats": lambda: L.call("mzba_grad_stats", L.ptr(ln.G), n, ln._g_bounds, nseg, L.ptr(loss),
                                     L.ptr(ln._g_ws), ln._g_ws.numel(), s),
        "guard_finish": lambda: L.call("mzba_guard_finish", L.ptr(ln._g_ws), ln._g_ws.numel(), n, nseg,
                                       L.ptr(ln.guard_block), 10.0, 1, ln.lr, 0.1, 350000, None, BETAS[0], BETAS[1],
                                       ADAM_EPS, WEIGHT_DECAY, s),
        "adam_guard": lambda: L.call("mzba_adam_guard", L.ptr(ln.P), L.ptr(ln.G), L.ptr(ln.M1), L.ptr(ln.M2), n,
                                     L.ptr(ln.guard_block), s),
        "adam_dev": lambda: L.call("mzba_adam_dev", L.ptr(ln.P), L.ptr(ln.G), L.ptr(ln.M1), L.ptr(ln.M2), n,
                                   L.ptr(sc), s),
    }
    # each of the two also back to back with itself: alternating, either finds what the other left in the 256 MiB
    # Infinity Cache (the copy reads G right after the reduction has; the reduction finds G behind 2 x 169 MB)
    calls["copy_alone"], calls["grad_stats_alone"] = calls["copy_"], calls["grad_stats"]
    times = {k: [] for k in calls}
    for pair in (("copy_", "grad_stats"), ("copy_alone",), ("grad_stats_alone",), ("guard_finish",),
                 ("adam_dev", "adam_guard")):
        ev = {k: _events(iters) for k in pair}
        for i in range(warmup + iters):
            for k in pair:  # alternating, so that both see the same clocks and the same cache state
                if i >= warmup:
                    ev[k][i - warmup][0].record()
                calls[k]()
                if i >= warmup:
                    ev[k][i - warmup][1].record()
        torch.cuda.synchronize()
        for k in pair:
            times[k] = [a.elapsed_time(b) for a, b in ev[k]]
    out = {k: _stats(v, 1e3, "us") for k, v in times.items()}
    out["n"], out["bytes"] = n, 4 * n
    out["grad_stats_read_TBps"] = 4 * n / (out["grad_stats"]["median_us"] * 1e-6) / 1e12
    out["copy_moved_TBps"] = 8 * n / (out["copy_"]["median_us"] * 1e-6) / 1e12
    out["grad_stats_over_copy"] = out["grad_stats"]["median_us"] / out["copy_"]["median_us"]
    out["chunks"] = (n + 16383) // 16384
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minibatch", type=int, default=512)
    ap.add_argument("--ring", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=10, help="timed replays per kind and round")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=100, help="timed launches per kernel")
    ap.add_argument("--unguarded-only", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_guard.py needs a GPU")
    kinds = ("unguarded",) if args.unguarded_only else ("unguarded", "guarded")
    res = {"command": "python tools/bench_guard.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "library": os.environ.get("MZBA_LIB", "in-tree"), "minibatch": args.minibatch, "ring": args.ring}
    steps, ln = time_steps(args.ring, args.minibatch, args.warmup, args.steps, args.rounds, args.seed, kinds)
    res["captured_step_bf16"] = steps
    if ln is not None:
        res["kernels"] = time_kernels(ln, 10, args.iters)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
