"""Prioritized replay over the sink archive: the row sampler, the init rule and the captured step.

  timeout 1100 python tools/bench_archive_prio.py [--out profiles/r15/archive_prio/bench_archive_prio.json]
  python tools/bench_archive_prio.py --sampler-only      # no acting: the sampler on synthetic priorities of that shape

bf16 full-width nets, 4096 envs x 50 simulations, bench.py's random-init agent, one process: tools/bench_archive.py's
set-up. --stages real streamed stages (`StreamingStage(steps=1044, episode_cap=261).run`) are played and appended to a
`SinkArchive(prioritized=True)` of --slabs slabs. HIP events around every timed call, round 0 dropped, median with
p10 - p90.

(a) the sampler: `SinkArchive.sample` of --minibatch rows (its five launches together, a fresh Philox step per call),
    the init rule over one slab (`reprioritize`), and the priority update of --minibatch rows, each on its own, with the
    bytes each reads computed from the shapes.
(b) the step: the captured prioritized archive step (sample + gather + weighted minibatch + update:
    `Learner.capture(archive.prioritized_view(B), B, prioritized=True)`) against the captured uniform minibatch from the
    staged holder (tools/bench_archive.py's (c), the parent's path), two learners of one initialisation, alternating
    stage by stage of --batches steps. The bound is the uniform step's median plus its p90 - p10.

Prints one JSON line and writes it (after every part) to --out. Needs a GPU; there is no fallback."""
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


def _stats(v, unit="ms"):
    a = np.asarray(v, np.float64)
    return {f"median_{unit}": float(np.median(a)), f"p10_{unit}": float(np.percentile(a, 10)),
            f"p90_{unit}": float(np.percentile(a, 90)), "n": int(a.size)}


def timed(fn, n=1):
    ev = []
    for i in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(i)
        e1.record()
        ev.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def _bound(new, yard):
    b = yard["median_ms"] + (yard["p90_ms"] - yard["p10_ms"])
    return {"bound_ms": b, "within_bound": bool(new["median_ms"] <= b)}


def sampler_bytes(n_rows, n):
    """Bytes each launch of mzba_archive_sample reads, from the shapes: blocks of 1024 rows, super-blocks of 1024
    blocks; a sample's wave reads at most 11 + 10 prefix words, one block of q and, for the lookup, a handful of table
    words."""
    nblk = (n_rows + 1023) // 1024
    nsup = (nblk + 1023) // 1024
    return {"rows": n_rows, "blocks": nblk, "super_blocks": nsup,
            "partials_reads": 4 * n_rows, "block_scan_reads": 12 * nblk, "super_scan_reads": 12 * nsup,
            "sample_reads_at_most": n * (21 * 8 + 4096 + 64), "weights_reads": 8 * n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--steps", type=int, default=1044, help="rows of a streamed stage = rows of a slab")
    ap.add_argument("--cap", type=int, default=261, help="the stage's episode cap")
    ap.add_argument("--slabs", type=int, default=2)
    ap.add_argument("--stages", type=int, default=2, help="real stages played")
    ap.add_argument("--minibatch", type=int, default=512)
    ap.add_argument("--batches", type=int, default=15)
    ap.add_argument("--launches", type=int, default=50, help="(a): calls per round")
    ap.add_argument("--rounds", type=int, default=2, help="timed rounds (one more is run first and dropped)")
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--beta", type=float, default=0.4)
    ap.add_argument("--sampler-only", action="store_true", help="(a)'s sampler on synthetic priorities, nothing else")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_archive_prio.py needs a GPU")
    from mzba import _lib as L
    from mzba.agent import MuZeroAgent
    from mzba.archive import SinkArchive
    from mzba.config import default_config
    from mzba.learner import Learner
    from mzba.stream import StreamingStage
    from mzba.weights import init_state_dict

    cfg = default_config()
    cfg["num_simulations"], cfg["n_parallel"] = args.sims, args.envs
    mcfg = cfg["model"]
    K, Lh, B, T = cfg["num_unroll_steps"], mcfg["state_history_length"], args.envs, args.steps
    disc, mb, nb = cfg["discount_factor"], args.minibatch, args.batches
    n_rows = args.slabs * T * B
    res = {"command": "python tools/bench_archive_prio.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "envs": B, "sims": args.sims, "dtype": args.dtype, "steps": T,
           "episode_cap": args.cap, "slabs": args.slabs, "real_stages": args.stages, "rounds": args.rounds,
           "alpha": args.alpha, "beta": args.beta, "sampler_bytes": sampler_bytes(n_rows, mb)}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    def rounds_of(fn, per_round):
        acc = []
        for r in range(args.rounds + 1):
            ms = timed(fn, per_round)
            if r:
                acc += ms
        return _stats(acc)

    if args.sampler_only:
        # the plain row sampler on log-uniform priorities with 40 % dead rows: what the five launches cost at this
        # many rows, whatever the rows hold
        g = torch.Generator(device="cuda").manual_seed(args.seed)
        q = torch.exp(torch.rand(n_rows, generator=g, device="cuda") * 13.8 - 6.9)
        q[torch.rand(n_rows, generator=g, device="cuda") < 0.4] = 0.0
        n_live = int((q > 0).sum().item())
        ws = torch.empty(L.lib().mzba_archive_sample_ws_bytes(n_rows, mb), dtype=torch.uint8, device="cuda")
        rows = torch.empty(mb, dtype=torch.int32, device="cuda")
        prob, weight = torch.empty(mb, device="cuda"), torch.empty(mb, device="cuda")
        step = [0]

        def sample(i):
            step[0] += 1
            L.call("mzba_archive_sample", L.ptr(q), n_rows, mb, args.beta, n_live, None, 0, None, None, 0, 0, args.seed,
                   step[0], None, None, L.ptr(rows), None, L.ptr(prob), L.ptr(weight), L.ptr(ws), ws.numel(), L.stream())

        s = rounds_of(sample, args.launches)
        s["partials_read_bytes_per_s"] = 4 * n_rows / (s["median_ms"] * 1e-3)
        res["sampler_synthetic"] = {"live_rows": n_live, **s}
        save()
        print(json.dumps(res))
        return

    agent = MuZeroAgent(mcfg, dtype=args.dtype)
    agent.load_state_dict(init_state_dict(mcfg, args.seed))
    stage = StreamingStage(cfg, agent, steps=T, episode_cap=args.cap, seed=args.seed)
    arc = SinkArchive(args.slabs, T, B, K, Lh, disc, episode_cap=args.cap, prioritized=True, alpha=args.alpha,
                      beta=args.beta)
    res["stages"] = []
    for s in range(max(args.stages, args.slabs)):
        if s < args.stages:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stage.run(None)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        ms = timed(lambda i: arc.append_stage(stage))[0]  # copy, tail rule, plan, host read, the slab's priorities
        res["stages"].append({"played": s < args.stages, "acting_s": (t1 - t0) if s < args.stages else None,
                              "append_ms": ms, "segments": arc.segments, "windows": arc.windows})
        print(f"stage {s}: {res['stages'][-1]}", file=sys.stderr, flush=True)
    q = arc._q
    res["priorities"] = {"rows": n_rows, "bytes": 4 * n_rows, "roots": int((q > 0).sum().item()),
                         "windows": arc.windows, "sum": float(q.double().sum().item()), "max": float(q.max().item())}
    save()

    # (a) the sampler, the init rule over one slab, the update
    step = [1000]

    def sample(i):
        step[0] += 1
        arc.sample(mb, step[0], seed=args.seed)

    arc._sample_workspace(mb)
    a = {"sample": rounds_of(sample, args.launches),
         "init_one_slab": rounds_of(lambda i: arc.reprioritize(args.slabs - 1), args.launches)}
    rows, _, _, _ = arc.sample(mb, 1, seed=args.seed)
    td = torch.rand(mb, device="cuda")
    q_keep = q.clone()
    a["update"] = rounds_of(lambda i: arc.update_priorities(rows, td), args.launches)
    q.copy_(q_keep)
    a["sample"]["partials_read_bytes_per_s"] = 4 * n_rows / (a["sample"]["median_ms"] * 1e-3)
    # the init: per (row, env) the value, the env's two offsets and the store; per root up to 11 rewards, one more
    # value and four table words
    roots = res["priorities"]["roots"] // args.slabs
    a["init_one_slab"]["bytes_at_most"] = T * B * (4 + 8 + 4) + roots * (11 * 4 + 4 + 16)
    res["sampler"] = a
    save()
    print(f"sampler: {a}", file=sys.stderr, flush=True)

    # (b) the captured prioritized step against the captured uniform minibatch from the staged holder
    nwin = nb * mb
    staged = arc.staged(nwin)
    view = arc.prioritized_view(mb)
    uni = Learner(mcfg, init_state_dict(mcfg, args.seed), K=K, dtype=args.dtype)
    pri = Learner(mcfg, init_state_dict(mcfg, args.seed), K=K, dtype=args.dtype)
    arc.gather(nwin, step=0, seed=args.seed)
    slots = torch.arange(mb, dtype=torch.int32, device=arc.device)
    for _ in range(2):
        uni.train_minibatch(staged, slots)
        pri.prioritized_step(view, mb, args.seed)
    uni.capture(staged, mb)
    pri.capture(view, mb, prioritized=True, seed=args.seed)
    acc = {"prioritized": [], "uniform": [], "gather": []}
    sl = torch.arange(nwin, dtype=torch.int32, device=arc.device)
    for r in range(args.rounds + 1):
        p_ms = timed(lambda i: pri.prioritized_step(view, mb, args.seed), nb)
        g_ms = timed(lambda i: arc.gather(nwin, step=arc.draw_step, seed=args.seed))
        arc.draw_step += 1
        u_ms = timed(lambda i: uni.train_minibatch(staged, sl[i * mb:(i + 1) * mb]), nb)
        print(f"round {r}: prioritized {np.median(p_ms):.3f} ms, uniform {np.median(u_ms):.3f} ms per step, uniform "
              f"stage's gather {g_ms[0]:.3f} ms", file=sys.stderr, flush=True)
        if r:
            acc["prioritized"] += p_ms
            acc["uniform"] += u_ms
            acc["gather"] += g_ms
    t = {"minibatch": mb, "batches": nb, "prioritized_archive_step": _stats(acc["prioritized"]),
         "uniform_from_staged_holder": _stats(acc["uniform"]), "uniform_gather_per_stage": _stats(acc["gather"]),
         "yardstick": "uniform_from_staged_holder"}
    t.update(_bound(t["prioritized_archive_step"], t["uniform_from_staged_holder"]))
    t["difference_ms"] = t["prioritized_archive_step"]["median_ms"] - t["uniform_from_staged_holder"]["median_ms"]
    t["losses_finite"] = bool(torch.isfinite(pri._g_loss).all().item())
    t["unusable_draws_last_step"] = int((view.rows < 0).sum().item())
    res["step"] = t
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
