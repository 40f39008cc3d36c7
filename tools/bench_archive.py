"""The sink archive against the replay ring: the window gather, the plan and a training stage.

  timeout 1100 python tools/bench_archive.py [--out profiles/r14/archive/bench_archive.json]

bf16 full-width nets, 4096 envs x 50 simulations, bench.py's random-init agent, one process. --stages real streamed
stages (`StreamingStage(steps=1044, episode_cap=261).run`) are played and appended to a `SinkArchive` of --slabs slabs;
the last stage is also ingested into a `DeviceReplayBuffer` of `replay_buffer_max` windows, the parent's path. With
--stages below --slabs the last stage is appended again until every slab is filled (the record says so). HIP events
around every timed launch, round 0 dropped, median with p10 - p90.

(a) the gather: mzba_replay_stream_gather of --windows drawn windows (a fresh Philox step per launch) against the
    parent's mzba_replay_stream_write of the archive's own table into a ring of --windows rows (it writes the table's
    last --windows windows), alternating launch by launch. Both write the same bytes; the bound is the yardstick's
    median plus its p90 - p10.
(b) the plan: mzba_replay_stream_plan over the archive's slabs * steps rows against the same over the last stage's sink.
(c) a training stage: --batches minibatches of --minibatch windows on the learner's captured graph, from the staged
    holder (one gather, then the chunks) and from the ring (`Learner.training_stage`'s randperm slots), two learners of
    one initialisation, alternating stage by stage; events around every minibatch and around the gather.
(d) stored bytes per recorded row, per ring window, and of the whole archive.

Prints one JSON line and writes it (after every part, so a cut run keeps what it had) to --out. Needs a GPU; there is
no fallback."""
import argparse
import ctypes
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
    ap.add_argument("--launches", type=int, default=50, help="(a): launches per kernel and round")
    ap.add_argument("--rounds", type=int, default=2, help="timed rounds (one more is run first and dropped)")
    ap.add_argument("--no-learner", action="store_true", help="skip (c)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_archive.py needs a GPU")
    from mzba import _lib as L
    from mzba.agent import MuZeroAgent
    from mzba.archive import SinkArchive, StagedWindows
    from mzba.config import default_config
    from mzba.learner import Learner
    from mzba.replay import DeviceReplayBuffer
    from mzba.stream import StreamingStage
    from mzba.weights import init_state_dict

    cfg = default_config()
    cfg["num_simulations"], cfg["n_parallel"] = args.sims, args.envs
    mcfg = cfg["model"]
    K, Lh, B, T = cfg["num_unroll_steps"], mcfg["state_history_length"], args.envs, args.steps
    disc, HW = cfg["discount_factor"], 16 * 20
    nwin = args.batches * args.minibatch
    res = {"command": "python tools/bench_archive.py " + " ".join(sys.argv[1:]), "device": torch.cuda.get_device_name(0),
           "envs": B, "sims": args.sims, "dtype": args.dtype, "steps": T, "episode_cap": args.cap, "slabs": args.slabs,
           "real_stages": args.stages, "rounds": args.rounds}

    def save():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(res, indent=1) + "\n")

    agent = MuZeroAgent(mcfg, dtype=args.dtype)
    agent.load_state_dict(init_state_dict(mcfg, args.seed))
    stage = StreamingStage(cfg, agent, steps=T, episode_cap=args.cap, seed=args.seed)
    arc = SinkArchive(args.slabs, T, B, K, Lh, disc, episode_cap=args.cap)
    ring = DeviceReplayBuffer(Lh, K, cfg["replay_buffer_max"], disc, 64)
    res["stages"] = []
    for s in range(max(args.stages, args.slabs)):
        if s < args.stages:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            stage.run(None)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        ms = timed(lambda i: arc.append_stage(stage))[0]  # copy, tail rule, plan, the host read of the totals
        res["stages"].append({"played": s < args.stages, "acting_s": (t1 - t0) if s < args.stages else None,
                              "append_ms": ms, "segments": arc.segments, "windows": arc.windows})
        print(f"stage {s}: {res['stages'][-1]}", file=sys.stderr, flush=True)
    loop = stage.loop
    ms = timed(lambda i: ring.ingest_stream(loop.rec, T, loop.env.done, loop.env.hist_len, episode_cap=args.cap))[0]
    res["ring"] = {"max_length": ring.max_length, "ingest_ms": ms, "windows_given": ring.last_stream["windows"],
                   "windows_kept": len(ring)}
    # (d) bytes
    row = sum(v[0, 0].numel() * v.element_size() for v in arc.rec.values())
    win = sum(v[0].numel() * v.element_size() for v in ring._ring.values())
    res["bytes"] = {"per_recorded_row": row, "per_ring_window": win, "archive_total": arc.stored_bytes(),
                    "archive_rows": arc.T * B, "archive_windows": arc.windows,
                    "archive_windows_as_ring_bytes": arc.windows * win,
                    "ring_total": ring.max_length * win, "plan_table_and_scratch": 4 * (arc._table.numel() +
                                                                                         arc._cnt.numel() +
                                                                                         arc._offs.numel())}
    save()

    # (a) the gather against the parent's writer, same table, same number of windows
    st = StagedWindows(nwin, Lh, K, HW, arc.device)
    yard_ring = StagedWindows(nwin, Lh, K, HW, arc.device)
    sk, dpow = ctypes.byref(arc._sink), L.ptr(arc._dpow)
    step = [1000]

    def gather(i):
        step[0] += 1
        L.call("mzba_replay_stream_gather", sk, arc.H, arc.W, arc.paddle_width, arc.brick_rows, L.ptr(arc._table),
               arc.nmax, L.ptr(arc._totals), None, nwin, args.seed, step[0], None, ctypes.byref(st._abi), 0, dpow, None,
               L.stream())

    def write(i):
        L.call("mzba_replay_stream_write", sk, arc.H, arc.W, arc.paddle_width, arc.brick_rows, L.ptr(arc._table),
               arc.nmax, arc.segments, arc.windows, ctypes.byref(yard_ring._abi), 0, dpow, L.stream())

    kernels = {"mzba_replay_stream_gather": gather, "mzba_replay_stream_write": write}
    acc = {k: [] for k in kernels}
    for r in range(args.rounds + 1):
        per = {k: [] for k in kernels}
        for i in range(args.launches):
            for k, fn in kernels.items():
                per[k] += timed(fn)
        if r:
            for k in kernels:
                acc[k] += per[k]
    written = nwin * win
    g = {"windows": nwin, "bytes_written": written, "bytes_written_plus_frames_read": written + nwin * Lh * HW}
    for k, v in acc.items():
        s = _stats(v)
        s["written_bytes_per_s"] = written / (s["median_ms"] * 1e-3)
        g[k] = s
    g["yardstick"] = "mzba_replay_stream_write"
    g.update(_bound(g["mzba_replay_stream_gather"], g["mzba_replay_stream_write"]))
    res["gather"] = g
    save()
    print(f"gather: {g}", file=sys.stderr, flush=True)

    # (b) the plan: the archive's rows against one stage's
    B1 = B
    cnt = torch.empty(B1, 2, dtype=torch.int32, device=arc.device)
    offs = torch.empty(B1 + 1, 2, dtype=torch.int32, device=arc.device)
    nmax1 = B1 * (T // max(arc.min_len + 1, K))
    table = torch.empty(6, nmax1 + 1, dtype=torch.int32, device=arc.device)
    sink1 = L.sink(loop.rec, T, HW)
    plan1 = lambda i: L.call("mzba_replay_stream_plan", ctypes.byref(sink1), L.ptr(loop.env.done),  # noqa: E731
                             L.ptr(loop.env.hist_len), K, arc.min_len, args.cap, 0, L.ptr(cnt), L.ptr(offs),
                             L.ptr(table), nmax1, L.stream())
    plans = {"archive": lambda i: arc._plan(), "one_stage": plan1}
    acc = {k: [] for k in plans}
    for i in range(21):
        for k, fn in plans.items():
            ms = timed(fn)
            if i:
                acc[k] += ms
    res["plan"] = {"archive_rows": arc.T, "stage_rows": T, **{k: _stats(v) for k, v in acc.items()}}
    res["plan"]["ratio"] = res["plan"]["archive"]["median_ms"] / res["plan"]["one_stage"]["median_ms"]
    save()
    print(f"plan: {res['plan']}", file=sys.stderr, flush=True)

    # (c) a training stage from the staged holder and from the ring
    if not args.no_learner:
        mb, nb = args.minibatch, args.batches
        staged = arc.staged(nwin)
        learners = {}
        for kind, holder in (("archive", staged), ("ring", ring)):
            ln = Learner(mcfg, init_state_dict(mcfg, args.seed), K=K, dtype=args.dtype)
            if kind == "archive":
                arc.gather(nwin, step=0, seed=args.seed)
            slots = torch.arange(mb, dtype=torch.int32, device=arc.device)
            ln.train_minibatch(holder, slots)
            ln.train_minibatch(holder, slots)
            ln.capture(holder, mb)
            learners[kind] = ln
        acc = {"archive": [], "ring": [], "gather": []}
        gen = torch.Generator().manual_seed(args.seed)
        for r in range(args.rounds + 1):
            # the archive's stage: SinkArchive.training_stage with events between its launches
            gms = timed(lambda i: arc.gather(nwin, step=arc.draw_step, seed=args.seed))
            arc.draw_step += 1
            sl = torch.arange(nwin, dtype=torch.int32, device=arc.device)
            a_ms = timed(lambda i: learners["archive"].train_minibatch(staged, sl[i * mb:(i + 1) * mb]), nb)
            # the ring's: Learner.training_stage's slots
            perm = torch.randperm(len(ring), generator=gen)
            rs = ((perm[:nwin].to(arc.device) + ring.start) % ring.max_length).to(torch.int32)
            r_ms = timed(lambda i: learners["ring"].train_minibatch(ring, rs[i * mb:(i + 1) * mb]), nb)
            print(f"round {r}: archive {np.median(a_ms):.3f} ms, ring {np.median(r_ms):.3f} ms per minibatch, gather "
                  f"{gms[0]:.3f} ms", file=sys.stderr, flush=True)
            if r:
                acc["archive"] += a_ms
                acc["ring"] += r_ms
                acc["gather"] += gms
        t = {"minibatch": mb, "batches": nb, "from_staged_holder": _stats(acc["archive"]), "from_ring": _stats(acc["ring"]),
             "gather_per_stage": _stats(acc["gather"])}
        t.update(_bound(t["from_staged_holder"], t["from_ring"]))
        gm, am = t["gather_per_stage"]["median_ms"], t["from_staged_holder"]["median_ms"]
        t["gather_share_of_stage"] = gm / (gm + nb * am)
        res["training_stage"] = t
        save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
