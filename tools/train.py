"""Train on the fast path (mzba.train.Trainer) and log the run as JSON lines.

  python tools/train.py --preset small --envs 256 --steps 261 --slabs 4 --simulations 16 --search gumbel \
      --iterations 40 --eval-every 10 --out run.jsonl [--save run.pth] [--resume run.pth]

Streamed acting into a sink archive, the bf16 device learner, the weight hand-off after every training stage,
optionally reanalyse and prioritized replay. Every iteration writes one line {"kind": "train", ...} with the episode
statistics of its stage (counted on the device), the losses and, with --guard, the guard's block; every --eval-every
iterations, before the first and after the last, one line {"kind": "eval", ...}: `Trainer.evaluate` on a stage of its
own (temperature 0.1, no root noise). --budget-seconds stops iterating once that much wall time is spent, so the closing
evaluation still runs under an outer time limit. Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "muzero-breakout_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--preset", choices=("small", "full"), default="small", help="small_model_cfg or the full nets")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=261, help="rows per stage")
    ap.add_argument("--slabs", type=int, default=4, help="stages the archive keeps")
    ap.add_argument("--simulations", type=int, default=16)
    ap.add_argument("--search", choices=("puct", "gumbel"), default="gumbel")
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--eval-every", type=int, default=0, help="0: only before the first and after the last iteration")
    ap.add_argument("--eval-episodes", type=int, default=1)
    ap.add_argument("--episode-cap", type=int, default=261)
    ap.add_argument("--batches", type=int, default=None, help="minibatches per iteration (default: the config's)")
    ap.add_argument("--minibatch", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=None, help="archive windows before training starts")
    ap.add_argument("--prioritized", action="store_true")
    ap.add_argument("--reanalyse-every", type=int, default=0)
    ap.add_argument("--guard", action="store_true", help="step guard: clip the gradient norm at 5, skip non-finite")
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--resume", default=None, help="a file written by --save")
    ap.add_argument("--save", default=None, help="write the checkpoint here at the end")
    ap.add_argument("--out", default=None, help="JSONL file, appended to (default: stdout only)")
    ap.add_argument("--budget-seconds", type=float, default=0.0)
    a = ap.parse_args(argv)

    from mzba.agent import MuZeroAgent
    from mzba.config import default_config, small_model_cfg
    from mzba.guard import StepGuard
    from mzba.learner import Learner
    from mzba.train import Trainer
    from mzba.weights import init_state_dict

    cfg = default_config()
    if a.preset == "small":
        cfg["model"] = small_model_cfg(cfg)
    cfg["n_parallel"], cfg["num_simulations"] = a.envs, a.simulations
    cfg["search"]["kind"] = a.search
    sd = init_state_dict(cfg["model"], a.seed)
    agent = MuZeroAgent(cfg["model"], dtype="bf16")
    agent.load_state_dict(sd)
    learner = Learner(cfg["model"], sd, K=cfg["num_unroll_steps"], dtype="bf16", lr=a.lr,
                      guard=StepGuard(max_norm=5.0) if a.guard else None)
    tr = Trainer(cfg, agent, learner, steps=a.steps, slabs=a.slabs, episode_cap=a.episode_cap, seed=a.seed,
                 num_batches=a.batches, minibatch_size=a.minibatch, prioritized=a.prioritized, warmup_windows=a.warmup,
                 reanalyse_every=a.reanalyse_every)
    if a.resume:
        tr.load(a.resume)

    out = open(a.out, "a") if a.out else None
    t0 = time.time()

    class Log:
        """One line per record to stdout and to --out, with its kind and the wall time."""
        def __init__(self, kind):
            self.kind = kind

        def write(self, s):
            if s.strip():
                line = json.dumps({"kind": self.kind, "wall_s": round(time.time() - t0, 2), **json.loads(s)})
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()

        def flush(self):
            pass

    def evaluate():
        d = tr.evaluate(episodes=a.eval_episodes)
        d = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in d.items() if k not in ("ep_ret", "ep_len")}
        Log("eval").write(json.dumps({"iteration": tr.it, **d}))

    Log("args").write(json.dumps(vars(a)))
    evaluate()
    train_log = Log("train")
    for i in range(a.iterations):
        if a.budget_seconds and time.time() - t0 > a.budget_seconds:
            Log("note").write(json.dumps({"stopped_after": tr.it, "reason": "budget-seconds"}))
            break
        tr.run(1, log=train_log)
        if a.eval_every and tr.it % a.eval_every == 0 and i + 1 < a.iterations:
            evaluate()
    evaluate()
    if a.save:
        tr.save(a.save)
    if out:
        out.close()


if __name__ == "__main__":
    main()
