"""The training loop on the fast path: streamed acting, the sink archive, the device learner, the
weight hand-off and reanalyse run together, with episode statistics kept on the device.

    trainer = Trainer(cfg, agent, learner, steps=1044, slabs=4)
    trainer.run(100, log=open("train.jsonl", "a"))     # one JSON line every trainer.log_every iterations
    print(trainer.evaluate(episodes=1)["return_mean"])
    trainer.save("run.pth"); ...; trainer.load("run.pth")  # a fresh Trainer continues bit for bit

One iteration, in this order: `stage.run()`; `stats.add_stage(stage)`; `archive.append_stage(stage, tail="drop")`; from
`warmup_windows` archive windows on, `archive.training_stage(learner, ...)` and `agent.refresh_from_learner(learner)`;
every `reanalyse_every` iterations `archive.refresh` of the oldest filled slab other than the one just written, with a
`Reanalyser` on the same agent (so with the refreshed weights); `temperature_fn(iteration)` into the stage. The host
reads of an iteration are the archive's two: the plan's totals and the losses.
"""
import json

import numpy as np
import torch

from .archive import SinkArchive
from .checkpoint import checkpoint_dict
from .stats import EpisodeStats
from .stream import StreamingStage

EVAL_SEED_OFFSET = 1_000_003  # the evaluation stages' seed is the trainer's plus this


def _jsonable(x):
    if isinstance(x, np.ndarray):
        return x.tolist()
    if isinstance(x, np.generic):
        return x.item()
    if torch.is_tensor(x):
        return x.tolist()
    raise TypeError(f"not JSON serialisable: {type(x)}")


class Trainer:
    """`agent` acts (a bf16 `MuZeroAgent`), `learner` trains (a `Learner` of the same model config; with a
    `StepGuard` or without). cfg["n_parallel"] envs play `steps` rows per iteration into an archive of `slabs` stages.
    `num_batches`, `minibatch_size` and `warmup_windows` default to cfg's num_batches, minibatch_size and
    samples_before_train. `temperature_fn(i)`, if given, is the stage's temperature after iteration i (1-based)."""

    def __init__(self, cfg, agent, learner, steps, slabs, episode_cap=261, seed=0, num_batches=None,
                 minibatch_size=None, prioritized=False, warmup_windows=None, reanalyse_every=0, temperature_fn=None,
                 use_graph=True, log_every=1):
        self.cfg, self.agent, self.learner = cfg, agent, learner
        self.B, self.steps, self.slabs = int(cfg["n_parallel"]), int(steps), int(slabs)
        self.episode_cap, self.seed = int(episode_cap), int(seed)
        self.num_batches = int(cfg["num_batches"] if num_batches is None else num_batches)
        self.minibatch_size = int(cfg["minibatch_size"] if minibatch_size is None else minibatch_size)
        self.warmup_windows = int(cfg["samples_before_train"] if warmup_windows is None else warmup_windows)
        self.prioritized, self.reanalyse_every = bool(prioritized), int(reanalyse_every)
        self.temperature_fn, self.use_graph, self.log_every = temperature_fn, bool(use_graph), max(int(log_every), 1)
        K, disc = cfg["num_unroll_steps"], cfg["discount_factor"]
        if learner.K != K:
            raise ValueError(f"Trainer: the learner unrolls {learner.K} steps, cfg num_unroll_steps is {K}")
        self.stage = StreamingStage(cfg, agent, self.steps, episode_cap=self.episode_cap, seed=self.seed,
                                    use_graph=self.use_graph)
        loop = self.stage.loop
        self.archive = SinkArchive(self.slabs, self.steps, self.B, K, loop.Lh, disc, height=loop.H, width=loop.W,
                                   episode_cap=self.episode_cap, paddle_width=loop.env.pw,
                                   brick_rows=loop.env.brick_rows, device=agent.device, prioritized=self.prioritized)
        self.stats = EpisodeStats(self.B, gamma=disc, device=agent.device)
        self.reanalyser = None
        self.it = 0            # iterations done
        self.last_losses = []
        self._eval = {}        # (episodes, B) -> (StreamingStage, EpisodeStats)

    # -- one iteration ------------------------------------------------------------------------------------
    def _holder(self):
        """The ring-shaped object the learner trains from, the one its graph is captured for."""
        if self.prioritized:
            return self.archive.prioritized_view(self.minibatch_size)
        return self.archive.staged(self.num_batches * self.minibatch_size)

    def _train(self):
        ln, holder = self.learner, self._holder()
        losses = self.archive.training_stage(ln, self.num_batches, self.minibatch_size, seed=self.seed,
                                             prioritized=self.prioritized)
        # the eager stage above allocated what a capture needs; later stages replay the graph (bit-identical launches)
        if self.use_graph and not ln.captured_for(holder, self.minibatch_size, self.prioritized, self.seed):
            ln.capture(holder, self.minibatch_size, prioritized=self.prioritized, seed=self.seed)
        return losses

    def _reanalyse_slab(self, written):
        """The oldest filled slab other than `written`, or None."""
        arc = self.archive
        oldest = arc.appended % arc.slabs if arc.appended >= arc.slabs else 0
        return None if min(arc.appended, arc.slabs) < 2 or oldest == written else oldest

    def iteration(self):
        """-> {"iteration", "segments", "windows", "losses", "trained", "reanalysed"}."""
        stage, arc = self.stage, self.archive
        i = self.it + 1
        stage.run()
        self.stats.add_stage(stage)
        slab = arc.append_stage(stage, tail="drop")
        trained, losses, refreshed = False, [], None
        if arc.windows > 0 and arc.windows >= self.warmup_windows:
            losses = self._train()
            self.agent.refresh_from_learner(self.learner)
            trained = True
        if self.reanalyse_every and i % self.reanalyse_every == 0:
            refreshed = self._reanalyse_slab(slab)
            if refreshed is not None:
                if self.reanalyser is None:
                    env = stage.loop.env
                    from .reanalyse import Reanalyser
                    self.reanalyser = Reanalyser(self.cfg, self.agent, self.B, seed=self.seed, height=stage.loop.H,
                                                 width=stage.loop.W, pad_action=env.pad_action, paddle_width=env.pw,
                                                 brick_rows=env.brick_rows)
                arc.refresh(self.reanalyser, refreshed, use_graph=self.use_graph)
        if self.temperature_fn is not None:
            stage.temperature = float(self.temperature_fn(i))
        self.it, self.last_losses = i, losses
        return {"iteration": i, "segments": arc.segments, "windows": arc.windows, "losses": losses, "trained": trained,
                "reanalysed": refreshed}

    def run(self, n, log=None):
        """n iterations. With `log` (a text file object), every `log_every` iterations one JSON line of the training
        statistics since the last line (`stats.read()`), the last iteration's result and the guard's statistics when
        the learner has a guard; the training statistics are then reset. -> the last iteration's result."""
        out = None
        for _ in range(int(n)):
            out = self.iteration()
            if log is not None and self.it % self.log_every == 0:
                line = {**out, "stats": self.stats.read()}
                if self.learner.guard is not None and out["trained"]:
                    line["guard"] = self.learner.guard_stats()
                log.write(json.dumps(line, default=_jsonable) + "\n")
                log.flush()
                self.stats.reset()
        return out

    # -- evaluation ---------------------------------------------------------------------------------------
    def evaluate(self, episodes=1, B=None, temperature=0.1, noise_weight=0.0):
        """The first `episodes` episodes of each of B envs (default: the training batch), played by a stage of its
        own on the same agent: episodes * episode_cap rows, so every env closes that many; its own seed and an
        env_offset past the training envs, so no keyed draw is shared with training, whose results do not depend on
        whether this ran. -> `EpisodeStats.read()` of exactly episodes * B episodes, with their per-env returns and
        lengths (`ep_ret`, `ep_len`)."""
        stage, stats = self.eval_stage(episodes, B)
        stage.temperature = float(temperature)
        stage.set_noise_weight(float(noise_weight))
        stage.run()
        stats.reset()
        stats.add_stage(stage)
        return stats.read()

    def eval_stage(self, episodes=1, B=None):
        """The evaluation stage and its statistics for (episodes, B), built once -> (StreamingStage, EpisodeStats)."""
        episodes, B = int(episodes), self.B if B is None else int(B)
        if episodes < 1 or B < 1:
            raise ValueError("Trainer.evaluate: episodes and B must be positive")
        key = (episodes, B)
        if key not in self._eval:
            cfg = {**self.cfg, "n_parallel": B}
            stage = StreamingStage(cfg, self.agent, episodes * self.episode_cap, episode_cap=self.episode_cap,
                                   seed=self.seed + EVAL_SEED_OFFSET, env_offset=self.B, use_graph=self.use_graph)
            stats = EpisodeStats(B, first_n=episodes, ep_n=episodes, gamma=self.cfg["discount_factor"],
                                 device=self.agent.device)
            self._eval[key] = (stage, stats)
        return self._eval[key]

    # -- checkpoint ---------------------------------------------------------------------------------------
    def save(self, path, archive=True):
        """The reference's checkpoint layout (`mzba.checkpoint.load_checkpoint` reads the file: the agent's weights,
        the learner's optimizer state, the counters, an empty replay_buffer) plus one "trainer" entry of tensors and
        plain values: the archive (`SinkArchive.state`), the stage's counters, the learner's raw state, the
        statistics block and the temperature. Call it between iterations. archive=False leaves the sink tensors and
        priorities out: such a resume starts from an empty archive (it acts and trains on, but not bit-equal to the
        uninterrupted run, and warms up again)."""
        ln = self.learner
        ck = checkpoint_dict(self.agent, learner=ln, training_iteration=ln.step_count,
                             acting_step=self.stage.loop.step_index, iteration=self.it)
        ck["trainer"] = {
            "version": 1, "iteration": self.it, "seed": self.seed, "episode_cap": self.episode_cap,
            "archive": self.archive.state(sinks=bool(archive)), "stage": self.stage.state(), "learner": ln.state(),
            "stats": self.stats.state().cpu(), "temperature": float(self.stage.temperature),
        }
        torch.save(ck, path)

    def load(self, path):
        """Inverse of `save` into this trainer's objects (built with the saved run's arguments); the archive is
        planned again. The next `iteration()` continues the saved run. -> the checkpoint dict."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        tr = ck.get("trainer")
        if tr is None:
            raise ValueError(f"{path} holds no trainer state (written by save_checkpoint, not Trainer.save)")
        if (tr["seed"], tr["episode_cap"]) != (self.seed, self.episode_cap):
            raise ValueError("Trainer.load: the saved run's seed or episode_cap is not this trainer's")
        self.learner.load_state(tr["learner"])
        self.agent.load_state_dict(ck["model_state_dict"])
        if self.learner.step_count > 0:  # the hand-off of the last trained iteration, by its own path
            self.agent.refresh_from_learner(self.learner)
        self.archive.load_state(tr["archive"])
        self.stage.load_state(tr["stage"])
        self.stats.load_state(tr["stats"])
        self.stage.temperature = float(tr["temperature"])
        self.it = int(tr["iteration"])
        return ck
