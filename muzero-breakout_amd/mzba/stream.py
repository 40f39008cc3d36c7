"""Streaming acting (DESIGN.md "Streaming acting"): finished envs restart in place, records are ingested by episode.

The lockstep stage (`mzba.acting.ActingStage`, the reference's `_acting_stage`) searches every env until the last one
of the batch is done; a finished env keeps its lane and records nothing. A `StreamingStage` plays a fixed number of
rows T instead: at the head of every step the restart kernel (csrc/env.hip) resets each env that is done, or whose
episode holds `episode_cap` records, under the episode key `ep_base + t`, and marks the row with the env's start word.
The sink then holds several episodes per env (segments); `DeviceReplayBuffer.ingest_stream` turns each kept segment
into the windows the reference builds for a trajectory of that length, and `stream_trajectories` into the host
`ObservationTrajectory` objects. Opt-in: nothing here is used by the lockstep path.
"""
import numpy as np
import torch

from .acting import ActingLoop, ObservationTrajectory
from .env import gray_lut


def unpack_start(word):
    """start word -> (paddle, bx, by) of s0 (include/mzba.h)."""
    w = int(word)
    return w & 1023, (w >> 10) & 1023, (w >> 20) & 1023


def render_s0(word, H, W, paddle_width=6, brick_rows=3):
    """u8 gray codes (H*W,) of g(s0) from a start word: full brick rows, paddle in the last row, ball."""
    paddle, bx, by = unpack_start(word)
    f = np.zeros((H, W), np.uint8)
    f[:brick_rows] |= 4
    f[H - 1, paddle:paddle + paddle_width] |= 1
    f[by, bx] |= 2
    return f.reshape(-1)


def segments(start, T, done, hlen, episode_cap=ActingLoop.MAX_STEPS):
    """Host arrays -> [(env, start_row, end_row, closed)] by env, then start row: env b's rows from a non-zero start
    word up to the next one, or T; the last one is closed iff done[b] or hlen[b] >= episode_cap."""
    start = np.asarray(start)[:T]
    out = []
    for b in range(start.shape[1]):
        rows = np.flatnonzero(start[:, b])
        for i, t0 in enumerate(rows):
            last = i + 1 == len(rows)
            out.append((b, int(t0), T if last else int(rows[i + 1]),
                        bool(done[b] != 0 or hlen[b] >= episode_cap) if last else True))
    return out


def stream_trajectories(rec, T, done, hlen, L_, H, W, episode_cap=ActingLoop.MAX_STEPS, pad_action=0, paddle_width=6,
                        brick_rows=3):
    """A streamed sink's first T rows -> [(env, start_row, closed, ObservationTrajectory)], every segment, by env then
    start row; each trajectory as `trajectories_from_records` builds one (31 pad frames g(s0), here rendered from the
    start word, 32 pad actions, then the segment's records)."""
    rec = {k: v[:T].cpu().numpy() for k, v in rec.items() if v is not None}
    done, hlen = done.cpu().numpy(), hlen.cpu().numpy()
    start = rec["start"].view(np.uint32)
    lut = gray_lut()
    out = []
    for b, t0, t1, closed in segments(start, T, done, hlen, episode_cap):
        m = np.zeros(T, bool)
        m[t0:t1] = rec["mask"][t0:t1, b].astype(bool)
        pad = torch.from_numpy(lut[render_s0(start[t0, b], H, W, paddle_width, brick_rows)].reshape(1, H, W))
        states = [pad] * (L_ - 1)
        if rec.get("frame") is not None:
            states += [torch.from_numpy(lut[f & 7].reshape(1, H, W)) for f in rec["frame"][m, b]]
        rs = np.float32(0)
        for r in rec["reward"][m, b]:
            rs = np.float32(rs + r)
        tr = ObservationTrajectory([pad_action] * L_ + [int(a) for a in rec["action"][m, b]], states,
                                   [0] * L_ + [float(r) for r in rec["reward"][m, b]],
                                   [torch.zeros(3)] * L_ + [torch.from_numpy(c) for c in rec["counts"][m, b]],
                                   [0.0] * L_ + [float(v) for v in rec["values"][m, b]], int(m.sum()), float(rs))
        out.append((b, t0, closed, tr))
    return out


class StreamingStage:
    """`steps` acting rows of cfg's `n_parallel` envs with in-place restarts. Stage i resets every env under the episode
    key ep_base = i * steps and restarts under ep_base + t at row t (1 <= t < steps), so no key is used twice and the
    host knows every key without reading the device. One captured step graph serves every stage: the row comes from
    the loop's step context, (ep_base, episode_cap) from a device block, temperature and noise weight from their
    device words as in ActingStage."""

    def __init__(self, cfg, agent, steps, episode_cap=ActingLoop.MAX_STEPS, seed=0, env_offset=0, use_graph=True,
                 world_size=1, rank=0, pow_threads=None, height=16, width=20):
        if world_size > 1:
            raise NotImplementedError("streaming over ShardedSink: its packed row format has no start word")
        if steps < 1 or episode_cap < 1:
            raise ValueError("StreamingStage: steps and episode_cap must be positive")
        self.cfg, self.steps, self.episode_cap = cfg, int(steps), int(episode_cap)
        B = cfg["n_parallel"]
        self.loop = loop = ActingLoop(cfg, agent, B, seed=seed, env_offset=env_offset, n_envs_total=env_offset + B,
                                      pow_threads=pow_threads, max_steps=self.steps, height=height, width=width)
        dev = agent.device
        loop.rec["start"] = torch.zeros(self.steps, B, dtype=torch.int32, device=dev)  # u32 start words
        self.blk = torch.zeros(2, dtype=torch.int32, device=dev)  # {ep_base, episode_cap}
        loop.restart = self._restart
        self.use_graph = use_graph
        self.ep_base = 0
        self.last_search_id0 = None  # the search id of row 0 of the last stage run

    def _restart(self, loop):
        loop.env.restart(loop.rec["start"], loop.ctx, self.blk)

    @property
    def temperature(self):
        return self.loop.temperature

    @temperature.setter
    def temperature(self, t):
        self.loop.temperature = t  # a device value: the captured step graph stays valid

    def set_noise_weight(self, w):
        self.loop.search.noise_weight = w  # copied to the device before the next step

    def state(self):
        """The host counters a resumed run continues from (between stages nothing else is carried: every stage resets
        all envs under its own key): the next stage's ep_base, the loop's search id and step index, and the search id
        of the last stage's row 0."""
        return {"ep_base": self.ep_base, "search_id": self.loop.search_id, "step_index": self.loop.step_index,
                "last_search_id0": self.last_search_id0}

    def load_state(self, st):
        self.ep_base = int(st["ep_base"])
        self.loop.search_id, self.loop.step_index = int(st["search_id"]), int(st["step_index"])
        self.last_search_id0 = st["last_search_id0"]

    def run(self, replay_buffer=None, trajectories=False, tail="drop"):
        """One stage: reset under ep_base, exactly `steps` steps with no host synchronisation between them, then
        the ingest into `replay_buffer` (its counts: replay_buffer.last_stream) and/or the segments' host
        trajectories (`stream_trajectories`' list; None unless `trajectories`)."""
        loop = self.loop
        self.blk.copy_(torch.tensor([self.ep_base, self.episode_cap], dtype=torch.int32))
        loop.reset(self.ep_base)
        self.ep_base += self.steps  # this stage's restarts use the keys in between
        self.last_search_id0 = loop.search_id  # row t of this stage is searched under this id + t (reanalyse)
        for _ in range(self.steps):
            loop.act()
            if self.use_graph and loop.graph is None and loop.inject_noise is None and loop.noise_log is None:
                loop.capture()
        env = loop.env
        if replay_buffer is not None:
            replay_buffer.ingest_stream(loop.rec, self.steps, env.done, env.hist_len, tail=tail,
                                        episode_cap=self.episode_cap, paddle_width=env.pw, brick_rows=env.brick_rows)
        if trajectories:
            return stream_trajectories(loop.rec, self.steps, env.done, env.hist_len, loop.Lh, loop.H, loop.W,
                                       self.episode_cap, env.pad_action, env.pw, env.brick_rows)
        return None
