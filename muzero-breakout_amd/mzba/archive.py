"""Replay archive: keep streamed sinks, build a window only when it is drawn.

A `DeviceReplayBuffer` stores finished windows, each with its own copy of the frame history (10 660 bytes at 16x20,
L = 32, K = 5); the sink row a window is built from costs 358. `SinkArchive` keeps the last `slabs` streamed stages as
one sink of `slabs * steps` rows, plans it as `ingest_stream` plans a stage, and materialises a list of windows, given or
drawn on the device, into a small ring-shaped staging area the learner trains from:

    archive = SinkArchive(slabs, steps, B, K, seq_len, discount)
    stage.run(); archive.append_stage(stage)                 # instead of stage.run(replay_buffer)
    losses = archive.training_stage(learner, num_batches, minibatch_size)
    archive.refresh(reanalyser, slab)                        # reanalyse: nothing follows, the next gather sees it

`prioritized=True` adds prioritized replay in sink-row space (csrc/archive_prio.hip): a priority per
sink row, set at `append` and `refresh` from |searched value - n-step target|, a device sampler of rows (`sample`) and
the learner's write-back (`update_priorities`); `prioritized_view(B)` lets an unedited `Learner` run its prioritized
step from the archive.

A gathered window is bit-equal to the one `ingest_stream` writes (csrc/replay.hip: mzba_replay_stream_gather runs
mzba_replay_stream_write's window body). Opt-in: nothing else of the package uses it.
"""
import ctypes

import numpy as np
import torch

from . import _lib as L

_KEYS = ("action", "reward", "mask", "counts", "values", "frame", "start")
RING_FIELDS = tuple(k for k, _ in L.ReplayRing._fields_[:8])


class StagedWindows:
    """A replay-ring-shaped holder of `capacity` materialised windows: the eight ring fields in `_ring`, the C ABI's
    view of them, start = 0, max_length = length = capacity. `Learner.train_minibatch` and `Learner.capture` take it
    as `ring`; its tensors are allocated once, so a graph captured on it stays valid across gathers."""

    def __init__(self, capacity, seq_len, K, HW, device):
        cap, dev = int(capacity), device
        self._ring = {
            "past_actions": torch.zeros(cap, seq_len, dtype=torch.int64, device=dev),
            "future_actions": torch.zeros(cap, K, dtype=torch.int64, device=dev),
            "states": torch.zeros(cap, seq_len, HW, dtype=torch.uint8, device=dev),
            "rewards": torch.zeros(cap, K, dtype=torch.float32, device=dev),
            "counts": torch.zeros(cap, K, 3, dtype=torch.float32, device=dev),
            "values": torch.zeros(cap, K, dtype=torch.float32, device=dev),
            "targets": torch.zeros(cap, K, dtype=torch.float32, device=dev),
            "reward_sum": torch.zeros(cap, dtype=torch.float32, device=dev),
        }
        self._abi = L.ReplayRing(*(self._ring[k].data_ptr() for k in RING_FIELDS), cap, K, seq_len)
        self.capacity = self.max_length = self.length = cap
        self.start = 0

    def __len__(self):
        return self.length


class SinkArchive:
    """The last `slabs` streamed stages of B envs and `steps` rows each, as one streamed sink.

    Stage sink number i lands in rows [(i % slabs) * steps, ...): the oldest slab is overwritten. The tensors are
    zero-initialised and allocated once; a zero mask is "no record" and a zero start word "no episode starts here",
    so an unfilled slab plans to nothing and the archive is always planned whole. Segments never cross a slab: a
    stage has a start word for every env at its row 0.

    The tail rule is applied once, at `append`, in the archive's copy: with tail="drop" the mask of the last
    segment's rows is cleared for every env that is not closed at the end of the stage (closed = done[b] or
    hlen[b] >= episode_cap, `ingest_stream`'s rule), with tail="keep" nothing is. The archive is then planned with
    every last segment closed.

    prioritized=True keeps q f32[T * B] beside the sink, indexed row * B + env: (|value - n-step target| + prio_eps)
    ** alpha at the root record of every window, exactly 0 at every other row. A root's row does not move when other
    slabs are appended; the sampler draws rows and looks their windows up in the table of the moment. The one
    ordering rule, as for the ring: no `append` or `refresh` between a `sample` and its `update_priorities`.

    Not supported: lockstep (`frame0`) sinks, sharded sinks, an open tail carried into the next stage."""

    def __init__(self, slabs, steps, B, K, seq_len, discount, height=16, width=20, min_len=None, episode_cap=261,
                 paddle_width=6, brick_rows=3, device="cuda", prioritized=False, alpha=1.0, beta=1.0, prio_eps=1e-3):
        L.require_gpu()
        if slabs < 1 or steps < 1 or B < 1:
            raise ValueError("SinkArchive: slabs, steps and B must be positive")
        self.slabs, self.steps, self.B, self.K, self.hist_seq_len = int(slabs), int(steps), int(B), int(K), int(seq_len)
        self.discount, self.H, self.W = discount, int(height), int(width)
        self.min_len = K + 1 if min_len is None else int(min_len)
        self.episode_cap, self.paddle_width, self.brick_rows = int(episode_cap), int(paddle_width), int(brick_rows)
        self.device = dev = torch.device(device)
        T, HW = self.slabs * self.steps, self.H * self.W
        if T * self.B >= 2 ** 31:
            raise ValueError("SinkArchive: slabs * steps * B must stay below 2^31 rows")
        self.T = T
        self.rec = {
            "action": torch.zeros(T, B, dtype=torch.uint8, device=dev),
            "reward": torch.zeros(T, B, dtype=torch.float32, device=dev),
            "mask": torch.zeros(T, B, dtype=torch.uint8, device=dev),
            "counts": torch.zeros(T, B, 3, dtype=torch.int64, device=dev),
            "values": torch.zeros(T, B, dtype=torch.float32, device=dev),
            "frame": torch.zeros(T, B, HW, dtype=torch.uint8, device=dev),
            "start": torch.zeros(T, B, dtype=torch.int32, device=dev),  # u32 start words
        }
        self._sink = L.sink(self.rec, T, HW)
        # the plan's workspace and table: fixed addresses, read by every (captured) gather
        self.nmax = B * (T // max(self.min_len + 1, K))
        self._cnt = torch.zeros(B, 2, dtype=torch.int32, device=dev)
        self._offs = torch.zeros(B + 1, 2, dtype=torch.int32, device=dev)
        self._table = torch.zeros(6, self.nmax + 1, dtype=torch.int32, device=dev)
        self._totals = self._offs[B]  # {kept segments, windows}, read on the device by the gather
        self._closed = torch.ones(B, dtype=torch.uint8, device=dev)
        self._hlen0 = torch.zeros(B, dtype=torch.int32, device=dev)
        self._rows = torch.arange(self.steps, device=dev).unsqueeze(1)
        # dpow[k] = f32(discount ** k), k <= T, then f32(discount ** K): python double pow, DeviceReplayBuffer._powers
        tab = [discount ** k for k in range(T + 1)] + [discount ** K]
        self._dpow = torch.tensor(np.array(tab, dtype=np.float64).astype(np.float32), device=dev)
        self.appended = 0     # stage sinks given so far
        self.segments = 0     # kept segments of the archive as planned last
        self.windows = 0      # ... and their windows
        self.search_id0 = [None] * self.slabs
        self.draw_step = 0    # the Philox step of training_stage's next gather
        self._staged = {}
        self.prioritized = bool(prioritized)
        self.alpha, self.beta, self.prio_eps = float(alpha), float(beta), float(prio_eps)
        self._q = torch.zeros(T * B, dtype=torch.float32, device=dev) if self.prioritized else None
        self._sample_ws = {}
        self._views = {}

    def __len__(self):
        return self.windows

    # -- storage ------------------------------------------------------------------------------------------
    def slab_rec(self, slab):
        """The sink dict of one slab: views of its `steps` rows."""
        r0 = int(slab) * self.steps
        return {k: v[r0:r0 + self.steps] for k, v in self.rec.items()}

    def stored_bytes(self):
        """Bytes of the seven sink tensors."""
        return sum(v.numel() * v.element_size() for v in self.rec.values())

    def _plan(self):
        L.call("mzba_replay_stream_plan", ctypes.byref(self._sink), L.ptr(self._closed), L.ptr(self._hlen0), self.K,
               self.min_len, self.episode_cap, 1, L.ptr(self._cnt), L.ptr(self._offs), L.ptr(self._table), self.nmax,
               L.stream())

    def append(self, rec, T, done, hlen, tail="drop", search_id0=None):
        """A streamed stage's sink (`ingest_stream`'s rec, done, hlen) into the oldest slab: copy the rows, apply the
        tail rule, plan the whole archive. One host read (the totals, into `segments` / `windows`). -> the slab."""
        if tail not in ("drop", "keep"):
            raise ValueError("tail must be 'drop' or 'keep'")
        if rec.get("frame") is None or rec.get("start") is None:
            raise ValueError("SinkArchive.append needs the sink's recorded frames and start words")
        if T != self.steps:
            raise ValueError(f"SinkArchive.append: T = {T}, the archive's slabs hold {self.steps} rows")
        if rec["action"].shape[1] != self.B or rec["frame"].shape[-1] != self.H * self.W:
            raise ValueError("SinkArchive.append: the sink's envs or frame size are not the archive's")
        slab = self.appended % self.slabs
        mine = self.slab_rec(slab)
        for k in _KEYS:
            src = rec[k][:T]
            mine[k].copy_(src.view(torch.int32) if k == "start" and src.dtype != torch.int32 else src)
        if tail == "drop":
            rows = self._rows
            last = torch.where(mine["start"] != 0, rows, -1).amax(0)  # the last segment's start row, -1: none
            is_open = ~((done.to(self.device) != 0) | (hlen.to(self.device) >= self.episode_cap))
            mine["mask"].masked_fill_((rows >= last) & (is_open & (last >= 0)), 0)
        self._plan()
        self.segments, self.windows = self._totals.tolist()
        self.search_id0[slab] = search_id0
        self.appended += 1
        if self.prioritized:  # the evicted stage's priorities go, the other slabs' learned ones stay
            self.reprioritize(slab)
        return slab

    def append_stage(self, stage, tail="drop"):
        """`append` from a `StreamingStage` after its run()."""
        loop = stage.loop
        env = loop.env
        if (env.pw, env.brick_rows) != (self.paddle_width, self.brick_rows):
            raise ValueError("SinkArchive.append_stage: the env's paddle_width / brick_rows are not the archive's")
        if stage.episode_cap != self.episode_cap:
            raise ValueError("SinkArchive.append_stage: the stage's episode_cap is not the archive's")
        return self.append(loop.rec, stage.steps, env.done, env.hist_len, tail=tail,
                           search_id0=stage.last_search_id0)

    # -- checkpoint (mzba.train.Trainer.save / load) --------------------------------------------------------
    def state(self, sinks=True):
        """What a resumed run needs, as host tensors and plain values: the seven sink tensors (sinks=False: None, the
        resume then starts from an empty archive), `appended`, `search_id0`, `draw_step`, and `q` when prioritized. The
        plan is not stored: `load_state` plans again."""
        return {"rec": {k: v.cpu() for k, v in self.rec.items()} if sinks else None,
                "q": self._q.cpu() if sinks and self.prioritized else None,
                "appended": self.appended, "search_id0": list(self.search_id0), "draw_step": self.draw_step,
                "shape": [self.slabs, self.steps, self.B, self.H * self.W], "prioritized": self.prioritized}

    def load_state(self, st):
        """Inverse of `state` into this archive's own tensors (their addresses stay, so captured gathers stay valid),
        then the plan and its one host read. Without sink tensors the archive is emptied; `draw_step` is kept either
        way, so no draw of the saved run is repeated."""
        if list(st["shape"]) != [self.slabs, self.steps, self.B, self.H * self.W]:
            raise ValueError(f"SinkArchive.load_state: saved shape {list(st['shape'])} is not this archive's")
        if st["rec"] is not None and bool(st["prioritized"]) != self.prioritized:
            raise ValueError("SinkArchive.load_state: the saved archive's prioritized flag is not this archive's")
        if st["rec"] is None:
            for v in self.rec.values():
                v.zero_()
            self.appended, self.search_id0 = 0, [None] * self.slabs
            if self.prioritized:
                self._q.zero_()
        else:
            for k, v in self.rec.items():
                v.copy_(st["rec"][k])
            self.appended, self.search_id0 = int(st["appended"]), list(st["search_id0"])
            if self.prioritized:
                self._q.copy_(st["q"])
        self.draw_step = int(st["draw_step"])
        self._plan()
        self.segments, self.windows = self._totals.tolist()

    # -- windows on draw ----------------------------------------------------------------------------------
    def staged(self, capacity):
        """The archive's own staging area of `capacity` windows (one per capacity, kept)."""
        st = self._staged.get(capacity)
        if st is None:
            st = self._staged[capacity] = StagedWindows(capacity, self.hist_seq_len, self.K, self.H * self.W,
                                                        self.device)
        return st

    def gather(self, n, idx=None, step=0, seed=0, step_dev=None, slot0=0, out=None):
        """Materialise n windows -> (staged, slots, idx_out). `idx` (device i32[n]) lists archive windows, in
        [0, windows); without it window i is drawn as ((u64)x * windows) >> 32 with x the first word of Philox
        (i, stream 6, step, 0) under `seed` (`step_dev`, a device i32 / u32 [1], overrides `step`: a captured gather
        draws afresh on every replay, and follows later appends, because the counts are read on the device). Window i
        lands in row slot0 + i of `out` (a StagedWindows, default the archive's own of capacity slot0 + n); slots =
        slot0 + arange(n) i32; idx_out i32[n] = the window written, -1 for a listed index outside the archive, whose
        row is left as it was. No host read."""
        n, slot0 = int(n), int(slot0)
        if idx is None and self.windows == 0:
            raise ValueError("draw from an empty archive")
        if idx is not None:
            if idx.dtype != torch.int32 or not idx.is_cuda or idx.numel() != n:
                raise ValueError("idx must be a device int32 tensor of n window indices")
            idx = idx.contiguous()
        if step_dev is not None and (step_dev.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32))
                                     or not step_dev.is_cuda):
            raise ValueError("step_dev must be a device int32 / uint32 tensor")
        st = self.staged(slot0 + n) if out is None else out
        idx_out = torch.empty(n, dtype=torch.int32, device=self.device)
        L.call("mzba_replay_stream_gather", ctypes.byref(self._sink), self.H, self.W, self.paddle_width,
               self.brick_rows, L.ptr(self._table), self.nmax, L.ptr(self._totals), L.ptr(idx), n, int(seed),
               int(step) & 0xFFFFFFFF, L.ptr(step_dev), ctypes.byref(st._abi), slot0, L.ptr(self._dpow),
               L.ptr(idx_out), L.stream())
        slots = torch.arange(slot0, slot0 + n, dtype=torch.int32, device=self.device)
        return st, slots, idx_out

    def training_stage(self, learner, num_batches, minibatch_size, seed=0, prioritized=False):
        """num_batches minibatches of drawn windows: one gather of num_batches * minibatch_size windows under the
        archive's own draw step (advanced here, so no two stages share draws), then learner.train_minibatch on each
        chunk of the staged rows (the learner's captured graph where one was captured for that holder:
        learner.capture(archive.staged(num_batches * minibatch_size), minibatch_size)). The only host read is that
        of the losses at the end. -> the per-minibatch losses (host floats).

        prioritized=True: num_batches prioritized steps instead (learner.prioritized_step on
        prioritized_view(minibatch_size): sample rows, gather their windows, the weighted minibatch, update the
        rows' priorities; the captured graph where learner.capture(view, minibatch_size, prioritized=True, seed) was
        called), under the learner's own step counter."""
        if prioritized:
            view = self.prioritized_view(minibatch_size)
            losses = [learner.prioritized_step(view, minibatch_size, seed).clone() for _ in range(num_batches)]
            return [float(x[0]) for x in losses]
        n = int(num_batches) * int(minibatch_size)
        st, slots, _ = self.gather(n, step=self.draw_step, seed=seed)
        self.draw_step += 1
        losses = [learner.train_minibatch(st, slots[i * minibatch_size:(i + 1) * minibatch_size]).clone()
                  for i in range(num_batches)]
        return [float(x[0]) for x in losses]

    # -- reanalyse ----------------------------------------------------------------------------------------
    def refresh(self, reanalyser, slab, rows=None, noise_weight=None, use_graph=True):
        """`reanalyser.refresh_stream` on the rows of one slab (views of the archive's tensors), under the search
        id the slab was appended with. Nothing follows it: the next `gather` computes counts, values and n-step
        targets from the refreshed rows. Rows whose mask the tail rule cleared are searched but not written
        (mzba_record_results_masked). The reanalyser's captured row holds the sink's addresses in its key, so it is
        captured again when the slab changes. -> rows searched."""
        slab = int(slab)
        if not 0 <= slab < min(self.appended, self.slabs):
            raise ValueError(f"SinkArchive.refresh: slab {slab} holds no stage")
        if self.search_id0[slab] is None:
            raise ValueError(f"SinkArchive.refresh: slab {slab} was appended without its search_id0")
        n = reanalyser.refresh_stream(self.slab_rec(slab), self.steps, self.search_id0[slab], rows=rows,
                                      noise_weight=noise_weight, use_graph=use_graph)
        if self.prioritized:  # Appendix G: reanalyse writes priorities
            self.reprioritize(slab)
        return n

    # -- prioritized replay in sink-row space (csrc/archive_prio.hip) -----------------------
    def _need_prio(self):
        if not self.prioritized:
            raise RuntimeError("this SinkArchive was built with prioritized=False")

    def reprioritize(self, slab):
        """The init rule over the rows of one slab: q = (|value - n-step target| + prio_eps) ** alpha at every root
        record, 0 elsewhere, from the sink and the plan as they are now. `append` and `refresh` call it."""
        self._need_prio()
        slab = int(slab)
        if not 0 <= slab < self.slabs:
            raise ValueError(f"SinkArchive.reprioritize: no slab {slab}")
        L.call("mzba_archive_priority_init", ctypes.byref(self._sink), L.ptr(self._table), self.nmax,
               L.ptr(self._offs), L.ptr(self._totals), L.ptr(self._q), slab * self.steps, self.steps, self.K,
               L.ptr(self._dpow), self.alpha, self.prio_eps, L.stream())

    def _sample_workspace(self, n):
        """The sampler's scratch for n samples, kept per n (allocate it before a graph capture that samples)."""
        self._need_prio()
        ws = self._sample_ws.get(n)
        if ws is None:
            nbytes = L.lib().mzba_archive_sample_ws_bytes(self.T * self.B, n)
            ws = self._sample_ws[n] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    def sample(self, n, step, seed=0, u=None, step_dev=None):
        """n windows drawn in proportion to their priorities (stratified: sample j from the j-th n-th of the mass), on
        the device with no host round trip -> (rows i32[n] sink rows row * B + env, idx i32[n] their windows for
        `gather`, weights f32[n] = (windows * P) ** -beta over the batch's largest, probs f32[n]). The draws are 53-bit
        Philox uniforms (j, stream 7, step, 0) under `seed`; `step_dev` (device i32/u32 [1]) overrides `step`; `u`
        (device f64[n] in [0, 1)) replaces the draws. The window count is read on the device, so a captured sample
        follows later appends. A draw that cannot be used (no priority mass; a row that is no root any more) gives
        rows = idx = -1 and weight 0."""
        self._need_prio()
        n, dev = int(n), self.device
        rows = torch.empty(n, dtype=torch.int32, device=dev)
        idx = torch.empty(n, dtype=torch.int32, device=dev)
        probs = torch.empty(n, dtype=torch.float32, device=dev)
        weights = torch.empty(n, dtype=torch.float32, device=dev)
        if u is not None:
            u = u.to(device=dev, dtype=torch.float64).contiguous()
            if u.numel() != n:
                raise ValueError("u must hold one draw per sample")
        if step_dev is not None and (step_dev.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32))
                                     or not step_dev.is_cuda):
            raise ValueError("step_dev must be a device int32 / uint32 tensor")
        ws = self._sample_workspace(n)
        L.call("mzba_archive_sample", L.ptr(self._q), self.T * self.B, n, self.beta, 0, L.ptr(self._table), self.nmax,
               L.ptr(self._offs), L.ptr(self._totals), self.B, self.K, int(seed), int(step) & 0xFFFFFFFF,
               L.ptr(step_dev), L.ptr(u), L.ptr(rows), L.ptr(idx), L.ptr(probs), L.ptr(weights), L.ptr(ws), ws.numel(),
               L.stream())
        return rows, idx, weights, probs

    def update_priorities(self, rows, td, guard_block=None):
        """q[rows[j]] = (td[j] + prio_eps) ** alpha (td: the learner's last_td for the windows of a `sample`; a row of
        -1 is skipped). No append or refresh may run between the sample and this call; duplicates are the same
        window and carry equal td. guard_block (a guarded Learner's device stats block): q stays as it is when that
        step was skipped."""
        self._need_prio()
        if rows.dtype != torch.int32 or td.dtype != torch.float32 or rows.numel() != td.numel():
            raise ValueError("update_priorities takes i32 rows and f32 td of one length")
        rows, td = rows.contiguous(), td.contiguous()  # held until the launch is made
        if guard_block is not None:
            L.call("mzba_replay_priority_update_g", L.ptr(self._q), L.ptr(rows), L.ptr(td), rows.numel(),
                   self.T * self.B, self.alpha, self.prio_eps, L.ptr(guard_block), L.stream())
            return
        L.call("mzba_replay_priority_update", L.ptr(self._q), L.ptr(rows), L.ptr(td), rows.numel(), self.T * self.B,
               self.alpha, self.prio_eps, L.stream())

    def root_rows(self):
        """Sink row (row * B + env, device i64) of every window's root record, in archive window order."""
        ns = self.segments
        env, t0, ln, woff = (self._table[k, :ns].long() for k in (0, 1, 2, 5))
        seg = torch.repeat_interleave(torch.arange(ns, device=self.device), ln - self.K + 1)
        s = torch.arange(seg.numel(), device=self.device) - woff[seg]
        return (t0[seg] + s) * self.B + env[seg]

    def priorities(self):
        """q = p ** alpha at the windows' root records, in archive window order (f32 device tensor)."""
        self._need_prio()
        return self._q[self.root_rows()]

    def prioritized_view(self, B):
        """The ring-shaped object (one per B, kept) that runs an unedited Learner's prioritized step from the archive:
        Learner.capture(view, B, prioritized=True, seed), Learner.prioritized_step(view, B, seed),
        Learner.training_stage(view, ..., prioritized=True)."""
        self._need_prio()
        view = self._views.get(B)
        if view is None:
            view = self._views[B] = PrioritizedView(self, int(B))
        return view


class PrioritizedView:
    """`SinkArchive.staged(B)` with a prioritized ring's sampling surface: `sample` draws B rows of the archive,
    gathers their windows into the staged rows 0 .. B - 1 and remembers the rows; `update_priorities` writes to them.
    An unusable draw (weight 0) leaves its staged row as it was."""

    def __init__(self, archive, B):
        self.archive, self.B = archive, B
        self.staged = archive.staged(B)
        self._ring, self._abi = self.staged._ring, self.staged._abi
        self._slots = torch.arange(B, dtype=torch.int32, device=archive.device)
        self.rows = None

    def _sample_workspace(self, B):
        return self.archive._sample_workspace(B)

    def sample(self, B, step, seed=0, step_dev=None):
        if B != self.B:
            raise ValueError(f"this view stages {self.B} windows, not {B}")
        rows, idx, weights, probs = self.archive.sample(B, step, seed=seed, step_dev=step_dev)
        self.archive.gather(B, idx=idx, out=self.staged)
        self.rows = rows
        return self._slots, weights, probs

    def update_priorities(self, slots, td, guard_block=None):
        self.archive.update_priorities(self.rows, td, guard_block=guard_block)
