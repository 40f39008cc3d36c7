"""Device replay buffer: drop-in for replay_buffer.py:ReplayBuffer.

The windows the reference builds in a Python triple loop (`save_observation_trajectory`,
replay_buffer.py:96-165) are built on the device (csrc/replay.hip) straight from the acting
loop's sink (`ingest_records`; `ingest_stream` for a streamed stage's sink of several episodes per
env) or from host `ObservationTrajectory` objects
(`save_observation_trajectory`, same arithmetic). Storage is a FIFO ring of `max_length`
fixed-size rows in HBM (frames as u8 gray codes, 10 KB per window at 16x20); the getters
return device tensors with the reference's dtypes and shapes.

`prioritized=True` adds MuZero's prioritized replay (Appendix G; csrc/replay_prio.hip): a
priority array beside the ring, set at ingest from |searched value - n-step target|, a device sampler
(`sample`) and the learner's write-back (`update_priorities`). Off by default; nothing else changes.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib as L
from .env import gray_lut

# What `ingest_records` leaves in `last_ingest` for a later `reingest_records`: the ring slot of the
# ingest's window 0, its window count (evicted-at-once ones included), the serial of window 0 (a count of every
# window the buffer was given in its epoch, so it only grows) and that epoch (`empty_buffer` starts a new one).
IngestHandle = collections.namedtuple("IngestHandle", "head n serial epoch")
# The same for `ingest_stream` / `reingest_stream`, with the kept segments' count and what the ingest
# planned with, so that the reingest plans the same table.
StreamHandle = collections.namedtuple("StreamHandle", "head n segments serial epoch tail min_len episode_cap")


def live_windows(serial, n, written, length):
    """Which windows of an ingest are still in the ring: the ingest gave windows with serials [serial, serial + n),
    the ring holds the newest `length` of the `written` windows given so far, serials [written - length, written).
    -> (j_first, count): the live windows are j in [j_first, j_first + count), count = 0 when none is."""
    j_first = max(0, written - length - serial)
    return (j_first, n - j_first) if j_first < n else (n, 0)


class DeviceReplayBuffer:
    """ReplayBuffer(seq_len, K, max_length, discount, num_rewards_to_sum) (replay_buffer.py:76-92)."""

    def __init__(self, seq_len, K, max_length, discount, num_rewards_to_sum, height=16, width=20, device="cuda",
                 prioritized=False, alpha=1.0, beta=1.0, prio_eps=1e-3):
        L.require_gpu()
        self.hist_seq_len, self.K, self.max_length = seq_len, K, max_length
        self.discount, self.num_rewards_to_sum = discount, num_rewards_to_sum
        self.H, self.W = height, width
        self.device = torch.device(device)
        cap, dev = max_length, self.device
        self._ring = {
            "past_actions": torch.zeros(cap, seq_len, dtype=torch.int64, device=dev),
            "future_actions": torch.zeros(cap, K, dtype=torch.int64, device=dev),
            "states": torch.zeros(cap, seq_len, height * width, dtype=torch.uint8, device=dev),
            "rewards": torch.zeros(cap, K, dtype=torch.float32, device=dev),
            "counts": torch.zeros(cap, K, 3, dtype=torch.float32, device=dev),
            "values": torch.zeros(cap, K, dtype=torch.float32, device=dev),
            "targets": torch.zeros(cap, K, dtype=torch.float32, device=dev),
            "reward_sum": torch.zeros(cap, dtype=torch.float32, device=dev),
        }
        # the C ABI's view of the ring (include/mzba.h mzba_replay_ring): the rows are never reallocated
        self._abi = L.ReplayRing(*(self._ring[k].data_ptr() for k, _ in L.ReplayRing._fields_[:8]), cap, K, seq_len)
        self._lut = torch.from_numpy(gray_lut()).to(dev)
        self.start = 0      # ring slot of the oldest window
        self.length = 0     # windows stored (replay_buffer.py:87)
        self._dpow = {}
        # prioritized replay: q[slot] = p^alpha of a live window, exactly 0 for a slot that holds none (slot space,
        # so the sampler needs neither start nor length); kept outside _ring, which other ring holders imitate
        self.prioritized = bool(prioritized)
        self.alpha, self.beta, self.prio_eps = float(alpha), float(beta), float(prio_eps)
        self._q = torch.zeros(cap, dtype=torch.float32, device=dev) if self.prioritized else None
        self._sample_ws = {}
        # reanalyse bookkeeping: windows given to the ring in this epoch, the epoch, the last ingests' handles
        self._written = 0
        self._epoch = 0
        self.last_ingest = None
        self.last_stream_ingest = None

    def __len__(self):
        return self.length

    # -- ingest ------------------------------------------------------------------------
    def _powers(self, T):
        if T not in self._dpow:
            d = self.discount
            tab = [d ** k for k in range(T + 1)] + [d ** self.K]  # python double pow, as the reference
            self._dpow[T] = torch.tensor(np.array(tab, dtype=np.float64).astype(np.float32), device=self.device)
        return self._dpow[T]

    def ingest_records(self, rec, frame0, T, min_len=None):
        """Every trajectory of an acting-loop episode batch: rec = the loop's sink dict of
        (T_max, B, ...) device tensors (first T rows used), frame0 u8 [B][H*W] = g(s0) codes.
        Trajectories with length <= min_len (default K + 1, train_torch.py:224) are skipped;
        the rest are saved in env order, like the reference's loop over trajectories."""
        min_len = self.K + 1 if min_len is None else min_len
        B = rec["action"].shape[1]
        HW = self.H * self.W
        if rec.get("frame") is None:
            raise ValueError("ingest_records needs the loop's recorded frames (record_frames=True)")
        dev = self.device
        lens = torch.empty(B, dtype=torch.int32, device=dev)
        rsum = torch.empty(B, dtype=torch.float32, device=dev)
        offs = torch.empty(B + 1, dtype=torch.int32, device=dev)
        sk = ctypes.byref(L.sink(rec, T, HW))
        L.call("mzba_replay_plan", sk, L.ptr(frame0), self.K, min_len, L.ptr(lens), L.ptr(rsum), L.ptr(offs),
               L.stream())
        n = int(offs[B].item())
        head = (self.start + self.length) % self.max_length
        L.call("mzba_replay_write", sk, L.ptr(frame0), L.ptr(lens), L.ptr(rsum), L.ptr(offs), n,
               ctypes.byref(self._abi), head, L.ptr(self._powers(T)), L.stream())
        self.last_ingest = IngestHandle(head, n, self._written, self._epoch)
        self._commit(head, n)
        return n

    def reingest_records(self, handle, rec, frame0, T, min_len=None):
        """After the sink of an earlier `ingest_records` (its `last_ingest` handle, the same rec layout, frame0, T
        and min_len) had its counts and values refreshed (mzba.reanalyse.Reanalyser): rewrite counts, values and
        n-step targets of the ingest's windows that are still in the ring, and with prioritized=True their
        priorities by the ingest rule. Windows evicted since are skipped (their slots hold newer windows); start and
        length do not change. The same ordering rule as an ingest: none between a sample and its
        update_priorities. -> windows rewritten (0 for an evicted or pre-empty_buffer handle)."""
        if handle is None or handle.epoch != self._epoch:
            return 0
        j_first, count = live_windows(handle.serial, handle.n, self._written, self.length)
        if count == 0:
            return 0
        min_len = self.K + 1 if min_len is None else min_len
        B = rec["action"].shape[1]
        dev = self.device
        lens = torch.empty(B, dtype=torch.int32, device=dev)
        rsum = torch.empty(B, dtype=torch.float32, device=dev)
        offs = torch.empty(B + 1, dtype=torch.int32, device=dev)
        sk = ctypes.byref(L.sink(rec, T, self.H * self.W))
        L.call("mzba_replay_plan", sk, L.ptr(frame0), self.K, min_len, L.ptr(lens), L.ptr(rsum), L.ptr(offs),
               L.stream())
        n = int(offs[B].item())
        if n != handle.n:
            raise ValueError(f"reingest_records: the sink plans {n} windows, the handle's ingest wrote {handle.n}")
        L.call("mzba_replay_rewrite", sk, L.ptr(frame0), L.ptr(lens), L.ptr(rsum), L.ptr(offs), n, j_first,
               ctypes.byref(self._abi), handle.head, L.ptr(self._powers(T)), L.stream())
        if self.prioritized:  # the ingest rule over slots (head + j) % cap, j in [j_first, n)
            self._init_priorities((handle.head + j_first) % self.max_length, n - j_first)
        return count

    def _commit(self, head, n):
        """The ring's bookkeeping after n windows were written from slot `head` on (the newest max_length kept)."""
        cap = self.max_length
        if self.prioritized:
            self._init_priorities(head, n)
        self._written += n
        total = self.length + n
        self.length = min(total, cap)
        self.start = (self.start + total - self.length) % cap

    def _plan_stream(self, rec, T, done, hlen, tail, min_len, episode_cap):
        """The segment table of a streamed sink -> (sink, table, nmax, segments, windows). One host read."""
        B = rec["action"].shape[1]
        dev = self.device
        nmax = B * (T // max(min_len + 1, self.K))
        cnt = torch.empty(B, 2, dtype=torch.int32, device=dev)
        offs = torch.empty(B + 1, 2, dtype=torch.int32, device=dev)
        table = torch.empty(6, nmax + 1, dtype=torch.int32, device=dev)
        sink = L.sink(rec, T, self.H * self.W)
        L.call("mzba_replay_stream_plan", ctypes.byref(sink), L.ptr(done), L.ptr(hlen), self.K, min_len,
               int(episode_cap), 1 if tail == "keep" else 0, L.ptr(cnt), L.ptr(offs), L.ptr(table), nmax, L.stream())
        nseg, n = offs[B].tolist()
        return sink, table, nmax, nseg, n

    def ingest_stream(self, rec, T, done, hlen, tail="drop", min_len=None, episode_cap=261, paddle_width=6,
                      brick_rows=3):
        """A streamed stage's sink (mzba.stream.StreamingStage): `rec` as for ingest_records plus rec["start"], the
        (T_max, B) start words; `done` u8 [B] and `hlen` i32 [B] are the envs' flags at the end of the stage. A
        segment (one env's rows from a start word up to the next one, or T) is a trajectory: pad frames g(s0)
        rendered from its start word, then its records. An env's last segment is closed iff done[b] or hlen[b] >=
        episode_cap; an open one is dropped (tail="drop") or ingested as a truncated trajectory (tail="keep"). Kept
        segments (length > min_len, default K + 1, and >= K) are saved by env, then by start row, so a sink with
        one closed segment per env fills the ring exactly as ingest_records does. One host read. -> windows.
        Leaves `last_stream` (the counts) and `last_stream_ingest` (the handle of a later `reingest_stream`)."""
        if tail not in ("drop", "keep"):
            raise ValueError("tail must be 'drop' or 'keep'")
        if rec.get("frame") is None or rec.get("start") is None:
            raise ValueError("ingest_stream needs the sink's recorded frames and start words")
        min_len = self.K + 1 if min_len is None else min_len
        sink, table, nmax, nseg, n = self._plan_stream(rec, T, done, hlen, tail, min_len, episode_cap)
        head = (self.start + self.length) % self.max_length
        L.call("mzba_replay_stream_write", ctypes.byref(sink), self.H, self.W, paddle_width, brick_rows, L.ptr(table),
               nmax, nseg, n, ctypes.byref(self._abi), head, L.ptr(self._powers(T)), L.stream())
        self.last_stream_ingest = StreamHandle(head, n, nseg, self._written, self._epoch, tail, min_len,
                                               int(episode_cap))
        self._commit(head, n)
        # a segment of L records gives L - K + 1 windows: the kept rows are windows + segments * (K - 1)
        self.last_stream = {"segments": nseg, "windows": n}
        return n

    def reingest_stream(self, handle, rec, T, done, hlen, paddle_width=6, brick_rows=3):
        """`reingest_records` for a streamed sink: after the sink of an earlier `ingest_stream` (its
        `last_stream_ingest` handle; the same rec layout and T, `done` / `hlen` as they were at that ingest,
        Reanalyser.snapshot_stream keeps them) had its counts and values refreshed (Reanalyser.refresh_stream):
        rewrite counts, values and n-step targets of the ingest's windows that are still in the ring, and with
        prioritized=True their priorities by the ingest rule. The sink is planned again with the handle's tail,
        min_len and episode_cap (mask, reward and start words are never written, so the table is the ingest's);
        ValueError if it plans other segments or windows than the handle's. start and length do not change; the
        ordering rules are reingest_records'. No frame is rendered: paddle_width and brick_rows, ingest_stream's
        arguments, are accepted and not used. -> windows rewritten (0 for an evicted or pre-empty_buffer handle)."""
        if handle is None or handle.epoch != self._epoch:
            return 0
        j_first, count = live_windows(handle.serial, handle.n, self._written, self.length)
        if count == 0:
            return 0
        if rec.get("start") is None:
            raise ValueError("reingest_stream needs the sink's start words")
        sink, table, nmax, nseg, n = self._plan_stream(rec, T, done, hlen, handle.tail, handle.min_len,
                                                       handle.episode_cap)
        if (nseg, n) != (handle.segments, handle.n):
            raise ValueError(f"reingest_stream: the sink plans {nseg} segments and {n} windows, the handle's ingest "
                             f"wrote {handle.segments} and {handle.n}")
        L.call("mzba_replay_stream_rewrite", ctypes.byref(sink), L.ptr(table), nmax, nseg, n, j_first,
               ctypes.byref(self._abi), handle.head, L.ptr(self._powers(T)), L.stream())
        if self.prioritized:  # the ingest rule over slots (head + j) % cap, j in [j_first, n)
            self._init_priorities((handle.head + j_first) % self.max_length, n - j_first)
        return count

    def save_observation_trajectory(self, observation_trajectory):
        """replay_buffer.py:96-165 for one host trajectory (padded as _pad_initial_state builds it)."""
        t = observation_trajectory
        h, Lr = self.hist_seq_len, t.length
        if Lr == 0:
            return
        inv = {float(v): c for c, v in reversed(list(enumerate(gray_lut())))}

        def codes(img):
            a = np.asarray(img.cpu() if torch.is_tensor(img) else img, dtype=np.float32).reshape(-1)
            try:
                return np.array([inv[float(x)] for x in a], dtype=np.uint8)
            except KeyError as e:
                raise ValueError(f"state value {e} is not a convert_to_grayscale output") from None

        dev = self.device
        T = Lr
        tensor = lambda x, dt: torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)  # noqa: E731
        rec = {
            "action": tensor(np.array([int(a) for a in t.actions[h:]], np.uint8).reshape(T, 1), torch.uint8),
            "reward": tensor(np.array([float(r) for r in t.rewards[h:]], np.float32).reshape(T, 1), torch.float32),
            "mask": torch.ones(T, 1, dtype=torch.uint8, device=dev),
            "counts": tensor(np.stack([np.asarray(c.cpu() if torch.is_tensor(c) else c) for c in
                                       t.visit_counts[h:]]).astype(np.int64).reshape(T, 1, 3), torch.int64),
            "values": tensor(np.array([float(v) for v in t.values[h:]], np.float32).reshape(T, 1), torch.float32),
            "frame": tensor(np.stack([codes(s) for s in t.states[h - 1:]]).reshape(T, 1, -1), torch.uint8),
        }
        frame0 = tensor(codes(t.states[0]).reshape(1, -1), torch.uint8)
        self.ingest_records(rec, frame0, T, min_len=-1)

    # -- getters (replay_buffer.py:167-225) --------------------------------------------------
    def _slots(self, batch_idxs):
        idx = torch.as_tensor(batch_idxs, device=self.device).to(torch.int64)
        if idx.numel():
            lo, hi = torch.stack([idx.min(), idx.max()]).tolist()
            if lo < 0 or hi >= self.length:
                raise IndexError("replay index out of range")
        return (idx + self.start) % self.max_length

    def get_batched_past_actions(self, batch_idxs):
        return self._ring["past_actions"][self._slots(batch_idxs)]

    def get_batched_future_actions(self, batch_idxs):
        return self._ring["future_actions"][self._slots(batch_idxs)]

    def get_batched_states(self, batch_idxs):
        """[batch, hist, 1, H, W] f32 grayscale (the stacked (1, H, W) frames)."""
        slots = self._slots(batch_idxs).to(torch.int32)
        n = slots.numel()
        out = torch.empty(n, self.hist_seq_len, 1, self.H, self.W, dtype=torch.float32, device=self.device)
        L.call("mzba_replay_states", L.ptr(self._ring["states"]), L.ptr(slots), n, L.ptr(self._lut), L.ptr(out),
               self.hist_seq_len, self.H * self.W, L.stream())
        return out

    def get_batched_rewards(self, batch_idxs):
        return self._ring["rewards"][self._slots(batch_idxs)]

    def get_batched_visit_counts(self, batch_idxs):
        return self._ring["counts"][self._slots(batch_idxs)]

    def get_batched_values(self, batch_idxs):
        """The bootstrapped n-step value targets (replay_buffer.py:209-214)."""
        return self._ring["targets"][self._slots(batch_idxs)]

    def get_values(self, batch_idxs):
        """value_buffer rows (the searched root values) — kept for inspection."""
        return self._ring["values"][self._slots(batch_idxs)]

    def get_reward_sums(self):
        """Reward sums of the newest `num_rewards_to_sum` windows (replay_buffer.py:221-225)."""
        n = min(self.num_rewards_to_sum, self.length)
        idx = torch.arange(self.length - n, self.length, device=self.device)
        return [float(x) for x in self._ring["reward_sum"][self._slots(idx)].cpu()]

    def empty_buffer(self):
        self.start = self.length = 0
        self._written = 0
        self._epoch += 1  # handles of earlier ingests no longer name windows of this ring
        if self.prioritized:
            self._q.zero_()

    # -- prioritized replay (csrc/replay_prio.hip) --------------------------------------------------
    def _need_prio(self):
        if not self.prioritized:
            raise RuntimeError("this DeviceReplayBuffer was built with prioritized=False")

    def _init_priorities(self, head, n):
        """The ingest rule for the n windows written from slot `head` on (the newest max_length of them):
        q = (|values[slot][0] - targets[slot][0]| + prio_eps) ** alpha."""
        g = self._ring
        L.call("mzba_replay_priority_init", L.ptr(self._q), L.ptr(g["values"]), L.ptr(g["targets"]), self.max_length,
               head, n, self.K, self.alpha, self.prio_eps, L.stream())

    def _sample_workspace(self, n):
        """The sampler's scratch for n samples, kept per n (allocate it before a graph capture that samples)."""
        ws = self._sample_ws.get(n)
        if ws is None:
            nbytes = L.lib().mzba_replay_sample_ws_bytes(self.max_length, n)
            ws = self._sample_ws[n] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws

    def sample(self, n, step, seed=0, u=None, step_dev=None):
        """n windows drawn in proportion to their priorities (stratified: sample j from the j-th n-th of the
        mass), on the device with no host round trip -> (slots i32[n] ring rows, weights f32[n] =
        (len * P) ** -beta over the batch's largest, probs f32[n]). The draws are Philox (j, stream 4, step, 0)
        under `seed`; `step_dev` (device i32/u32 [1]) overrides `step`, so a captured graph draws afresh on every
        replay; `u` (device f32[n] in [0, 1)) replaces the draws. len(self) is read when the call is recorded: it
        cancels in the normalised weights up to rounding."""
        self._need_prio()
        if self.length == 0:
            raise ValueError("sample from an empty replay buffer")
        n = int(n)
        dev = self.device
        slots = torch.empty(n, dtype=torch.int32, device=dev)
        probs = torch.empty(n, dtype=torch.float32, device=dev)
        weights = torch.empty(n, dtype=torch.float32, device=dev)
        if u is not None:
            u = u.to(device=dev, dtype=torch.float32).contiguous()
            if u.numel() != n:
                raise ValueError("u must hold one draw per sample")
        if step_dev is not None and (step_dev.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not step_dev.is_cuda):
            raise ValueError("step_dev must be a device int32 / uint32 tensor")
        ws = self._sample_workspace(n)
        L.call("mzba_replay_sample", L.ptr(self._q), self.max_length, n, self.beta, self.length, int(seed),
               int(step) & 0xFFFFFFFF, L.ptr(step_dev), L.ptr(u), L.ptr(slots), L.ptr(probs), L.ptr(weights), L.ptr(ws),
               ws.numel(), L.stream())
        return slots, weights, probs

    def update_priorities(self, slots, td, guard_block=None):
        """q[slots[j]] = (td[j] + prio_eps) ** alpha (td: the learner's last_td for the windows `slots` of a
        `sample`). No ingest may run between the sample and this call; duplicates must carry equal td.
        guard_block (a guarded Learner's device stats block): q stays as it is when that step was skipped."""
        self._need_prio()
        if slots.dtype != torch.int32 or td.dtype != torch.float32 or slots.numel() != td.numel():
            raise ValueError("update_priorities takes i32 slots and f32 td of one length")
        slots, td = slots.contiguous(), td.contiguous()  # held until the launch is made
        if guard_block is not None:
            L.call("mzba_replay_priority_update_g", L.ptr(self._q), L.ptr(slots), L.ptr(td), slots.numel(),
                   self.max_length, self.alpha, self.prio_eps, L.ptr(guard_block), L.stream())
            return
        L.call("mzba_replay_priority_update", L.ptr(self._q), L.ptr(slots), L.ptr(td), slots.numel(), self.max_length,
               self.alpha, self.prio_eps, L.stream())

    def priorities(self):
        """q = p ** alpha of the stored windows, oldest first (f32 device tensor)."""
        self._need_prio()
        idx = torch.arange(self.length, device=self.device)
        return self._q[(idx + self.start) % self.max_length]

    # -- the reference's list layout (checkpoint replay_buffer, train_torch.py:624-635) ----
    def to_reference_lists(self):
        idx = torch.arange(self.length, device=self.device)
        cpu = lambda t: list(t.cpu().unbind(0)) if self.length else []  # noqa: E731
        sl = self._slots(idx) if self.length else idx
        d = {
            "past_actions_buffer": cpu(self._ring["past_actions"][sl]),
            "future_actions_buffer": cpu(self._ring["future_actions"][sl]),
            "state_buffer": cpu(self.get_batched_states(idx)) if self.length else [],
            "reward_buffer": cpu(self._ring["rewards"][sl]),
            "visit_counts_buffer": cpu(self._ring["counts"][sl]),
            "value_buffer": cpu(self._ring["values"][sl]),
            "reward_sums": [float(x) for x in self._ring["reward_sum"][sl].cpu()],
            "length": self.length,
            "max_length": self.max_length,
            "bootstrapped_values": cpu(self._ring["targets"][sl]),
        }
        if self.prioritized:  # beside the reference's keys, which stay as they are
            d["priorities"] = self.priorities().cpu()
        return d

    def load_reference_lists(self, d):
        """Replace the contents with a reference replay_buffer dict (oldest first)."""
        n = int(d["length"])
        if n > self.max_length:
            raise ValueError(f"checkpoint holds {n} windows, buffer max_length is {self.max_length}")
        self.empty_buffer()
        if n == 0:
            return
        lut = gray_lut()
        vals, first = np.unique(lut, return_index=True)
        st = np.stack([np.asarray(s, np.float32) for s in d["state_buffer"][:n]]).reshape(n, self.hist_seq_len, -1)
        pos = np.searchsorted(vals, st).clip(0, len(vals) - 1)
        if not np.array_equal(vals[pos], st):
            raise ValueError("state_buffer holds values that are not convert_to_grayscale outputs")
        g, dev = self._ring, self.device
        put = lambda key, rows, dt: g[key][:n].copy_(torch.as_tensor(np.stack([np.asarray(x) for x in rows]),  # noqa: E731
                                                                  dtype=dt).to(dev))
        g["states"][:n].copy_(torch.from_numpy(first[pos].astype(np.uint8)).to(dev))
        put("past_actions", d["past_actions_buffer"][:n], torch.int64)
        put("future_actions", d["future_actions_buffer"][:n], torch.int64)
        put("rewards", d["reward_buffer"][:n], torch.float32)
        put("counts", d["visit_counts_buffer"][:n], torch.float32)
        put("values", d["value_buffer"][:n], torch.float32)
        put("targets", d["bootstrapped_values"][:n], torch.float32)
        g["reward_sum"][:n].copy_(torch.tensor(np.asarray(d["reward_sums"][:n], np.float32)).to(dev))
        self.start, self.length = 0, n
        self._written = n
        if self.prioritized:
            if d.get("priorities") is not None:
                self._q[:n].copy_(torch.as_tensor(d["priorities"], dtype=torch.float32)[:n].to(dev))
            else:
                self._init_priorities(0, n)
