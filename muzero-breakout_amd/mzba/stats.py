"""Episode statistics on the device (csrc/episode_stats.hip).

`EpisodeStats` owns one `mzba_episode_stats` block on the device and adds streamed sinks to it with
`mzba_stream_episode_stats`: no host read, capturable in a graph. `read()` is the one host copy.

    stats = EpisodeStats(B)
    stage.run(); stats.add_stage(stage)         # a StreamingStage after its run()
    stats.add_slab(archive, slab)               # or a slab of a SinkArchive
    d = stats.read()                            # counts, sums, histogram and the derived means

An episode is a closed segment with at least one record; with `first_n` > 0 only the first `first_n` episodes of every
env are counted (evaluation: a fixed-length stage with dropped tails over-represents short episodes, the first n of
every env do not). `ep_n` > 0 also keeps the return and length of each env's first `ep_n` counted episodes.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from .config import default_config

# include/mzba.h mzba_episode_stats, field for field
BLOCK_DT = np.dtype([("episodes", "<i8"), ("capped", "<i8"), ("rows", "<i8"), ("ret_sum", "<f8"), ("ret_sq", "<f8"),
                     ("ret_min", "<f4"), ("ret_max", "<f4"), ("len_min", "<i4"), ("len_max", "<i4"),
                     ("hist", "<i8", (32,)), ("verr_rows", "<i8"), ("verr_sum", "<f8"), ("verr_abs", "<f8"),
                     ("verr_sq", "<f8"), ("value_sum", "<f8"), ("entropy_sum", "<f8")])
BLOCK_BYTES = BLOCK_DT.itemsize


def block_dict(raw):
    """The raw block (360 bytes: a uint8 array or tensor) -> {field: python value; hist: list of 32 ints}."""
    a = np.frombuffer(np.asarray(raw, dtype=np.uint8).tobytes(), dtype=BLOCK_DT)[0]
    return {k: (a[k].tolist() if k == "hist" else a[k].item()) for k in BLOCK_DT.names}


def derived(d):
    """The means a reader wants, from a block's fields (None where the denominator is 0)."""
    n, rows, vr = d["episodes"], d["rows"], d["verr_rows"]
    mean = d["ret_sum"] / n if n else None
    return {
        "return_mean": mean,
        "return_std": math.sqrt(max(d["ret_sq"] / n - mean * mean, 0.0)) if n else None,
        "length_mean": rows / n if n else None,
        "capped_share": d["capped"] / n if n else None,
        "value_error_mean": d["verr_sum"] / vr if vr else None,
        "value_error_abs": d["verr_abs"] / vr if vr else None,
        "value_error_rms": math.sqrt(d["verr_sq"] / vr) if vr else None,
        "root_value_mean": d["value_sum"] / rows if rows else None,
        "target_entropy_mean": d["entropy_sum"] / rows if rows else None,
    }


class EpisodeStats:
    """One accumulating statistics block for sinks of B envs. `gamma` (default: the config's discount_factor)
    discounts the return the root values are compared with; the histogram's bin of a return R is
    clamp(floor((R - hist_lo) / hist_step), 0, 31)."""

    def __init__(self, B, first_n=0, ep_n=0, hist_lo=-8.0, hist_step=1.0, gamma=None, device="cuda"):
        L.require_gpu()
        if B < 1 or first_n < 0 or ep_n < 0 or not hist_step > 0:
            raise ValueError("EpisodeStats: B >= 1, first_n >= 0, ep_n >= 0 and hist_step > 0")
        if ctypes.sizeof(L.EpisodeStats) != BLOCK_BYTES:
            raise RuntimeError("mzba.stats.BLOCK_DT does not match the binding's mzba_episode_stats")
        self.B, self.first_n, self.ep_n = int(B), int(first_n), int(ep_n)
        self.hist_lo, self.hist_step = float(hist_lo), float(hist_step)
        self.gamma = float(default_config()["discount_factor"] if gamma is None else gamma)
        self.device = dev = torch.device(device)
        # the block and the per-env lists in one buffer: read() is one copy
        n = self.B * self.ep_n
        self._buf = torch.zeros(BLOCK_BYTES + 8 * n, dtype=torch.uint8, device=dev)
        self.block = self._buf[:BLOCK_BYTES]
        self.ep_ret = self._buf[BLOCK_BYTES:BLOCK_BYTES + 4 * n].view(torch.float32).view(self.B, self.ep_n) if n else None
        self.ep_len = self._buf[BLOCK_BYTES + 4 * n:].view(torch.int32).view(self.B, self.ep_n) if n else None
        self._ws = torch.empty(int(L.lib().mzba_stream_episode_stats_ws_bytes(self.B)), dtype=torch.uint8, device=dev)

    def add(self, rec, T, done, hlen, episode_cap):
        """A streamed sink's first T rows (`ingest_stream`'s rec, done, hlen) into the block. No host read."""
        if rec.get("start") is None:
            raise ValueError("EpisodeStats.add needs a streamed sink (its start words)")
        if rec["action"].shape[1] != self.B:
            raise ValueError(f"EpisodeStats.add: the sink has {rec['action'].shape[1]} envs, not {self.B}")
        done = done.to(device=self.device, dtype=torch.uint8).contiguous()
        hlen = hlen.to(device=self.device, dtype=torch.int32).contiguous()
        frame = rec.get("frame")
        sink = L.sink(rec, int(T), frame.shape[-1] if frame is not None else 0)
        L.call("mzba_stream_episode_stats", ctypes.byref(sink), L.ptr(done), L.ptr(hlen), int(episode_cap),
               self.first_n, self.gamma, self.hist_lo, self.hist_step, L.ptr(self.block), L.ptr(self.ep_ret),
               L.ptr(self.ep_len), self.ep_n, L.ptr(self._ws), self._ws.numel(), L.stream())

    def add_stage(self, stage):
        """`add` from a `StreamingStage` after its run()."""
        env = stage.loop.env
        self.add(stage.loop.rec, stage.steps, env.done, env.hist_len, stage.episode_cap)

    def add_slab(self, archive, slab):
        """`add` of one slab of a `SinkArchive`: every last segment counts as closed, and the tails the archive
        dropped have no record left, so they are no episodes."""
        slab = int(slab)
        if not 0 <= slab < archive.slabs:
            raise ValueError(f"EpisodeStats.add_slab: no slab {slab}")
        self.add(archive.slab_rec(slab), archive.steps, archive._closed, archive._hlen0, archive.episode_cap)

    def reset(self):
        self._buf.zero_()

    def state(self):
        """The raw block (a device uint8 copy)."""
        return self.block.clone()

    def load_state(self, raw):
        if raw.numel() != BLOCK_BYTES or raw.dtype != torch.uint8:
            raise ValueError("EpisodeStats.load_state takes the 360 raw bytes of state()")
        self.block.copy_(raw.to(self.device))

    def read(self):
        """One device-to-host copy (it synchronises) -> the block's fields, the derived means and, with ep_n > 0,
        `ep_ret` f32 [B][ep_n] / `ep_len` i32 [B][ep_n] of the last sink added."""
        host = self._buf.cpu().numpy()
        d = block_dict(host[:BLOCK_BYTES])
        d.update(derived(d))
        n = self.B * self.ep_n
        if n:
            d["ep_ret"] = host[BLOCK_BYTES:BLOCK_BYTES + 4 * n].view(np.float32).reshape(self.B, self.ep_n).copy()
            d["ep_len"] = host[BLOCK_BYTES + 4 * n:].view(np.int32).reshape(self.B, self.ep_n).copy()
        return d
