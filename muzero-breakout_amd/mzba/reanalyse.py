"""Reanalyse (MuZero, Appendix H): re-run the search on the rows of a recorded trajectory sink
with the current net and write the fresh visit counts and root values back into the sink.

The acting loop's sink (`ActingLoop.rec`) holds a whole episode: per step the action, reward, mask, frame, visit
counts and root value of every env. The representation input of step t is a function of the sink's rows < t and
g(s0) alone (csrc/reanalyse.hip), so any row can be searched again, in any order, with any net:

    rec, frame0 = Reanalyser.snapshot(stage.loop.rec, stage.loop.frame0, T)   # the stage reuses its own sink
    handle = buffer.last_ingest                                               # of the ingest of that episode
    ... train, refresh_from_learner(agent, learner) ...
    Reanalyser(cfg, agent, B, seed).refresh(rec, frame0, T, search_id0)
    buffer.reingest_records(handle, rec, frame0, T)

A row runs the acting step's launches without the action sampling and the env step. The recorded actions, rewards,
masks and frames are never written.

A streamed sink (`mzba.stream.StreamingStage`: several episodes per env, `rec["start"]`) has entry points of its own,
because an env's history stops at its segment's start word, which also renders the segment's g(s0): there is no frame0.

    rec, done, hlen = Reanalyser.snapshot_stream(stage.loop.rec, T, env.done, env.hist_len)
    handle, sid0 = buffer.last_stream_ingest, stage.last_search_id0
    ... train, refresh_from_learner(agent, learner) ...
    Reanalyser(cfg, agent, B, seed).refresh_stream(rec, T, sid0)
    buffer.reingest_stream(handle, rec, T, done, hlen)
"""
import ctypes

import torch

from . import _lib as L
from .search import MCTSSearchVec, SearchWorkspace

_SINK_KEYS = ("action", "mask", "counts", "values", "frame")


class Reanalyser:
    """The search of `ActingLoop` over B envs without an env, a sampler or a sink of its own. `seed` and
    `env_offset` key the root noise and the tie-breaks exactly as the acting loop's do: with the recording
    loop's values, the same agent and the same search ids a refresh reproduces the sink bit for bit.
    `paddle_width` and `brick_rows` are the env's (a streamed sink's g(s0) is rendered from its start words)."""

    def __init__(self, cfg, agent, B, seed=0, env_offset=0, height=16, width=20, pad_action=0, paddle_width=6,
                 brick_rows=3):
        L.require_gpu()
        self.cfg, self.agent, self.B = cfg, agent, B
        self.seed, self.env_offset, self.pad_action = seed, env_offset, pad_action
        self.Lh = cfg["model"]["state_history_length"]
        self.H, self.W = height, width
        self.paddle_width, self.brick_rows = paddle_width, brick_rows
        dev = agent.device
        self.search = MCTSSearchVec(cfg, agent, None, seed=seed, env_offset=env_offset)
        self.ws = SearchWorkspace(self.search, B)
        p = agent.packed
        self.cs = (2 * self.Lh + 63) // 64 * 64
        self.rep_in = torch.empty(B * height * width * self.cs, dtype=p.tdt, device=dev)
        self.rep_runner = agent.runner(B, height, width)
        # device step context [search id, 0, sink row t]: the one captured row graph reads both from here
        self.ctx = torch.zeros(3, dtype=torch.int32, device=dev)
        # one captured row per kind of sink, each valid for the addresses in its key
        self.graph = None
        self._graph_key = None
        self.stream_graph = None
        self._stream_graph_key = None
        # streamed sinks: origin[t][b] = the row env b's episode at row t started at, filled per refresh (the captured
        # row holds its address, so it is reallocated only for a longer sink)
        self._origin = None

    @staticmethod
    def snapshot(rec, frame0, T):
        """Clones of the sink's first T rows and of g(s0): an archive to reanalyse while the stage goes on
        recording into its own sink."""
        return ({k: (None if v is None else v[:T].clone()) for k, v in rec.items()}, frame0.clone())

    @staticmethod
    def snapshot_stream(rec, T, done, hlen):
        """Clones of a streamed sink's first T rows (start words included) and of the envs' `done` / `hist_len` at
        the end of the stage, which `reingest_stream` plans with: the next stage overwrites all three."""
        return {k: (None if v is None else v[:T].clone()) for k, v in rec.items()}, done.clone(), hlen.clone()

    def _check_rows(self, what, rec, T):
        if rec.get("frame") is None:
            raise ValueError(f"{what} needs the sink's recorded frames (record_frames=True)")
        if rec["action"].shape[1] != self.B:
            raise ValueError(f"{what}: the sink holds {rec['action'].shape[1]} envs, the workspace {self.B}")
        if not 0 < T <= rec["action"].shape[0]:
            raise ValueError(f"{what}: T = {T} outside the sink's {rec['action'].shape[0]} rows")

    def _check(self, rec, frame0, T):
        if rec.get("start") is not None:
            raise ValueError("refresh: a streamed sink holds several episodes per env; use refresh_stream "
                             "(DESIGN.md §17)")
        self._check_rows("refresh", rec, T)
        if frame0.numel() != self.B * self.H * self.W or frame0.dtype != torch.uint8 or not frame0.is_contiguous():
            raise ValueError("refresh: frame0 must be the contiguous u8 [B][H*W] codes of g(s0)")

    def _check_stream(self, rec, T):
        start = rec.get("start")
        if start is None:
            raise ValueError("refresh_stream: the sink has no start words (a lockstep sink: use refresh)")
        self._check_rows("refresh_stream", rec, T)
        if start.shape != rec["action"].shape or start.element_size() != 4 or not start.is_contiguous():
            raise ValueError("refresh_stream: start must be the contiguous 32-bit (T, B) start words of the sink")

    def _search_and_record(self, sk):
        ws = self.ws
        self.rep_runner.representation(self.rep_in, ws.cur, pool=ws.pool, pool_env_stride=(ws.S + 1) * ws.n)
        values, counts = ws.search(0, ctx=self.ctx)
        L.call("mzba_record_results_masked", L.ptr(counts), L.ptr(values), sk, 0, L.ptr(self.ctx), L.stream())

    def _row_body(self, sk, frame0):
        """One row, every launch stream-ordered and parameterised by self.ctx."""
        L.call("mzba_sink_rep_input", sk, L.ptr(frame0), self.Lh, self.pad_action, 0, L.ptr(self.ctx),
               L.ptr(self.rep_in), 1 if self.agent.dtype == "bf16" else 0, self.cs, L.stream())
        self._search_and_record(sk)

    def _row_body_stream(self, sk):
        """_row_body for a streamed sink: the gather takes the env's segment from the origin table."""
        L.call("mzba_sink_rep_input_stream", sk, L.ptr(self._origin), self.H, self.W, self.paddle_width,
               self.brick_rows, self.Lh, self.pad_action, 0, L.ptr(self.ctx), L.ptr(self.rep_in),
               1 if self.agent.dtype == "bf16" else 0, self.cs, L.stream())
        self._search_and_record(sk)

    def refresh(self, rec, frame0, T, search_id0, rows=None, noise_weight=None, use_graph=True):
        """Search the rows `rows` (default all T; any subset, in any order: a row depends only on the actions and
        frames of earlier rows, which are never written) of the sink `rec` (dict of (T_max, B, ...) device tensors,
        first T rows) again, row t under the search id search_id0 + t, and write counts and values of the envs
        recorded at that row. No host synchronisation; `use_graph` captures the row once and replays it."""
        run = self.begin(rec, frame0, T, search_id0, rows, noise_weight, use_graph)
        for i in range(run.n):
            run.row(i)
        return run.n

    def begin(self, rec, frame0, T, search_id0, rows=None, noise_weight=None, use_graph=True):
        """refresh's checks and set-up (the device table of the rows' step contexts, the captured row) -> an
        object whose row(i) launches the i-th of the rows; refresh is begin + every row in turn."""
        self._check(rec, frame0, T)
        rows = _rows("refresh", rows, T)
        return _Run(self, rec, T, search_id0, rows, noise_weight, use_graph, frame0)

    def refresh_stream(self, rec, T, search_id0, rows=None, noise_weight=None, use_graph=True):
        """`refresh` for a streamed sink (`rec["start"]`; no frame0). Row t of a stage was searched under the id
        search_id0 + t with search_id0 = `StreamingStage.last_search_id0`: search and noise keys run on across
        restarts. Every row of a streamed sink is recorded, so every env's counts and values are written."""
        run = self.begin_stream(rec, T, search_id0, rows, noise_weight, use_graph)
        for i in range(run.n):
            run.row(i)
        return run.n

    def begin_stream(self, rec, T, search_id0, rows=None, noise_weight=None, use_graph=True):
        """`begin` for a streamed sink."""
        self._check_stream(rec, T)
        rows = _rows("refresh_stream", rows, T)
        return _Run(self, rec, T, search_id0, rows, noise_weight, use_graph, None)


def _rows(what, rows, T):
    rows = list(range(T)) if rows is None else [int(t) for t in rows]
    if any(not 0 <= t < T for t in rows):
        raise ValueError(f"{what}: rows must lie in [0, {T})")
    return rows


class _Run:
    """One refresh in progress (Reanalyser.begin with the sink's frame0, begin_stream with frame0 = None)."""

    def __init__(self, rean, rec, T, search_id0, rows, noise_weight, use_graph, frame0):
        self.rean, self.n, self.use_graph = rean, len(rows), use_graph
        if not rows:
            return
        rean.ws.sync_noise_weight(noise_weight)
        self.sink = L.sink(rec, T, rean.H * rean.W)  # held: the launches read it through this reference
        sk = ctypes.byref(self.sink)
        self.streamed = frame0 is None
        self.slot = "stream_graph" if self.streamed else "graph"  # the Reanalyser's captured row of this kind
        self.body = (lambda: rean._row_body_stream(sk)) if self.streamed else (lambda: rean._row_body(sk, frame0))
        self.table = torch.tensor([[search_id0 + t, 0, t] for t in rows], dtype=torch.int32).to(rean.agent.device)
        if self.streamed:  # one column walk per refresh: the rows then read one word each
            if rean._origin is None or rean._origin.shape[0] < T:
                rean._origin = torch.empty(T, rean.B, dtype=torch.int32, device=rean.agent.device)
            L.call("mzba_sink_origin", sk, L.ptr(rean._origin), L.stream())
        if use_graph:
            # the captured launches hold the sink's addresses and T; each kind of sink has a graph of its own
            first = (rec["start"].data_ptr(), rean._origin.data_ptr()) if self.streamed else (frame0.data_ptr(),)
            key = (T,) + first + tuple(None if rec.get(k) is None else rec[k].data_ptr() for k in _SINK_KEYS)
            if getattr(rean, f"_{self.slot}_key") != key:
                rean.ctx.copy_(self.table[0])
                self.body()  # eager once: lazy allocations happen outside the capture
                setattr(rean, self.slot, L.capture(self.body))
                setattr(rean, f"_{self.slot}_key", key)

    def row(self, i):
        rean = self.rean
        rean.ctx.copy_(self.table[i])  # stream-ordered, between two replays
        if self.use_graph:
            getattr(rean, self.slot).replay()
        else:
            self.body()
