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
masks and frames are never written. Streamed sinks (several episodes per env) are out of scope.
"""
import ctypes

import torch

from . import _lib as L
from .search import MCTSSearchVec, SearchWorkspace


class Reanalyser:
    """The search of `ActingLoop` over B envs without an env, a sampler or a sink of its own. `seed` and
    `env_offset` key the root noise and the tie-breaks exactly as the acting loop's do: with the recording
    loop's values, the same agent and the same search ids a refresh reproduces the sink bit for bit."""

    def __init__(self, cfg, agent, B, seed=0, env_offset=0, height=16, width=20, pad_action=0):
        L.require_gpu()
        self.cfg, self.agent, self.B = cfg, agent, B
        self.seed, self.env_offset, self.pad_action = seed, env_offset, pad_action
        self.Lh = cfg["model"]["state_history_length"]
        self.H, self.W = height, width
        dev = agent.device
        self.search = MCTSSearchVec(cfg, agent, None, seed=seed, env_offset=env_offset)
        self.ws = SearchWorkspace(self.search, B)
        p = agent.packed
        self.cs = (2 * self.Lh + 63) // 64 * 64
        self.rep_in = torch.empty(B * height * width * self.cs, dtype=p.tdt, device=dev)
        self.rep_runner = agent.runner(B, height, width)
        # device step context [search id, 0, sink row t]: the one captured row graph reads both from here
        self.ctx = torch.zeros(3, dtype=torch.int32, device=dev)
        self.graph = None
        self._graph_key = None

    @staticmethod
    def snapshot(rec, frame0, T):
        """Clones of the sink's first T rows and of g(s0): an archive to reanalyse while the stage goes on
        recording into its own sink."""
        return ({k: (None if v is None else v[:T].clone()) for k, v in rec.items()}, frame0.clone())

    def _check(self, rec, frame0, T):
        if rec.get("start") is not None:
            raise ValueError("refresh: a streamed sink holds several episodes per env (out of scope, DESIGN.md §16)")
        if rec.get("frame") is None:
            raise ValueError("refresh needs the sink's recorded frames (record_frames=True)")
        if rec["action"].shape[1] != self.B:
            raise ValueError(f"refresh: the sink holds {rec['action'].shape[1]} envs, the workspace {self.B}")
        if not 0 < T <= rec["action"].shape[0]:
            raise ValueError(f"refresh: T = {T} outside the sink's {rec['action'].shape[0]} rows")
        if frame0.numel() != self.B * self.H * self.W or frame0.dtype != torch.uint8 or not frame0.is_contiguous():
            raise ValueError("refresh: frame0 must be the contiguous u8 [B][H*W] codes of g(s0)")

    def _row_body(self, sk, frame0):
        """One row, every launch stream-ordered and parameterised by self.ctx."""
        ws = self.ws
        L.call("mzba_sink_rep_input", sk, L.ptr(frame0), self.Lh, self.pad_action, 0, L.ptr(self.ctx),
               L.ptr(self.rep_in), 1 if self.agent.dtype == "bf16" else 0, self.cs, L.stream())
        self.rep_runner.representation(self.rep_in, ws.cur, pool=ws.pool, pool_env_stride=(ws.S + 1) * ws.n)
        values, counts = ws.search(0, ctx=self.ctx)
        L.call("mzba_record_results_masked", L.ptr(counts), L.ptr(values), sk, 0, L.ptr(self.ctx), L.stream())

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
        rows = list(range(T)) if rows is None else [int(t) for t in rows]
        if any(not 0 <= t < T for t in rows):
            raise ValueError(f"refresh: rows must lie in [0, {T})")
        return _Run(self, rec, frame0, T, search_id0, rows, noise_weight, use_graph)


class _Run:
    """One refresh in progress (Reanalyser.begin)."""

    def __init__(self, rean, rec, frame0, T, search_id0, rows, noise_weight, use_graph):
        self.rean, self.frame0, self.n, self.use_graph = rean, frame0, len(rows), use_graph
        if not rows:
            return
        rean.ws.sync_noise_weight(noise_weight)
        self.sink = L.sink(rec, T, rean.H * rean.W)  # held: the launches read it through this reference
        self.sk = ctypes.byref(self.sink)
        self.table = torch.tensor([[search_id0 + t, 0, t] for t in rows], dtype=torch.int32).to(rean.agent.device)
        if use_graph:
            # the captured launches hold the sink's addresses and T
            key = (T, frame0.data_ptr()) + tuple(None if rec.get(k) is None else rec[k].data_ptr()
                                                 for k in ("action", "mask", "counts", "values", "frame"))
            if rean._graph_key != key:
                rean.ctx.copy_(self.table[0])
                rean._row_body(self.sk, frame0)  # eager once: lazy allocations happen outside the capture
                rean.graph, rean._graph_key = L.capture(lambda: rean._row_body(self.sk, frame0)), key

    def row(self, i):
        rean = self.rean
        rean.ctx.copy_(self.table[i])  # stream-ordered, between two replays
        if self.use_graph:
            rean.graph.replay()
        else:
            rean._row_body(self.sk, self.frame0)
