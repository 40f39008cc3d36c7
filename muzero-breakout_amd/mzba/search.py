"""Latent MCTS on the MI355X path (mirror of src/mcts.py:MCTSSearchVec).

The whole search runs on the device with no host synchronisation, every launch a torch custom op
(`torch.ops.mz`): per simulation the fused dynamics step (`dynamics_`, parent latents gathered from
the node pool by the selected slots) and the fused prediction step that also backs up the
simulation and selects the next leaf (`prediction_tree_`); unfused, one select kernel, the
prediction net and one backup kernel.
The launch sequence is identical for every call of a given (B, S), so the acting loop
can capture it in a HIP graph.

cfg["search"]["kind"] == "gumbel" selects the Gumbel search (csrc/gumbel.hip): per
simulation the dynamics step, the prediction step without a tree and one tree launch (backup +
next selection). An absent key or "puct" is the path above.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _lib as L
from .agent import MuZeroAgent  # noqa: F401  (re-export for the drop-in module)


def ucb_tables(S, c1, c2, device):
    """f32(sqrt(n)) and f32(c1 + log((n + c2 + 1) / c2)) for n = 0..S, evaluated in
    double exactly as mcts.py:285-289 does (math.sqrt / math.log on Python floats)."""
    sq = np.array([math.sqrt(n) for n in range(S + 1)], dtype=np.float64).astype(np.float32)
    ct = np.array([c1 + math.log((n + c2 + 1) / c2) for n in range(S + 1)], dtype=np.float64).astype(np.float32)
    return torch.from_numpy(sq).to(device), torch.from_numpy(ct).to(device)


def gumbel_schedule(S, m):
    """The root visit schedule seq[0..S) of sequential halving over m considered actions:
    simulation s visits a considered action whose visit count is seq[s]."""
    l2 = max(1, math.ceil(math.log2(m)))
    visits = [0] * m
    nc = m
    seq = []
    while len(seq) < S:
        extra = max(1, int(S / (l2 * nc)))
        for _ in range(extra):
            seq += visits[:nc]
            for i in range(nc):
                visits[i] += 1
        nc = max(2, nc // 2)
    return seq[:S]


def gumbel_params(cfg):
    """(max_considered, c_visit, c_scale, scale) of cfg["search"]["gumbel"] with the defaults 3, 50, 1, 1."""
    g = cfg["search"].get("gumbel", {})
    m = int(g.get("max_considered", 3))
    if m not in (2, 3):
        raise ValueError(f"gumbel search: max_considered must be 2 or 3, not {m}")
    return m, float(g.get("c_visit", 50.0)), float(g.get("c_scale", 1.0)), float(g.get("scale", 1.0))


def search_kind(cfg):
    kind = cfg["search"].get("kind", "puct")
    if kind not in ("puct", "gumbel"):
        raise ValueError(f"cfg['search']['kind'] must be 'puct' or 'gumbel', not {kind!r}")
    return kind


class GumbelState:
    """Device buffers of the Gumbel search over a TreeState's trees, and its three launches."""

    def __init__(self, tree, m, c_visit, c_scale, scale, device):
        self.tree = tree
        B, S = tree.B, tree.S
        self.m, self.c_visit, self.c_scale, self.scale = m, c_visit, c_scale, scale
        self.g = torch.empty(B, 3, dtype=torch.float32, device=device)
        self.considered = torch.empty(B, dtype=torch.uint8, device=device)
        self.seq = torch.tensor(gumbel_schedule(S, m), dtype=torch.int32, device=device)
        self.variates = torch.empty(B, 3, dtype=torch.float32, device=device)  # the root's standard Gumbel draws
        self.actions = torch.empty(B, dtype=torch.int64, device=device)
        self.root_n = torch.empty(B, 3, dtype=torch.int32, device=device)

    def _structs(self, ta, sim=0, gamma=0.0, r=None):
        ts = self.tree.step(*ta, sim, gamma, r)
        gm = L.Gumbel(L.addr(self.g), L.addr(self.considered), L.addr(self.seq), self.m, self.c_visit, self.c_scale,
                      self.scale)
        return ctypes.byref(ts), ctypes.byref(gm)

    def root(self, ta, v_root, pi_root, g_in=None):
        L.call("mzba_gumbel_root", *self._structs(ta), L.ptr(v_root), L.ptr(pi_root), L.ptr(g_in),
               L.ptr(self.variates), L.stream())

    def step(self, ta, sim, r, v, pi, gamma):
        L.call("mzba_gumbel_step", *self._structs(ta, sim, gamma, r), L.ptr(v), L.ptr(pi), L.stream())

    def results(self, ta):
        t = self.tree
        L.call("mzba_gumbel_results", *self._structs(ta), L.ptr(t.counts), L.ptr(t.values), L.ptr(self.actions),
               L.ptr(self.root_n), L.stream())


class TreeState:
    """Device buffers of B search trees with S simulations."""

    def __init__(self, B, S, c1, c2, device):
        self.B, self.S = B, S
        nb = L.lib().mzba_mcts_node_bytes()
        self.nodes = torch.empty(B * (S + 1) * nb, dtype=torch.uint8, device=device)
        self.root_sum = torch.empty(B, dtype=torch.float32, device=device)
        self.calls = torch.empty(B, dtype=torch.int32, device=device)
        self.leaf_parent = torch.empty(B, dtype=torch.int32, device=device)
        self.leaf_action = torch.empty(B, dtype=torch.int32, device=device)
        self.depth = torch.empty(B, dtype=torch.int32, device=device)
        self.path = torch.empty(B * (S + 1), dtype=torch.int32, device=device)
        self.sqrt_tab, self.c_tab = ucb_tables(S, c1, c2, device)
        self.counts = torch.empty(B, 3, dtype=torch.int64, device=device)
        self.values = torch.empty(B, dtype=torch.float32, device=device)
        self.noise = torch.empty(B, 3, dtype=torch.float32, device=device)

    def args(self, env_offset, search_id, seed, ctx=None):
        """Tree arguments of the torch.ops.mz tree ops (csrc/torch_ops.cpp). ctx: optional device
        int32[3] step context (its [0] overrides search_id; graph replay)."""
        return (self.nodes, self.root_sum, self.calls, self.leaf_parent, self.leaf_action, self.depth, self.path,
                self.sqrt_tab, self.c_tab, self.S, env_offset, search_id, seed, ctx)

    def step(self, env_offset, search_id, seed, ctx=None, sim=0, gamma=0.0, r=None):
        """The trees as the C ABI's mzba_tree_step, for simulation `sim` where the entry point reads one."""
        a = L.addr
        return L.TreeStep(a(self.nodes), a(self.root_sum), a(self.calls), a(self.leaf_parent), a(self.leaf_action),
                          a(self.depth), a(self.path), a(self.sqrt_tab), a(self.c_tab), self.B, self.S, env_offset,
                          search_id, seed, a(ctx), sim, gamma, a(r))

    # individual kernels, dispatched as torch custom ops -----------------------------------------
    def root(self, tree_args, v_root, pi_root, noise_in, w_pol, w_noise, alpha, w_dev=None):
        L.ops().mcts_root_(*tree_args, v_root, pi_root, noise_in, self.noise, w_pol, w_noise, w_dev, alpha)

    def select(self, tree_args, sim):
        L.ops().mcts_select_(*tree_args, sim)

    def backup(self, tree_args, sim, r, v, pi, gamma):
        L.ops().mcts_backup_(*tree_args, sim, r, v, pi, gamma)

    def results(self, tree_args):
        L.ops().mcts_results_(*tree_args, self.values, self.counts)


class MCTSSearchVec:
    """Drop-in for src/mcts.py:MCTSSearchVec (constructor and `search` signature).

    search(hidden_state (B,C,h,w), action_mask (B,3), training_iteration)
      -> (values f32[B] CPU, visit_counts i64[B,3] CPU), like mcts.py:71.
    In Gumbel mode (cfg["search"]["kind"] == "gumbel") the second result is the improved policy in 24-bit
    fixed point (rows sum to 2^24 within rounding), the first its value, and the chosen actions are kept
    in `self.selected_actions` (i64[B] CPU); `noise` then injects the root's Gumbel variates.
    `action_mask` and `training_iteration` are accepted and ignored, as in the
    reference (mcts.py:124,157 use ones_like(action_mask)).
    Randomness: Dirichlet root noise and ucb tie-breaks come from the keyed Philox
    stream (seed, global env, search id) — see DESIGN.md §RNG.
    """

    def __init__(self, cfg, mu_zero, scalar_transforms=None, seed=0, env_offset=0):
        self.num_simulations = cfg["num_simulations"]  # mcts.py:13-22
        self.actions = cfg["actions"]
        self.c1 = cfg["search"]["c1"]
        self.c2 = cfg["search"]["c2"]
        self.discount = cfg["search"]["discount_factor"]
        self.mu_zero = mu_zero
        self.scalar_transforms = scalar_transforms
        self.latent_resolution = cfg["latent_resolution"]
        self.dirchlet_alpha = 0.25
        self.noise_weight = 0.175
        self.seed = seed
        self.env_offset = env_offset
        self.search_id = 0
        self.kind = search_kind(cfg)
        self.gumbel = gumbel_params(cfg) if self.kind == "gumbel" else None
        self.selected_actions = None
        self._ws = {}

    # workspace per (B, agent) -------------------------------------------------------------
    def workspace(self, B):
        key = (B, id(self.mu_zero), self.mu_zero.dtype)
        ws = self._ws.get(key)
        if ws is None:
            ws = SearchWorkspace(self, B)
            self._ws = {key: ws}
        return ws

    def search(self, hidden_state, action_mask=None, training_iteration=0, noise=None):
        B = hidden_state.shape[0]
        ws = self.workspace(B)
        ws.load_root(hidden_state)
        if noise is not None:  # injected Dirichlet rows (Gumbel mode: variates) (B, 3), any array-like
            noise = torch.as_tensor(np.asarray(noise, dtype=np.float32), device=ws.agent.device).contiguous()
        if self.kind == "gumbel":
            values, counts, actions = ws.run_gumbel(self.search_id, noise)
            self.selected_actions = actions.cpu()
        else:
            values, counts = ws.run(self.search_id, noise)
        self.search_id += 1
        return values.cpu(), counts.cpu()


class SearchWorkspace:
    """Buffers + launch sequence of one search over B envs (NHWC latents)."""

    def __init__(self, search, B):
        agent = search.mu_zero
        self.s = search
        self.agent = agent
        dev = agent.device
        p = agent.packed
        self.B, self.S = B, search.num_simulations
        self.n = p.lh * p.lw * p.c1
        self.tree = TreeState(B, self.S, search.c1, search.c2, dev)
        self.pool = torch.empty(B * (self.S + 1) * self.n, dtype=p.tdt, device=dev)
        self.cur = torch.empty(B * self.n, dtype=p.tdt, device=dev)
        self.r = torch.empty(B, dtype=torch.float32, device=dev)
        self.v = torch.empty(B, dtype=torch.float32, device=dev)
        self.pi = torch.empty(B, 3, dtype=torch.float32, device=dev)
        self.runner = agent.runner(B, p.lh * 4, p.lw * 4)
        self.gumbel = GumbelState(self.tree, *search.gumbel, dev) if search.gumbel is not None else None
        # (f32(1 - noise_weight), f32(noise_weight)) of the root expansion, read on the device: the schedule
        # (train_torch.py:134-135) needs no new graph capture
        self.root_w_dev = torch.zeros(2, dtype=torch.float32, device=dev)
        self._noise_weight = None
        # backup + next select ride on the fused prediction launch (MZBA_TREE_FUSION=0: separate kernels)
        self.use_tree_fusion = os.environ.get("MZBA_TREE_FUSION", "1") != "0"
        # fused steps: latents straight from / to their node-pool slots (MZBA_POOL_SLOTS=0: through `cur`,
        # the round-3 second-session form, for A/B runs)
        self.use_pool_slots = os.environ.get("MZBA_POOL_SLOTS", "1") != "0"

    def load_root(self, hidden_state):
        """NCHW (B,C,h,w) latent -> pool slot 0 (NHWC)."""
        p = self.agent.packed
        B = self.B
        x = hidden_state.to(self.agent.device).permute(0, 2, 3, 1).reshape(B, self.n).to(p.tdt)
        self.pool.view(B, self.S + 1, self.n)[:, 0].copy_(x)

    def root_slot(self):
        return self.pool.view(self.B, self.S + 1, self.n)[:, 0]

    def sync_noise_weight(self, w=None):
        """Bring root_w_dev up to `w`, by default the search object's noise_weight (train_torch.py:134-135 sets it
        there)."""
        w = self.s.noise_weight if w is None else w
        if w != self._noise_weight:
            self._noise_weight = w
            self.root_w_dev.copy_(torch.tensor([np.float32(1 - w), np.float32(w)], dtype=torch.float32))

    def search(self, search_id, noise=None, ctx=None):
        """The configured search of the acting and reanalyse loops -> (values, counts): run_gumbel, or run with the
        root weights of root_w_dev (sync_noise_weight)."""
        if self.s.kind == "gumbel":
            return self.run_gumbel(search_id, noise, ctx=ctx)[:2]
        return self.run(search_id, noise, ctx=ctx, w_dev=self.root_w_dev)

    def _dynamics(self, sim, direct):
        """Simulation sim's dynamics step: parent latents gathered from the node pool, the new latent to slot
        sim + 1 (and to `cur` unless `direct`), decoded rewards to r."""
        env_stride = (self.S + 1) * self.n
        self.runner.dynamics(self.pool, self.tree.leaf_action, None if direct else self.cur, self.r,
                             slot=self.tree.leaf_parent, env_stride=env_stride, slot_stride=self.n, pool=self.pool,
                             pool_env_stride=env_stride, pool_slot=sim + 1)

    def run(self, search_id, noise=None, ctx=None, w_dev=None):
        """mcts.py:24-71 on the device. Root latent must be in pool slot 0. With `ctx` the
        search id is read on the device (HIP-graph replayable launch sequence); `w_dev` (device
        f32[2]) supplies the root mixing weights (f32(1 - noise_weight), f32(noise_weight))."""
        s = self.s
        B, S, n = self.B, self.S, self.n
        ta = self.tree.args(s.env_offset, search_id, s.seed, ctx)
        rn = self.runner
        slots = self.pool.view(B, S + 1, n)  # node pool: slot 0 the root, slot s + 1 the node of simulation s
        fused = rn.fused_ok() and self.use_tree_fusion
        direct = fused and self.use_pool_slots
        # the fused steps read each latent from its node-pool slot and the dynamics step writes the new
        # latent there only (no copy into `cur`: one latent write per env and simulation, not two)
        rn.prediction(slots[:, 0] if direct else self._root_copy(slots), self.pi, self.v)  # _expand_root_nodes mcts.py:95-100
        w_pol = float(np.float32(1 - s.noise_weight))
        w_noise = float(np.float32(s.noise_weight))
        self.tree.root(ta, self.v, self.pi, noise, w_pol, w_noise, s.dirchlet_alpha, w_dev)
        gamma = float(np.float32(s.discount))
        for sim in range(S):
            if sim > 0 and not fused:
                self.tree.select(ta, sim)
            self._dynamics(sim, direct)
            if fused:  # prediction + backup(sim) + select(sim + 1) in one launch
                rn.prediction(slots[:, sim + 1] if direct else self.cur, self.pi, self.v, tree=(ta, sim, gamma, self.r))
            else:
                rn.prediction(self.cur, self.pi, self.v)
                self.tree.backup(ta, sim, self.r, self.v, self.pi, gamma)
        self.tree.results(ta)
        return self.tree.values, self.tree.counts

    def run_gumbel(self, search_id, g=None, ctx=None, record=None):
        """The Gumbel search on the device; root latent in pool slot 0. Returns (values, the
        improved policy in 24-bit fixed point i64[B][3], chosen actions i64[B]). `g` (device f32 [B][3]) injects
        the root's Gumbel variates in place of the device draw; `ctx` as in run(). Per simulation: the dynamics
        step, the prediction step without a tree, one tree launch (backup + the next selection). `record` (a
        dict, tests) receives copies of the decoded network outputs: v_root, pi_root and lists r, v, pi by
        simulation, what replay_search_gumbel takes."""
        s, gs = self.s, self.gumbel
        if gs is None:
            raise RuntimeError("run_gumbel: the search was not configured with cfg['search']['kind'] == 'gumbel'")
        B, S, n = self.B, self.S, self.n
        ta = (s.env_offset, search_id, s.seed, ctx)
        rn = self.runner
        slots = self.pool.view(B, S + 1, n)
        direct = rn.fused_ok() and self.use_pool_slots
        rn.prediction(slots[:, 0] if direct else self._root_copy(slots), self.pi, self.v)
        if record is not None:
            record.update(v_root=self.v.clone(), pi_root=self.pi.clone(), r=[], v=[], pi=[])
        gs.root(ta, self.v, self.pi, g)
        gamma = float(np.float32(s.discount))
        for sim in range(S):
            self._dynamics(sim, direct)
            rn.prediction(slots[:, sim + 1] if direct else self.cur, self.pi, self.v)
            if record is not None:
                for k, t in (("r", self.r), ("v", self.v), ("pi", self.pi)):
                    record[k].append(t.clone())
            gs.step(ta, sim, self.r, self.v, self.pi, gamma)
        gs.results(ta)
        return self.tree.values, self.tree.counts, gs.actions

    def _root_copy(self, slots):
        """The root latents contiguous in `cur` (the unfused launches read contiguous latents)."""
        self.cur.view(self.B, self.n).copy_(slots[:, 0])
        return self.cur


def replay_search(B, S, cfg, v_root, pi_root, noise, r, v, pi, seed, search_id, env_offset=0, device="cuda"):
    """Tree kernels driven by recorded decoded network outputs (fixture replay mode):
    the same select/backup/results launches as SearchWorkspace.run, without nets."""
    L.require_gpu()
    t = TreeState(B, S, cfg["search"]["c1"], cfg["search"]["c2"], device)
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=device)  # noqa: E731
    ta = t.args(env_offset, search_id, seed)
    t.root(ta, dv(v_root), dv(pi_root), dv(noise), float(np.float32(1 - 0.175)), float(np.float32(0.175)), 0.25)
    gamma = float(np.float32(cfg["search"]["discount_factor"]))
    leaf = np.zeros((S, B), dtype=np.int64)
    for sim in range(S):
        if sim > 0:
            t.select(ta, sim)
        leaf[sim] = t.leaf_action.cpu().numpy()
        t.backup(ta, sim, dv(r[sim]), dv(v[sim]), dv(pi[sim]), gamma)
    t.results(ta)
    return t.values.cpu().numpy(), t.counts.cpu().numpy(), leaf


def replay_search_gumbel(B, S, cfg, v_root, pi_root, g, r, v, pi, seed, search_id, env_offset=0, device="cuda"):
    """The Gumbel tree kernels driven by recorded decoded network outputs, without nets: r / v / pi [S][B](x3) are
    indexed by simulation. `g` f32 [B][3] injects the root's Gumbel variates (None: the device draw). Returns a dict:
    values, counts (fixed point), actions, root_n, leaf_parent / leaf_action [S][B], variates, g, considered."""
    L.require_gpu()
    t = TreeState(B, S, cfg["search"]["c1"], cfg["search"]["c2"], device)
    gs = GumbelState(t, *gumbel_params(cfg), device)
    dv = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=device)  # noqa: E731
    ta = (env_offset, search_id, seed, None)
    gs.root(ta, dv(v_root), dv(pi_root), dv(g))
    gamma = float(np.float32(cfg["search"]["discount_factor"]))
    lp = torch.empty(S, B, dtype=torch.int32, device=device)
    la = torch.empty(S, B, dtype=torch.int32, device=device)
    rd, vd, pd = dv(r), dv(v), dv(pi)
    for sim in range(S):
        lp[sim].copy_(t.leaf_parent)
        la[sim].copy_(t.leaf_action)
        gs.step(ta, sim, rd[sim], vd[sim], pd[sim], gamma)
    gs.results(ta)
    host = lambda x: x.cpu().numpy()  # noqa: E731
    return dict(values=host(t.values), counts=host(t.counts), actions=host(gs.actions), root_n=host(gs.root_n),
                leaf_parent=host(lp), leaf_action=host(la), variates=host(gs.variates), g=host(gs.g),
                considered=host(gs.considered))
