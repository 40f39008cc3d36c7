"""Oracle and cases of the Gumbel search tests (tests/test_cpu_gumbel.py, tests/test_gpu_gumbel.py). Plain Python /
numpy; nothing here calls the library.

* `schedule`: the sequential-halving visit schedule seq[0..S) of DESIGN.md §15, restated.
* `search_one`: DESIGN.md §15 for one env on recorded network outputs, every operation passed through `rd`:
  the identity gives the f64 statement, `r32` (round to f32 after every operation; +, -, *, / of two f32 rounded
  from the f64 result are the correctly rounded f32 results, log / exp correctly rounded ones) the f32 restatement
  used for calibration. Inputs are f32 values in both. It returns the (parent, action) leaf of every simulation, root
  N, the chosen action, pi', the value, and the smallest top-two margin met in any argmax (the considered-set cut
  included).
* `gen_cases`: the seeded case generator; `CASE_SETS`: the committed case set shared by the CPU and GPU tests;
  `oracle`: the cached oracle results of one set.
"""
import functools
import math

import numpy as np

GAMMA = 0.985
AMBIGUOUS = 1e-3     # a case whose smallest f64 argmax margin is below this is ambiguous
Q24 = float(1 << 24)

# (B, S, m, env_offset, seed): B 1 / 5 / 257 (257 crosses a 256-thread block), S 1 .. 16 and one 50, m 2 and 3
CASE_SETS = [
    (1, 1, 3, 0, 11), (5, 1, 2, 0, 12), (5, 2, 3, 0, 13), (257, 2, 2, 0, 14), (257, 4, 3, 0, 15), (1, 4, 2, 0, 16),
    (257, 8, 3, 1000, 17), (5, 8, 2, 7, 18), (257, 16, 3, 0, 19), (257, 16, 2, 0, 20), (257, 50, 3, 0, 21),
]


def r32(x):
    return float(np.float32(x))


def ident(x):
    return x


def schedule(S, m):
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


class _Node:
    __slots__ = ("Q", "P", "R", "N", "child", "V")

    def __init__(self, P, V):
        self.Q = [0.0, 0.0, 0.0]
        self.P = list(P)
        self.R = [0.0, 0.0, 0.0]
        self.N = [0, 0, 0]
        self.child = [-1, -1, -1]
        self.V = V


def _argmax(scores, cand, track):
    """Lowest index of the largest score among `cand`; the top-two margin goes to track[0]."""
    best = cand[0]
    for a in cand[1:]:
        if scores[a] > scores[best]:
            best = a
    if len(cand) > 1:
        second = max(scores[a] for a in cand if a != best)
        track[0] = min(track[0], scores[best] - second)
    return best


def _logits(nd, rd):
    return [rd(math.log(max(p, 1e-37))) for p in nd.P]


def _sigma(nd, c_visit, c_scale, rd):
    n = sum(nd.N)
    v_mix = nd.V
    if n > 0:
        sp, spq = 0.0, 0.0
        for a in range(3):
            if nd.N[a] > 0:
                sp = rd(sp + nd.P[a])
                spq = rd(spq + rd(nd.P[a] * nd.Q[a]))
        wq = rd(spq / sp)
        v_mix = rd(rd(v_mix + rd(float(n) * wq)) / float(1 + n))
    cq = [nd.Q[a] if nd.N[a] > 0 else v_mix for a in range(3)]
    mn, mx = min(cq), max(cq)
    den = max(rd(mx - mn), rd(1e-8))
    k = rd(rd(c_visit + float(max(nd.N))) * c_scale)
    return cq, [rd(k * rd(rd(cq[a] - mn) / den)) for a in range(3)]


def _improved(l, sigma, rd):
    x = [rd(l[a] + sigma[a]) for a in range(3)]
    mx = max(x)
    e = [rd(math.exp(rd(x[a] - mx))) for a in range(3)]
    den = rd(rd(e[0] + e[1]) + e[2])
    return [rd(e[a] / den) for a in range(3)]


def search_one(v_root, pi_root, z, r, v, pi, S, m, rd=ident, c_visit=50.0, c_scale=1.0, scale=1.0, gamma=GAMMA):
    """One env: z[3] the root's standard Gumbel variates, r[S], v[S], pi[S][3] the decoded network outputs of the
    node each simulation creates."""
    c_visit, c_scale, scale = rd(c_visit), rd(c_scale), rd(scale)
    gamma = r32(gamma)  # the f32 discount in both statements, as the kernels take it
    seq = schedule(S, m)
    track = [math.inf]
    nodes = [_Node([float(p) for p in pi_root], float(v_root))]
    g = [rd(scale * float(z[a])) for a in range(3)]
    l0 = _logits(nodes[0], rd)
    gl = [rd(g[a] + l0[a]) for a in range(3)]
    considered = [0, 1, 2]
    if m == 2:
        w = 0
        for a in (1, 2):
            if gl[a] <= gl[w]:
                w = a
        considered = [a for a in range(3) if a != w]
        track[0] = min(track[0], min(gl[a] for a in considered) - gl[w])

    def root_pick(want):
        _, sg = _sigma(nodes[0], c_visit, c_scale, rd)
        cand = [a for a in considered if nodes[0].N[a] == want]
        assert cand, "no considered action with N == seq[s]"
        return _argmax([rd(gl[a] + sg[a]) for a in range(3)], cand, track)

    def interior_pick(nd):
        _, sg = _sigma(nd, c_visit, c_scale, rd)
        p = _improved(_logits(nd, rd), sg, rd)
        d = float(1 + sum(nd.N))
        return _argmax([rd(p[a] - rd(float(nd.N[a]) / d)) for a in range(3)], [0, 1, 2], track)

    leaves = []
    for s in range(S):
        node, a, path = 0, root_pick(seq[s]), []
        while nodes[node].child[a] >= 0:
            path.append((node, a))
            node = nodes[node].child[a]
            a = interior_pick(nodes[node])
        nodes[node].child[a] = s + 1
        leaves.append((node, a))
        # backup: the new node, the parent edge's reward, the return up the path
        nodes.append(_Node([float(p) for p in pi[s]], float(v[s])))
        nodes[node].R[a] = float(r[s])
        G = float(v[s])
        for pn, pa in reversed(path + [(node, a)]):
            e = nodes[pn]
            G = rd(rd(G * gamma) + e.R[pa])
            e.Q[pa] = rd(rd(rd(float(e.N[pa]) * e.Q[pa]) + G) / float(e.N[pa] + 1))
            e.N[pa] += 1
    root = nodes[0]
    cq, sg = _sigma(root, c_visit, c_scale, rd)
    nmax = max(root.N[a] for a in considered)
    action = _argmax([rd(gl[a] + sg[a]) for a in range(3)], [a for a in considered if root.N[a] == nmax], track)
    p = _improved(l0, sg, rd)
    value = rd(rd(rd(p[0] * cq[0]) + rd(p[1] * cq[1])) + rd(p[2] * cq[2]))
    return dict(leaves=leaves, root_n=list(root.N), action=action, pi=p, value=value, margin=track[0],
                considered=sum(1 << a for a in considered), g=g)


def gen_cases(B, S, seed):
    """Recorded inputs of B envs, all f32: prior logits N(0, 1.5^2) through a softmax, values U(-1, 3), rewards
    {0, 0, 0, +-1} * U(0.5, 1), Gumbel variates from uniforms."""
    rng = np.random.default_rng(seed)

    def softmax(x):
        e = np.exp(x - x.max(-1, keepdims=True))
        return (e / e.sum(-1, keepdims=True)).astype(np.float32)

    u = rng.random((B, 3))
    return dict(
        v_root=rng.uniform(-1, 3, B).astype(np.float32),
        pi_root=softmax(rng.normal(0, 1.5, (B, 3))),
        z=(-np.log(-np.log(u))).astype(np.float32),
        r=(rng.choice(np.array([0.0, 0.0, 0.0, 1.0, -1.0]), (S, B)) * rng.uniform(0.5, 1, (S, B))).astype(np.float32),
        v=rng.uniform(-1, 3, (S, B)).astype(np.float32),
        pi=softmax(rng.normal(0, 1.5, (S, B, 3))))


def run_cases(c, S, m, rd=ident, **kw):
    """search_one over a case dict -> arrays: leaf_parent / leaf_action [S][B], root_n [B][3], action [B], pi [B][3],
    value [B], margin [B], considered [B], counts [B][3] (the 24-bit fixed-point packing of pi')."""
    B = len(c["v_root"])
    res = [search_one(c["v_root"][b], c["pi_root"][b], c["z"][b], c["r"][:, b], c["v"][:, b], c["pi"][:, b], S, m,
                      rd, **kw) for b in range(B)]
    pi = np.array([x["pi"] for x in res], np.float64)
    return dict(
        leaf_parent=np.array([[x["leaves"][s][0] for x in res] for s in range(S)], np.int64).reshape(S, B),
        leaf_action=np.array([[x["leaves"][s][1] for x in res] for s in range(S)], np.int64).reshape(S, B),
        root_n=np.array([x["root_n"] for x in res], np.int64), action=np.array([x["action"] for x in res], np.int64),
        pi=pi, value=np.array([x["value"] for x in res], np.float64),
        margin=np.array([x["margin"] for x in res], np.float64),
        considered=np.array([x["considered"] for x in res], np.int64), counts=np.rint(pi * Q24).astype(np.int64),
        g=np.array([x["g"] for x in res], np.float64))


@functools.lru_cache(maxsize=None)
def oracle(i, f32=False):
    """(cases, results) of CASE_SETS[i]: the f64 statement, or the f32 restatement. Computed once; read-only."""
    B, S, m, _, seed = CASE_SETS[i]
    c = gen_cases(B, S, seed)
    return c, run_cases(c, S, m, r32 if f32 else ident)


def ambiguous_share(sets):
    """Share of ambiguous cases (f64 margin < AMBIGUOUS) pooled over the case sets `sets` (indices)."""
    mg = np.concatenate([oracle(i)[1]["margin"] for i in sets])
    return float((mg < AMBIGUOUS).mean())


SMALL_S = [i for i, cs in enumerate(CASE_SETS) if cs[1] <= 16]
LARGE_S = [i for i, cs in enumerate(CASE_SETS) if cs[1] > 16]
