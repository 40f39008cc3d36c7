// Gumbel search on the latent tree, one thread per env, trees in HBM as mcts.hip's.
//
// The root samples its actions without replacement (top m of g + l, g Gumbel noise, l = log P) and visits them by
// sequential halving along a host-built schedule seq[0..S); interior nodes take the deterministic improved-policy
// rule. The tree is mcts.hip's 64-byte Node; its 4 spare bytes (`pad`) hold the node's own value V (f32 bits), the
// decoded value head output at the node's creation. Every argmax takes the lowest index on a tie: no random
// tie-breaks, no `calls` counter. Every f32 expression is evaluated op by op (-ffp-contract=off):
//   l_a   = logf(max(P_a, 1e-37))
//   v_mix = V (no visits), else (V + f32(n) * (sum_vis(P_a Q_a) / sum_vis(P_a))) / f32(1 + n), sums in index order
//   cq_a  = N_a > 0 ? Q_a : v_mix;  sigma_a = ((c_visit + f32(max N)) * c_scale) * ((cq_a - min cq) / max(max cq - min cq, 1e-8))
//   pi'   = softmax(l + sigma), max-subtracted, denominator (e0 + e1) + e2
//   root: argmax over the considered a with N_a == seq[s] of (g_a + l_a) + sigma_a
//   interior: argmax of pi'_a - f32(N_a) / f32(1 + n)
// Backup is tree_backup_env unchanged, plus V of the new node.
#include "common.h"
#include "tree_dev.h"

namespace {

enum { MZ_STREAM_GUMBEL = 5 };  // Philox (global env, stream 5, search id, action); streams 0-4 are taken

struct GumbelArgs {
  float* g;              // [B][3] gumbel_scale * variate
  uint8_t* considered;   // [B] bit a: action a is in the considered set
  const int32_t* seq;    // [S] root visit schedule
  int m;
  float c_visit, c_scale, gumbel_scale;
};

MZ_DEV float node_value(const Node& nd) { return __int_as_float(nd.pad); }

// completed Q and sigma of one node
MZ_DEV void gumbel_sigma(const Node& nd, const GumbelArgs& ga, float* cq, float* sigma) {
  const int n = nd.N[0] + nd.N[1] + nd.N[2];
  float v_mix = node_value(nd);
  if (n > 0) {
    float sp = 0.f, spq = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
      if (nd.N[a] > 0) {
        sp = sp + nd.P[a];
        spq = spq + nd.P[a] * nd.Q[a];
      }
    const float wq = spq / sp;
    v_mix = (v_mix + (float)n * wq) / (float)(1 + n);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) cq[a] = nd.N[a] > 0 ? nd.Q[a] : v_mix;
  const float mn = fminf(fminf(cq[0], cq[1]), cq[2]);
  const float mx = fmaxf(fmaxf(cq[0], cq[1]), cq[2]);
  const float den = fmaxf(mx - mn, 1e-8f);
  const int nmax = max(max(nd.N[0], nd.N[1]), nd.N[2]);
  const float k = (ga.c_visit + (float)nmax) * ga.c_scale;
#pragma unroll
  for (int a = 0; a < 3; ++a) sigma[a] = k * ((cq[a] - mn) / den);
}

MZ_DEV void gumbel_logits(const Node& nd, float* l) {
#pragma unroll
  for (int a = 0; a < 3; ++a) l[a] = logf(fmaxf(nd.P[a], 1e-37f));
}

// pi' = softmax(l + sigma)
MZ_DEV void gumbel_improved(const float* l, const float* sigma, float* p) {
  float x[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) x[a] = l[a] + sigma[a];
  const float mx = fmaxf(fmaxf(x[0], x[1]), x[2]);
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = expf(x[a] - mx);
  const float den = (p[0] + p[1]) + p[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) p[a] = p[a] / den;
}

// root: the considered action with N == want of largest (g + l) + sigma. One always exists for a schedule built by
// the host rule; should none, the lowest considered action keeps every index in range.
MZ_DEV int gumbel_root_pick(const Node& nd, const GumbelArgs& ga, const float* gl, int mask, int want) {
  float cq[3], sigma[3];
  gumbel_sigma(nd, ga, cq, sigma);
  int best = -1, first = 0;
  float bs = 0.f;
#pragma unroll
  for (int a = 2; a >= 0; --a)
    if ((mask >> a) & 1) first = a;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (((mask >> a) & 1) && nd.N[a] == want) {
      const float s = gl[a] + sigma[a];
      if (best < 0 || s > bs) { best = a; bs = s; }
    }
  return best < 0 ? first : best;
}

MZ_DEV int gumbel_interior_pick(const Node& nd, const GumbelArgs& ga) {
  float cq[3], sigma[3], l[3], p[3];
  gumbel_sigma(nd, ga, cq, sigma);
  gumbel_logits(nd, l);
  gumbel_improved(l, sigma, p);
  const float d = (float)(1 + (nd.N[0] + nd.N[1] + nd.N[2]));
  int best = 0;
  float bs = p[0] - (float)nd.N[0] / d;
#pragma unroll
  for (int a = 1; a < 3; ++a) {
    const float s = p[a] - (float)nd.N[a] / d;
    if (s > bs) { best = a; bs = s; }
  }
  return best;
}

template <typename T> MZ_DEV T sel3(T x, T y, T z, int a) { return a == 0 ? x : (a == 1 ? y : z); }

// x, y or z by a, field by field (selects on registers: no indexed access to a register struct)
MZ_DEV Node node_sel(const Node& x, const Node& y, const Node& z, int a) {
  Node r;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r.Q[i] = sel3(x.Q[i], y.Q[i], z.Q[i], a);
    r.P[i] = sel3(x.P[i], y.P[i], z.P[i], a);
    r.R[i] = sel3(x.R[i], y.R[i], z.R[i], a);
    r.N[i] = sel3(x.N[i], y.N[i], z.N[i], a);
    r.child[i] = sel3(x.child[i], y.child[i], z.child[i], a);
  }
  r.pad = sel3(x.pad, y.pad, z.pad, a);
  return r;
}

// the walk of simulation sim >= 1: the schedule's root action, then the interior rule through expanded children;
// slot sim + 1 is claimed for the new leaf and leaf_parent / leaf_action / depth / path are written as
// tree_select_env writes them. A walk descends at most sim levels (the tree holds sim + 1 nodes). The level's cost
// is a dependent node load plus the pick's arithmetic (three logf, three expf, eleven divisions); the three children
// of a node are loaded while its pick is computed, so a level costs the longer of the two, not their sum.
MZ_DEV void gumbel_select_env(const TreeArgs& t, const GumbelArgs& ga, int sim, int b) {
  Node* tree = t.nodes + (size_t)b * (t.S + 1);
  int32_t* path = t.path + (size_t)b * (t.S + 1);
  // child a of p, or the root where there is none (a load that is never used, always in range)
  auto kid = [&](const Node& p, int a) {
    const int c = p.child[a];
    return tree[(c >= 0 && c <= sim) ? c : 0];
  };
  Node nd = tree[0];
  Node k0 = kid(nd, 0), k1 = kid(nd, 1), k2 = kid(nd, 2);
  float gl[3];
  gumbel_logits(nd, gl);
#pragma unroll
  for (int a = 0; a < 3; ++a) gl[a] = ga.g[b * 3 + a] + gl[a];
  int a = gumbel_root_pick(nd, ga, gl, ga.considered[b], ga.seq[sim]);
  int node = 0, d = 0;
  for (int it = 0;; ++it) {
    const int c = sel3(nd.child[0], nd.child[1], nd.child[2], a);
    if (c >= 0 && c <= sim && it < sim) {
      path[d++] = (node << 2) | a;
      node = c;
      nd = node_sel(k0, k1, k2, a);
      k0 = kid(nd, 0); k1 = kid(nd, 1); k2 = kid(nd, 2);
      a = gumbel_interior_pick(nd, ga);
    } else {
      tree[node].child[a] = sim + 1;
      t.leaf_parent[b] = node;
      t.leaf_action[b] = a;
      t.depth[b] = d;
      break;
    }
  }
}

__global__ void gumbel_root_kernel(TreeArgs t, GumbelArgs ga, const float* __restrict__ v_root,
                                   const float* __restrict__ pi_root, const float* __restrict__ g_in,
                                   float* __restrict__ g_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  float z[3];  // standard Gumbel variates -log(-log u)
  if (g_in) {
    z[0] = g_in[b * 3]; z[1] = g_in[b * 3 + 1]; z[2] = g_in[b * 3 + 2];
  } else {
    const uint32_t sid = (uint32_t)tree_search_id(t);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      // u = ((x >> 8) + 0.5) / 2^24 in (0, 1); in double: f32 would round the top half of the range to 1
      const uint32_t x = mz_u32((uint32_t)(b + t.env_offset), MZ_STREAM_GUMBEL, sid, (uint32_t)a, t.seed);
      const double u = ((double)(x >> 8) + 0.5) * (1.0 / 16777216.0);
      z[a] = (float)(-log(-log(u)));
    }
  }
  if (g_out) { g_out[b * 3] = z[0]; g_out[b * 3 + 1] = z[1]; g_out[b * 3 + 2] = z[2]; }
  Node nd;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    nd.Q[a] = 0.f; nd.P[a] = pi_root[b * 3 + a]; nd.R[a] = 0.f; nd.N[a] = 0; nd.child[a] = -1;
  }
  nd.pad = __float_as_int(v_root[b]);
  float g[3], gl[3];
  gumbel_logits(nd, gl);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    g[a] = ga.gumbel_scale * z[a];
    ga.g[b * 3 + a] = g[a];
    gl[a] = g[a] + gl[a];
  }
  int mask = 7;
  if (ga.m == 2) {  // drop the smallest g + l; among equal ones the highest index
    int w = 0;
    if (gl[1] <= gl[w]) w = 1;
    if (gl[2] <= gl[w]) w = 2;
    mask &= ~(1 << w);
  }
  ga.considered[b] = (uint8_t)mask;
  const int a0 = gumbel_root_pick(nd, ga, gl, mask, ga.seq[0]);
  nd.child[a0] = 1;  // simulation 0's node, linked
  t.nodes[(size_t)b * (t.S + 1)] = nd;
  t.root_sum[b] = v_root[b];
  t.leaf_parent[b] = 0;
  t.leaf_action[b] = a0;
  t.depth[b] = 0;
}

// backup(sim) and, when sim + 1 < S, select(sim + 1). One wave per block: every node access of a wave is 64 separate
// 64-byte lines (envs are (S + 1) nodes apart), so the kernel is bound by line transactions per CU, and 4096 envs in
// 256-thread blocks would sit on 16 CUs (S = 50, 4096 envs: 1.19 ms per acting step over PUCT with 256-thread blocks,
// 0.62 ms with 64; profiles/r11/gumbel/).
constexpr int STEP_BLOCK = 64;
__global__ void gumbel_step_kernel(TreeArgs t, GumbelArgs ga, int sim, const float* __restrict__ r,
                                   const float* __restrict__ v, const float* __restrict__ pi, float gamma) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  const float vb = v[b];
  tree_backup_env(t, sim, b, r[b], vb, pi + b * 3, gamma);
  t.nodes[(size_t)b * (t.S + 1) + sim + 1].pad = __float_as_int(vb);
  if (sim + 1 < t.S) gumbel_select_env(t, ga, sim + 1, b);
}

__global__ void gumbel_results_kernel(TreeArgs t, GumbelArgs ga, int64_t* __restrict__ counts,
                                      float* __restrict__ values, int64_t* __restrict__ action,
                                      int32_t* __restrict__ root_n) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  const Node nd = t.nodes[(size_t)b * (t.S + 1)];
  float cq[3], sigma[3], l[3], p[3];
  gumbel_sigma(nd, ga, cq, sigma);
  gumbel_logits(nd, l);
  gumbel_improved(l, sigma, p);
  const int mask = ga.considered[b];
  int nmax = -1;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if ((mask >> a) & 1) nmax = max(nmax, nd.N[a]);
  int best = 0;
  float bs = 0.f;
  bool have = false;
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (((mask >> a) & 1) && nd.N[a] == nmax) {
      const float s = (ga.g[b * 3 + a] + l[a]) + sigma[a];
      if (!have || s > bs) { best = a; bs = s; have = true; }
    }
  action[b] = best;
  values[b] = (p[0] * cq[0] + p[1] * cq[1]) + p[2] * cq[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    counts[b * 3 + a] = llrintf(p[a] * 16777216.0f);  // pi' in 24-bit fixed point: exact in the ring's f32 row
    if (root_n) root_n[b * 3 + a] = nd.N[a];
  }
}

GumbelArgs gumbel_args(const mzba_gumbel* gm) {
  return GumbelArgs{gm->g, gm->considered, gm->seq, gm->m, gm->c_visit, gm->c_scale, gm->gumbel_scale};
}

bool gumbel_ok(const mzba_tree_step* ts, const mzba_gumbel* gm) {
  return tree_ok(ts) && gm && (gm->m == 2 || gm->m == 3) && gm->g && gm->considered && gm->seq;
}

}  // namespace

extern "C" {

int mzba_gumbel_root(const mzba_tree_step* ts, const mzba_gumbel* gm, const float* v_root, const float* pi_root,
                     const float* g_in, float* g_out, hipStream_t stream) {
  MZ_CHECK_ARG(gumbel_ok(ts, gm) && v_root && pi_root, -1);
  hipLaunchKernelGGL(gumbel_root_kernel, dim3((ts->B + 255) / 256), dim3(256), 0, stream, tree_args(ts),
                     gumbel_args(gm), v_root, pi_root, g_in, g_out);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_gumbel_step(const mzba_tree_step* ts, const mzba_gumbel* gm, const float* v, const float* pi,
                     hipStream_t stream) {
  MZ_CHECK_ARG(gumbel_ok(ts, gm) && ts->sim >= 0 && ts->sim < ts->S && ts->r && v && pi, -1);
  hipLaunchKernelGGL(gumbel_step_kernel, dim3((ts->B + STEP_BLOCK - 1) / STEP_BLOCK), dim3(STEP_BLOCK), 0, stream,
                     tree_args(ts), gumbel_args(gm), ts->sim, ts->r, v, pi, ts->gamma);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_gumbel_results(const mzba_tree_step* ts, const mzba_gumbel* gm, int64_t* counts, float* values,
                        int64_t* action, int32_t* root_n, hipStream_t stream) {
  MZ_CHECK_ARG(gumbel_ok(ts, gm) && counts && values && action, -1);
  hipLaunchKernelGGL(gumbel_results_kernel, dim3((ts->B + 255) / 256), dim3(256), 0, stream, tree_args(ts),
                     gumbel_args(gm), counts, values, action, root_n);
  MZ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
