// Learner step guard (layouts and contracts in include/mzba.h): what watches the optimizer
// step, on the device and inside the captured minibatch.
//   grad_stats_kernel     one streaming pass over the flat gradient: per chunk and segment, the f64 sum of squares
//                         and the non-finite count (fixed ownership, fixed lane assignment, fixed fold order);
//   guard_finish_kernel   one wave: folds the partials, norm, clip coefficient, skip, the device step counter, the
//                         learning rate of that step and Adam's seven scalars, into the stats block;
//   adam_guard*_kernel    learn.hip's Adam update on coef * grad, nothing stored on a skipped step;
//   guard_copy_kernel     the BatchNorm running statistics: snapshot before the minibatch, restore on a skipped step.
// The guarded priority update lives beside the plain one in replay_prio.hip.
#include <math.h>

#include "common.h"

namespace {

constexpr int GS_T = 256;                 // threads per workgroup
constexpr int GS_U = 16;                  // 16-byte loads per thread and chunk, all issued before the first use
constexpr int GS_CH = GS_T * 4 * GS_U;    // elements per chunk (16384: 64 KiB)
constexpr int GS_MAX_GRID = 1024;         // workgroups of a default launch (4 per CU: 256 KiB of loads in flight per CU)
constexpr long long GS_HEAD = 16;         // ws: {i32 loss_nonfinite, pad}, then f64 sums [8][chunks], i32 counts [8][chunks]

int g_forced_grid = 0;  // mzba_grad_stats_set_grid (tests)

struct SegBounds { long long b[MZBA_GUARD_MAX_SEG + 1]; };

MZ_DEV int nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

MZ_DEV double shfl_xor_f64(double x, int mask) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const int lo = __shfl_xor((int)(uint32_t)u, mask, 64), hi = __shfl_xor((int)(uint32_t)(u >> 32), mask, 64);
  return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}
MZ_DEV double shfl_f64(double x, int src) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const int lo = __shfl((int)(uint32_t)u, src, 64), hi = __shfl((int)(uint32_t)(u >> 32), src, 64);
  return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}

// This thread's share of chunk [c0, c0 + GS_CH): elements o = (u GS_T + tid) 4 + j, u ascending, into accumulator j.
// VEC: the whole chunk lies inside the segment and g + c0 is 16-byte aligned; else only elements in [lo, hi) are
// loaded (the others enter as +0.0, an exact addition: both forms give the same bits).
template <bool VEC>
MZ_DEV void chunk_accumulate(const float* __restrict__ g, long long c0, long long lo, long long hi, int tid,
                             double& sum, int& cnt) {
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  int c = 0;
  if (VEC) {
    const float4* g4 = reinterpret_cast<const float4*>(g + c0);
    float4 x[GS_U];
#pragma unroll
    for (int u = 0; u < GS_U; ++u) x[u] = g4[u * GS_T + tid];  // all in flight before the first use
#pragma unroll
    for (int u = 0; u < GS_U; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float f = (&x[u].x)[j];
        const double d = (double)f;
        a[j] = a[j] + d * d;  // the square of an f32 is exact in f64
        c += nonfinite(f);
      }
  } else {
#pragma unroll 2
    for (int u = 0; u < GS_U; ++u) {
      const long long e0 = c0 + (long long)(u * GS_T + tid) * 4;
      float x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) x[j] = e0 + j >= lo && e0 + j < hi ? g[e0 + j] : 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double d = (double)x[j];
        a[j] = a[j] + d * d;
        c += nonfinite(x[j]);
      }
    }
  }
  sum = (a[0] + a[1]) + (a[2] + a[3]);
  cnt = c;
}

__global__ __launch_bounds__(GS_T) void grad_stats_kernel(const float* __restrict__ g, long long n, SegBounds sb,
                                                          int nseg, long long nchunks, int vec_ok,
                                                          const float* __restrict__ loss4, double* __restrict__ psum,
                                                          int32_t* __restrict__ pcnt, int32_t* __restrict__ head) {
  __shared__ double sh_sum[GS_T / 64];
  __shared__ int sh_cnt[GS_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (blockIdx.x == 0 && tid == 0) {
    int bad = 0;
    if (loss4)
      for (int i = 0; i < 4; ++i) bad += nonfinite(loss4[i]);
    head[0] = bad;
  }
  for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {  // chunk c -> partial c, whatever the grid
    const long long c0 = c * GS_CH, c1 = min(n, c0 + (long long)GS_CH);
    for (int s = 0; s < nseg; ++s) {
      const long long lo = max(sb.b[s], c0), hi = min(sb.b[s + 1], c1);
      double total = 0.0;
      int count = 0;
      if (lo < hi) {  // the same for every thread of the workgroup
        double sum;
        int cnt;
        if (vec_ok && lo == c0 && hi == c0 + GS_CH)
          chunk_accumulate<true>(g, c0, lo, hi, tid, sum, cnt);
        else
          chunk_accumulate<false>(g, c0, lo, hi, tid, sum, cnt);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          sum = sum + shfl_xor_f64(sum, o);
          cnt += __shfl_xor(cnt, o, 64);
        }
        if (lane == 0) { sh_sum[wave] = sum; sh_cnt[wave] = cnt; }
        __syncthreads();
        if (tid == 0) {
          total = ((sh_sum[0] + sh_sum[1]) + sh_sum[2]) + sh_sum[3];
          count = ((sh_cnt[0] + sh_cnt[1]) + sh_cnt[2]) + sh_cnt[3];
        }
        __syncthreads();
      }
      if (tid == 0) {
        psum[(long long)s * nchunks + c] = total;
        pcnt[(long long)s * nchunks + c] = count;
      }
    }
  }
}

struct FinishArgs {
  double max_norm, lr0, rate, b1, b2, eps, wd;
  int skip_nonfinite, sched_steps;
};

__global__ __launch_bounds__(64) void guard_finish_kernel(const double* __restrict__ psum,
                                                          const int32_t* __restrict__ pcnt,
                                                          const int32_t* __restrict__ head, long long nchunks, int nseg,
                                                          FinishArgs fa, const float* __restrict__ lr_dev,
                                                          mzba_guard_block* __restrict__ blk) {
  const int lane = threadIdx.x;
  const long long per = (nchunks + 63) / 64;
  const long long k0 = min(lane * per, nchunks), k1 = min(k0 + per, nchunks);
  double seg_sum[MZBA_GUARD_MAX_SEG];
  int seg_cnt[MZBA_GUARD_MAX_SEG];
#pragma unroll
  for (int s = 0; s < MZBA_GUARD_MAX_SEG; ++s) { seg_sum[s] = 0.0; seg_cnt[s] = 0; }
  // eight chunks of every segment in flight per memory round trip (a segment at a time pays nseg times as many:
  // DESIGN.md section 13), then added in index order
  for (long long k = k0; k < k1; k += 8) {
    double v[MZBA_GUARD_MAX_SEG][8];
    int w[MZBA_GUARD_MAX_SEG][8];
#pragma unroll
    for (int s = 0; s < MZBA_GUARD_MAX_SEG; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = s < nseg && k + j < k1;
        v[s][j] = in ? psum[(long long)s * nchunks + k + j] : 0.0;
        w[s][j] = in ? pcnt[(long long)s * nchunks + k + j] : 0;
      }
#pragma unroll
    for (int s = 0; s < MZBA_GUARD_MAX_SEG; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) { seg_sum[s] = seg_sum[s] + v[s][j]; seg_cnt[s] += w[s][j]; }
  }
#pragma unroll
  for (int s = 0; s < MZBA_GUARD_MAX_SEG; ++s) {
    if (s >= nseg) continue;  // the same for every lane
    const double a = seg_sum[s];
    double tot = 0.0;
    for (int l = 0; l < 64; ++l) tot = tot + shfl_f64(a, l);  // lane totals in lane order
    int c = seg_cnt[s];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    seg_sum[s] = tot;
    seg_cnt[s] = c;
  }
  if (lane != 0) return;
  double total = 0.0;
  int bad = 0;
#pragma unroll
  for (int s = 0; s < MZBA_GUARD_MAX_SEG; ++s) {
    if (s < nseg) { total = total + seg_sum[s]; bad += seg_cnt[s]; }
    blk->seg_sumsq[s] = seg_sum[s];
    blk->seg_norm[s] = sqrt(seg_sum[s]);
    blk->seg_nonfinite[s] = seg_cnt[s];
  }
  const double norm = sqrt(total);
  double coef = 1.0;
  if (fa.max_norm < (double)INFINITY) {
    const double c = fa.max_norm / (norm + 1e-6);
    coef = c < 1.0 ? c : (c != c ? c : 1.0);  // torch.clamp(max = 1): a NaN stays
  }
  const int loss_bad = head[0];
  const int skip = fa.skip_nonfinite && (bad > 0 || loss_bad > 0);
  const int t = blk->t_applied + (skip ? 0 : 1);
  const int skipped = blk->skipped + (skip ? 1 : 0);
  double lr = fa.lr0;
  if (lr_dev) lr = (double)lr_dev[0];
  else if (fa.sched_steps > 0) lr = fa.lr0 * pow(fa.rate, (double)(t - 1) / (double)fa.sched_steps);
  const double bc1 = 1.0 - pow(fa.b1, (double)t), bc2 = 1.0 - pow(fa.b2, (double)t);
  blk->norm = norm;
  blk->coef = (float)coef;
  blk->nonfinite = bad;
  blk->loss_nonfinite = loss_bad;
  blk->skip = skip;
  blk->t_applied = t;
  blk->skipped = skipped;
  blk->lr = (float)lr;
  blk->sc[0] = (float)(-(lr / bc1));
  blk->sc[1] = (float)(1.0 - fa.b1);
  blk->sc[2] = (float)fa.b2;
  blk->sc[3] = (float)(1.0 - fa.b2);
  blk->sc[4] = (float)sqrt(bc2);
  blk->sc[5] = (float)fa.eps;
  blk->sc[6] = (float)fa.wd;
}

// learn.hip's adam_dev_kernel / adam4_kernel<true> with g = coef * grad; a skipped step touches nothing
__global__ void adam_guard_kernel(float* __restrict__ p, const float* __restrict__ grad, float* __restrict__ m,
                                  float* __restrict__ v, size_t n, const mzba_guard_block* __restrict__ blk) {
  if (blk->skip) return;
  const float coef = blk->coef;
  const float* sc = blk->sc;
  const float neg_step = sc[0], one_m_b1 = sc[1], b2 = sc[2], one_m_b2 = sc[3], bc2s = sc[4], eps = sc[5], wd = sc[6];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float pv = p[i];
    const float g = coef * grad[i] + wd * pv;
    const float mv = m[i] + one_m_b1 * (g - m[i]);
    const float vv = v[i] * b2 + (one_m_b2 * g) * g;
    m[i] = mv;
    v[i] = vv;
    p[i] = pv + (neg_step * mv) / (sqrtf(vv) / bc2s + eps);
  }
}

__global__ void adam_guard4_kernel(float4* __restrict__ p, const float4* __restrict__ grad, float4* __restrict__ m,
                                   float4* __restrict__ v, size_t n4, const mzba_guard_block* __restrict__ blk) {
  if (blk->skip) return;
  const float coef = blk->coef;
  const float* sc = blk->sc;
  const float neg_step = sc[0], one_m_b1 = sc[1], b2 = sc[2], one_m_b2 = sc[3], bc2s = sc[4], eps = sc[5], wd = sc[6];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 p4 = p[i], g4 = grad[i], m4 = m[i], v4 = v[i];
    float po[4], mo[4], vo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float pv = (&p4.x)[k];
      const float g = coef * (&g4.x)[k] + wd * pv;
      const float mk = (&m4.x)[k];
      const float mv = mk + one_m_b1 * (g - mk);
      const float vv = (&v4.x)[k] * b2 + (one_m_b2 * g) * g;
      mo[k] = mv;
      vo[k] = vv;
      po[k] = pv + (neg_step * mv) / (sqrtf(vv) / bc2s + eps);
    }
    m[i] = make_float4(mo[0], mo[1], mo[2], mo[3]);
    v[i] = make_float4(vo[0], vo[1], vo[2], vo[3]);
    p[i] = make_float4(po[0], po[1], po[2], po[3]);
  }
}

struct GuardRec {
  float* live;
  float* snap;
  int32_t n;
  int32_t pad;
};

template <bool RESTORE>
__global__ __launch_bounds__(256) void guard_copy_kernel(const GuardRec* __restrict__ tab,
                                                         const mzba_guard_block* __restrict__ blk) {
  if (RESTORE && !blk->skip) return;
  const GuardRec r = tab[blockIdx.x];
  const float* src = RESTORE ? r.snap : r.live;
  float* dst = RESTORE ? r.live : r.snap;
  for (int i = threadIdx.x; i < r.n; i += 256) dst[i] = src[i];
}

inline long long chunks_of(long long n) { return (n + GS_CH - 1) / GS_CH; }

}  // namespace

extern "C" {

int mzba_guard_block_bytes(void) { return (int)sizeof(mzba_guard_block); }

long long mzba_grad_stats_ws_bytes(long long n) {
  if (n <= 0) return -1;
  const long long nc = chunks_of(n);
  return (GS_HEAD + nc * MZBA_GUARD_MAX_SEG * 12 + 15) & ~15LL;
}

int mzba_grad_stats_set_grid(int blocks) {
  MZ_CHECK_ARG(blocks >= 0, -1);
  g_forced_grid = blocks;
  return 0;
}

int mzba_grad_stats(const float* g, long long n, const long long* seg_bounds, int nseg, const float* loss4, void* ws,
                    long long ws_bytes, hipStream_t stream) {
  MZ_CHECK_ARG(g && seg_bounds && ws && n > 0 && nseg >= 1 && nseg <= MZBA_GUARD_MAX_SEG, -1);
  MZ_CHECK_ARG(((uintptr_t)g & 3) == 0 && ((uintptr_t)ws & 15) == 0 && mzba_grad_stats_ws_bytes(n) <= ws_bytes, -2);
  SegBounds sb;
  for (int s = 0; s <= MZBA_GUARD_MAX_SEG; ++s) sb.b[s] = seg_bounds[s < nseg ? s : nseg];
  MZ_CHECK_ARG(sb.b[0] >= 0 && sb.b[nseg] <= n, -3);
  for (int s = 0; s < nseg; ++s) MZ_CHECK_ARG(sb.b[s] <= sb.b[s + 1], -3);
  const long long nc = chunks_of(n);
  long long grid;
  if (g_forced_grid > 0) {
    grid = g_forced_grid < nc ? g_forced_grid : nc;
  } else {  // every workgroup the same number of chunks (the last pass may be short by less than one each)
    const long long passes = (nc + GS_MAX_GRID - 1) / GS_MAX_GRID;
    grid = (nc + passes - 1) / passes;
  }
  double* psum = (double*)((char*)ws + GS_HEAD);
  int32_t* pcnt = (int32_t*)(psum + nc * MZBA_GUARD_MAX_SEG);
  hipLaunchKernelGGL(grad_stats_kernel, dim3((unsigned)grid), dim3(GS_T), 0, stream, g, n, sb, nseg, nc,
                     (int)(((uintptr_t)g & 15) == 0), loss4, psum, pcnt, (int32_t*)ws);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_guard_finish(const void* ws, long long ws_bytes, long long n, int nseg, mzba_guard_block* block,
                      double max_norm, int skip_nonfinite, double lr0, double sched_rate, int sched_steps,
                      const float* lr_dev, double b1, double b2, double eps, double wd, hipStream_t stream) {
  MZ_CHECK_ARG(ws && block && n > 0 && nseg >= 1 && nseg <= MZBA_GUARD_MAX_SEG, -1);
  MZ_CHECK_ARG(((uintptr_t)ws & 15) == 0 && ((uintptr_t)block & 7) == 0 && mzba_grad_stats_ws_bytes(n) <= ws_bytes, -2);
  MZ_CHECK_ARG(max_norm > 0.0 && sched_steps >= 0 && (sched_steps == 0 || sched_rate > 0.0) &&
                   !(sched_steps > 0 && lr_dev), -3);
  const long long nc = chunks_of(n);
  const double* psum = (const double*)((const char*)ws + GS_HEAD);
  const int32_t* pcnt = (const int32_t*)(psum + nc * MZBA_GUARD_MAX_SEG);
  FinishArgs fa;
  fa.max_norm = max_norm; fa.lr0 = lr0; fa.rate = sched_rate; fa.b1 = b1; fa.b2 = b2; fa.eps = eps; fa.wd = wd;
  fa.skip_nonfinite = skip_nonfinite != 0; fa.sched_steps = sched_steps;
  hipLaunchKernelGGL(guard_finish_kernel, dim3(1), dim3(64), 0, stream, psum, pcnt, (const int32_t*)ws, nc, nseg, fa,
                     lr_dev, block);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_adam_guard(float* p, const float* grad, float* m, float* v, long long n, const mzba_guard_block* block,
                    hipStream_t stream) {
  MZ_CHECK_ARG(p && grad && m && v && block && n >= 0, -1);
  if (n == 0) return 0;
  const bool a16 = (((uintptr_t)p | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  if (n % 4 == 0 && a16)
    hipLaunchKernelGGL(adam_guard4_kernel, dim3(grid_for((size_t)n / 4)), dim3(256), 0, stream, (float4*)p,
                       (const float4*)grad, (float4*)m, (float4*)v, (size_t)n / 4, block);
  else
    hipLaunchKernelGGL(adam_guard_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, stream, p, grad, m, v, (size_t)n,
                       block);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_guard_snapshot(const void* table, int ntensors, hipStream_t stream) {
  MZ_CHECK_ARG(table && ntensors >= 0 && ((uintptr_t)table & 7) == 0, -1);
  if (ntensors == 0) return 0;
  hipLaunchKernelGGL(guard_copy_kernel<false>, dim3(ntensors), dim3(256), 0, stream, (const GuardRec*)table,
                     (const mzba_guard_block*)nullptr);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_guard_restore(const void* table, int ntensors, const mzba_guard_block* block, hipStream_t stream) {
  MZ_CHECK_ARG(table && block && ntensors >= 0 && ((uintptr_t)table & 7) == 0, -1);
  if (ntensors == 0) return 0;
  hipLaunchKernelGGL(guard_copy_kernel<true>, dim3(ntensors), dim3(256), 0, stream, (const GuardRec*)table, block);
  MZ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
