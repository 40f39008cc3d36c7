// Prioritized replay on the device (MuZero, Appendix G; DESIGN.md "Prioritized replay").
//
// q f32[cap] lives in *slot* space: q[slot] = p^alpha for a live window, exactly 0 for a slot that holds no
// window, so the sampler scans all cap slots and needs neither the ring's start nor its length.
//   prio_init_kernel     q of the windows an ingest has just written: p = |value[0] - target[0]| + eps;
//   prio_update_kernel   q[slots[j]] = (td[j] + eps)^alpha after a minibatch (a slot outside [0, cap) is skipped);
//   the sampler, stratified inverse-CDF over the inclusive prefix sum C of q, in four launches:
//     prio_partials_kernel  a wave per 1024-slot block: the block's f64 sum and its last slot with q > 0;
//     prio_scan_kernel      one wave: inclusive scan P of the block sums, S = P[last], the last live slot;
//     prio_sample_kernel    a wave per sample: binary search of P, then the block's own prefix;
//     prio_weight_kernel    importance weights over the batch's largest.
// Every sum is f64 in one fixed order (no atomics), and the prefix is *consistent*: with lane l of a block's
// wave owning slots 16 l .. 16 l + 15,
//   C[i] = P[b - 1] + (off_l + s_k),  s_k = ((v_0 + v_1) + ...) + v_k,  off_{l + 1} = off_l + s_15,  off_0 = 0,
//   P[b] = P[b - 1] + off_64,
// so the last C of a lane is the next lane's base, the last C of a block is P[b], C never decreases, and
// C[i] > C[i - 1] only where q[i] > 0: "the first i with C[i] > t" is always a live slot.
// prio_q, a block's prefix (load16, shfl_f64, block_prefix) and the weight kernel are in prio_dev.h, shared with the
// archive's row sampler (archive_prio.hip).
#include "prio_dev.h"

namespace {

constexpr int MZ_STREAM_REPLAY = 4;

__global__ __launch_bounds__(256) void prio_init_kernel(float* __restrict__ q, const float* __restrict__ values,
                                                        const float* __restrict__ targets, int cap, int head, int j0,
                                                        int n, int K, float alpha, float eps) {
  const int j = j0 + blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const size_t slot = ((size_t)head + j) % cap;
  q[slot] = prio_q(fabsf(values[slot * K] - targets[slot * K]), eps, alpha);
}

__global__ __launch_bounds__(256) void prio_update_kernel(float* __restrict__ q, const int32_t* __restrict__ slots,
                                                          const float* __restrict__ td, int n, int cap, float alpha,
                                                          float eps) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int slot = slots[j];
  if (slot < 0 || slot >= cap) return;  // never a store outside q, whatever the caller handed over
  q[slot] = prio_q(td[j], eps, alpha);
}

// prio_update_kernel under the learner's step guard (guard.hip): a skipped step leaves q as it is
__global__ __launch_bounds__(256) void prio_update_g_kernel(float* __restrict__ q, const int32_t* __restrict__ slots,
                                                            const float* __restrict__ td, int n, int cap, float alpha,
                                                            float eps, const mzba_guard_block* __restrict__ blk) {
  if (blk->skip) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const int slot = slots[j];
  if (slot < 0 || slot >= cap) return;
  q[slot] = prio_q(td[j], eps, alpha);
}

__global__ __launch_bounds__(256) void prio_partials_kernel(const float* __restrict__ q, int cap, int nblk,
                                                            double* __restrict__ part, int32_t* __restrict__ lastpos) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nblk) return;  // whole waves leave; no barrier below
  float v[16];
  double s[16], full;
  load16(q, cap, b, lane, v);
  block_prefix(v, lane, s, full);
  int last = -1;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (v[k] > 0.f) last = b * PB + lane * 16 + k;
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  if (lane == 0) { part[b] = full; lastpos[b] = last; }
}

// one wave: lane l owns blocks [l per, (l + 1) per); P[b] = P[b - 1] + part[b] exactly (lane bases summed lane by
// lane), in place. lastpos[nblk] = the last slot of the ring with q > 0 (-1: none).
__global__ __launch_bounds__(64) void prio_scan_kernel(double* __restrict__ part, int32_t* __restrict__ lastpos,
                                                       int nblk) {
  const int lane = threadIdx.x, per = (nblk + 63) / 64;  // per <= 16 (cap <= 2^20)
  const int b0 = min(lane * per, nblk), cnt = min(b0 + per, nblk) - b0;
  double p[16];
  int last = -1;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    p[k] = k < cnt ? part[b0 + k] : 0.0;
    if (k < cnt) last = max(last, lastpos[b0 + k]);
  }
  // lanes take their turns one after the other, each continuing from the last P of the lane before, so that
  // P[b] = P[b - 1] + part[b] holds across lane borders too (registers only: at most 1024 dependent adds)
  double run = 0.0;
  for (int l = 0; l < 64; ++l) {
    if (l == lane) {
#pragma unroll
      for (int k = 0; k < 16; ++k) { run = run + p[k]; p[k] = run; }
    }
    run = shfl_f64(run, l);
  }
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (k < cnt) part[b0 + k] = p[k];
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  if (lane == 0) lastpos[nblk] = last;
}

__global__ __launch_bounds__(256) void prio_sample_kernel(const float* __restrict__ q, int cap, int nblk, int n,
                                                          float beta, int n_live, uint64_t seed, uint32_t step,
                                                          const uint32_t* __restrict__ step_dev,
                                                          const float* __restrict__ u_in, const double* __restrict__ P,
                                                          const int32_t* __restrict__ lastpos,
                                                          int32_t* __restrict__ slots, float* __restrict__ prob,
                                                          double* __restrict__ raw) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;  // whole waves leave; no barrier below
  if (step_dev) step = step_dev[0];
  const float u = u_in ? u_in[j] : mz_uniform((uint32_t)j, MZ_STREAM_REPLAY, step, 0, seed);
  const double S = P[nblk - 1];
  const double t = (((double)j + (double)u) / (double)n) * S;
  int slot;
  if (!(t < S)) {
    slot = lastpos[nblk];  // rounding put t at or beyond S (or S == 0): the last live slot
    if (slot < 0) slot = 0;
  } else {
    int lo = 0, hi = nblk - 1;  // first block with P[b] > t (P[nblk - 1] = S > t)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (P[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int b = lo;
    const double base = b ? P[b - 1] : 0.0;
    float v[16];
    double s[16], full;
    load16(q, cap, b, lane, v);
    const double off = block_prefix(v, lane, s, full);
    // base + (off + s[15]) of lane 63 is P[b] > t: some lane fires
    const unsigned long long m = __ballot(base + (off + s[15]) > t);
    const int hit = m ? __ffsll((long long)m) - 1 : 63;
    int k = 0;
    if (lane == hit) {
      while (k < 15 && !(base + (off + s[k]) > t)) ++k;
    }
    slot = b * PB + hit * 16 + __shfl(k, hit, 64);
    if (slot >= cap) slot = max(lastpos[nblk], 0);  // unreachable while q[i >= cap] reads as 0; keeps the gather inside
  }
  if (lane == 0) {
    const double pr = S > 0.0 ? (double)q[slot] / S : 0.0;
    slots[j] = slot;
    prob[j] = (float)pr;
    raw[j] = beta == 0.f ? 1.0 : pow((double)n_live * pr, -(double)beta);
  }
}

}  // namespace

extern "C" {

int mzba_replay_priority_init(float* q, const float* values, const float* targets, int cap, int head, int n_windows,
                              int K, float alpha, float eps, hipStream_t stream) {
  MZ_CHECK_ARG(q && values && targets && cap > 0 && head >= 0 && head < cap && n_windows >= 0 && K > 0 &&
                   alpha >= 0.f && eps >= 0.f, -1);
  if (n_windows == 0) return 0;
  const int j0 = n_windows > cap ? n_windows - cap : 0;  // mzba_replay_write's range
  hipLaunchKernelGGL(prio_init_kernel, dim3((n_windows - j0 + 255) / 256), dim3(256), 0, stream, q, values, targets,
                     cap, head, j0, n_windows, K, alpha, eps);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_replay_priority_update(float* q, const int32_t* slots, const float* td, int n, int cap, float alpha,
                                float eps, hipStream_t stream) {
  MZ_CHECK_ARG(q && slots && td && n >= 0 && cap > 0 && alpha >= 0.f && eps >= 0.f, -1);
  if (n == 0) return 0;
  hipLaunchKernelGGL(prio_update_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, q, slots, td, n, cap, alpha,
                     eps);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_replay_priority_update_g(float* q, const int32_t* slots, const float* td, int n, int cap, float alpha,
                                  float eps, const mzba_guard_block* block, hipStream_t stream) {
  MZ_CHECK_ARG(q && slots && td && block && n >= 0 && cap > 0 && alpha >= 0.f && eps >= 0.f, -1);
  if (n == 0) return 0;
  hipLaunchKernelGGL(prio_update_g_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, q, slots, td, n, cap, alpha,
                     eps, block);
  MZ_LAUNCH_CHECK();
  return 0;
}

long long mzba_replay_sample_ws_bytes(int cap, int n) {
  if (cap <= 0 || n <= 0) return -1;
  const long long nblk = (cap + PB - 1) / PB;
  return align16(nblk * 8) + align16((nblk + 1) * 4) + align16((long long)n * 8);
}

int mzba_replay_sample(const float* q, int cap, int n, float beta, int n_live, uint64_t seed, uint32_t step,
                       const uint32_t* step_dev, const float* u_in, int32_t* slots, float* prob, float* weight,
                       void* ws, long long ws_bytes, hipStream_t stream) {
  MZ_CHECK_ARG(q && slots && prob && weight && ws && cap > 0 && cap <= (1 << 20) && n > 0 && n <= (1 << 20) &&
                   beta >= 0.f, -1);
  MZ_CHECK_ARG(n_live > 0 && n_live <= cap, -3);  // an empty buffer (S == 0) is an error, not a launch
  MZ_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)ws & 15) == 0 && mzba_replay_sample_ws_bytes(cap, n) <= ws_bytes,
               -2);
  const int nblk = (cap + PB - 1) / PB;
  double* P = (double*)ws;
  int32_t* lastpos = (int32_t*)((char*)ws + align16((long long)nblk * 8));
  double* raw = (double*)((char*)lastpos + align16(((long long)nblk + 1) * 4));
  hipLaunchKernelGGL(prio_partials_kernel, dim3((nblk + 3) / 4), dim3(256), 0, stream, q, cap, nblk, P, lastpos);
  hipLaunchKernelGGL(prio_scan_kernel, dim3(1), dim3(64), 0, stream, P, lastpos, nblk);
  hipLaunchKernelGGL(prio_sample_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, q, cap, nblk, n, beta, n_live, seed,
                     step, step_dev, u_in, (const double*)P, (const int32_t*)lastpos, slots, prob, raw);
  hipLaunchKernelGGL(prio_weight_kernel, dim3(1), dim3(256), 0, stream, (const double*)raw, n, weight);
  MZ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
