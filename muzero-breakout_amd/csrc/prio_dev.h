// The pieces of the prioritized samplers that the ring's (replay_prio.hip) and the archive's
// (archive_prio.hip, §19) share: the priority itself, a 1024-entry block's consistent f64 prefix, and the batch's
// importance weights.
#pragma once
#include "common.h"

namespace {

constexpr int PB = 1024;      // slots per block (one wave, 16 per lane)

MZ_DEV float prio_q(float td, float eps, float alpha) {
  const float p = td + eps;
  return alpha == 1.f ? p : (float)pow((double)p, (double)alpha);
}

// lane's 16 priorities of block b (0 past cap), 16-byte loads where the 16 are all inside
MZ_DEV void load16(const float* __restrict__ q, int cap, int b, int lane, float* v) {
  const int i0 = b * PB + lane * 16;
  if (i0 + 16 <= cap) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float4 x = reinterpret_cast<const float4*>(q + i0)[c];
      v[4 * c] = x.x; v[4 * c + 1] = x.y; v[4 * c + 2] = x.z; v[4 * c + 3] = x.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) v[k] = i0 + k < cap ? q[i0 + k] : 0.f;
  }
}

MZ_DEV double shfl_f64(double x, int src) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  const int lo = __shfl((int)(uint32_t)u, src, 64), hi = __shfl((int)(uint32_t)(u >> 32), src, 64);
  return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}

// s[k] = the lane's running sums; returns off_lane (the sum, lane by lane in order, of the totals of the lanes
// before this one) and in `full` off_64, both the same sequence of additions on every lane
MZ_DEV double block_prefix(const float* v, int lane, double* s, double& full) {
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { run = run + (double)v[k]; s[k] = run; }
  double off = 0.0, all = 0.0;
  for (int i = 0; i < 64; ++i) {
    const double t = shfl_f64(run, i);
    all = all + t;
    if (i < lane) off = all;
  }
  full = all;
  return off;
}

// weight_j = raw_j / max raw (max is exact in any order)
__global__ __launch_bounds__(256) void prio_weight_kernel(const double* __restrict__ raw, int n,
                                                          float* __restrict__ weight) {
  __shared__ double red[256];
  double m = 0.0;
  for (int j = threadIdx.x; j < n; j += 256) m = fmax(m, raw[j]);
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  m = red[0];
  for (int j = threadIdx.x; j < n; j += 256) weight[j] = m > 0.0 ? (float)(raw[j] / m) : 0.f;
}

inline long long align16(long long x) { return (x + 15) & ~15LL; }

}  // namespace
