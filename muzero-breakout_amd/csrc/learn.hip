// Learner kernels: one minibatch of RLSystem._training_stage
// (train_torch.py:380-407) = _k_step_rollout forward with train-mode BatchNorm, loss_fn, the
// backward pass and the Adam step, on NHWC activations (T = f32 for parity, bf16 for
// throughput; statistics, gradients and parameters are f32 throughout).
//
// The convolutions themselves run on conv_igemm_kernel (conv.hip): forward with the f32 master
// weights (or their bf16 cast), input gradients as a convolution of the output gradient with
// the flipped, transposed weights (conv_wt_kernel in pack.hip packs them every step, with every other
// weight pack); the conv weight gradient is wgrad.hip. This file holds the rest of what is specific to
// training: BatchNorm, pool, axpy, scale, Linear, loss, Adam and the input builders:
//   bn_stats_*        batch mean / biased variance per channel (chunk-wise mean + M2, combined
//                     with Chan's formula in double), running-stat update (networks.py BN layers
//                     in train mode, momentum 0.1, unbiased running variance);
//   bn_apply          y = x * (gamma * invstd) + (beta - mean * gamma * invstd) (+ residual) (ReLU);
//   bn_bwd_*          g = dy * [y > 0] (in place), dgamma / dbeta, dx = (g - (x - mean) k - mean_g)
//                     * gamma * invstd with k = sum(g (x - mean)) invstd^2 / N (torch's CPU order);
//   avgpool2_bwd, axpy  the 2x2 average pool's backward; y += x;
//   scale_fwd / bwd   MuZeroAgent._scale_state (networks.py:314-328) with the first min / max
//                     index in NCHW flatten order (torch.min/max(dim) semantics) for the backward;
//   linear_*          the heads' nn.Linear on an NHWC image (weights kept in [o][pixel][channel]);
//   loss              supports_representation (utils.py:30-64) + log_softmax + KL(batchmean)
//                     for reward / value / policy and their logit gradients (loss_fn :33-66);
//   adam              torch.optim.Adam(lr, weight_decay = 1e-4) single-tensor update (networks.py:268);
//   learner_input / dyn_input  the representation and dynamics nets' input images from the replay ring's fields.
#include "common.h"

namespace {

// ------------------------------------------------------------------ BatchNorm statistics
// 4 consecutive channels per thread (C % 4 == 0): f32 float4 / bf16 8-byte loads.
template <typename T> struct Vec4;
template <> struct Vec4<float> {
  static MZ_DEV float4 load(const float* p) { return *reinterpret_cast<const float4*>(p); }
  static MZ_DEV void store(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
};
template <> struct Vec4<bf16_t> {
  static MZ_DEV float4 load(const bf16_t* p) {
    const uint2 u = *reinterpret_cast<const uint2*>(p);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
  }
  static MZ_DEV void store(bf16_t* p, float4 v) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
  }
};
MZ_DEV float4 f4add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// part[chunk][c] = (chunk mean, chunk M2) over rows [chunk*rpc, min(M, (chunk+1)*rpc)).
// 256 threads = (channel quads of a 64-channel group = 16) x 16 row lanes.
constexpr int BN_RPC = 64;
constexpr int BN_FK = 8;  // chunks per lane the BN finalisers load ahead (nchunk <= 512 in one round trip)
template <typename T>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const T* __restrict__ x, int M, int C, int rpc,
                                                               float2* __restrict__ part) {
  __shared__ float4 red[16][16];
  const int tq = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int c = blockIdx.x * 64 + tq * 4;
  const int r0 = blockIdx.y * rpc, r1 = min(M, r0 + rpc);
  const int n = r1 - r0;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < C)
    for (int r = r0 + ty; r < r1; r += 16) s = f4add(s, Vec4<T>::load(x + (size_t)r * C + c));
  red[ty][tq] = s;
  __syncthreads();
  float4 t = red[0][tq];
  for (int k = 1; k < 16; ++k) t = f4add(t, red[k][tq]);
  const float4 mean = make_float4(t.x / n, t.y / n, t.z / n, t.w / n);
  __syncthreads();
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < C)
    for (int r = r0 + ty; r < r1; r += 16) {
      const float4 v = Vec4<T>::load(x + (size_t)r * C + c);
      const float4 d = make_float4(v.x - mean.x, v.y - mean.y, v.z - mean.z, v.w - mean.w);
      q = make_float4(q.x + d.x * d.x, q.y + d.y * d.y, q.z + d.z * d.z, q.w + d.w * d.w);
    }
  red[ty][tq] = q;
  __syncthreads();
  if (ty == 0 && c < C) {
    float4 m2 = red[0][tq];
    for (int k = 1; k < 16; ++k) m2 = f4add(m2, red[k][tq]);
    float2* o = part + (size_t)blockIdx.y * C + c;
    o[0] = make_float2(mean.x, m2.x);
    o[1] = make_float2(mean.y, m2.y);
    o[2] = make_float2(mean.z, m2.z);
    o[3] = make_float2(mean.w, m2.w);
  }
}

// combine the chunks (Chan et al., in double) -> mean, invstd, alpha = gamma*invstd,
// beta' = beta - mean*alpha; running stats: r = momentum*stat + (1 - momentum)*r (unbiased var).
// One wave per channel: lane l folds chunks l, l+64, ...; then a fixed butterfly over the lanes.
MZ_DEV void chan_combine(double& n, double& mean, double& m2, double nb, double mb, double m2b) {
  if (nb == 0) return;
  const double tot = n + nb, d = mb - mean;
  mean += d * nb / tot;
  m2 += m2b + d * d * n * nb / tot;
  n = tot;
}

__global__ __launch_bounds__(64) void bn_stats_final_kernel(const float2* __restrict__ part, int nchunk, int rpc, int M,
                                                            int C, float eps, float momentum,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ stats,
                                                            float* __restrict__ run_mean, float* __restrict__ run_var) {
  const int c = blockIdx.x, lane = threadIdx.x;
  // the per-channel operands of the tail, loaded with the partials (after the butterfly each was one more
  // memory round trip on the chain)
  const float g_c = gamma[c], b_c = beta[c];
  const float rm_c = run_mean ? run_mean[c] : 0.f, rv_c = run_mean ? run_var[c] : 0.f;
  double n = 0, mean = 0, m2 = 0;
  // the lane's chunks l, l + 64, ... (up to BN_FK of them) are all loaded before the first fold: a rolled
  // load-then-fold loop waited one memory round trip per chunk. The folds keep their order (the same sums)
  float2 pv[BN_FK];
#pragma unroll
  for (int i = 0; i < BN_FK; ++i) pv[i] = lane + 64 * i < nchunk ? part[(size_t)(lane + 64 * i) * C + c] : float2{};
#pragma unroll
  for (int i = 0; i < BN_FK; ++i) {
    const int k = lane + 64 * i;
    if (k < nchunk) chan_combine(n, mean, m2, (double)min(rpc, M - k * rpc), (double)pv[i].x, (double)pv[i].y);
  }
  for (int k = lane + 64 * BN_FK; k < nchunk; k += 64) {
    const float2 p = part[(size_t)k * C + c];
    chan_combine(n, mean, m2, (double)min(rpc, M - k * rpc), (double)p.x, (double)p.y);
  }
  for (int o = 1; o < 64; o <<= 1) {
    const double n2 = __shfl_xor(n, o), mean2 = __shfl_xor(mean, o), m22 = __shfl_xor(m2, o);
    chan_combine(n, mean, m2, n2, mean2, m22);
  }
  if (lane) return;
  const float var = (float)(m2 / M);
  const float invstd = (float)(1.0 / sqrt((double)var + (double)eps));
  const float alpha = invstd * g_c;
  const float fm = (float)mean;
  stats[c] = fm;                 // mean
  stats[C + c] = invstd;         // invstd
  stats[2 * C + c] = alpha;      // gamma * invstd
  stats[3 * C + c] = b_c - fm * alpha;
  if (run_mean) {
    run_mean[c] = (float)((double)momentum * mean + (1.0 - (double)momentum) * (double)rm_c);
    const double unbiased = M > 1 ? m2 / (double)(M - 1) : m2;
    run_var[c] = (float)((double)momentum * unbiased + (1.0 - (double)momentum) * (double)rv_c);
  }
}

// y = x*alpha + beta' (+ res) (ReLU); 4 channels per thread (C % 4 == 0)
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const T* __restrict__ x, const float* __restrict__ stats,
                                                       const T* res, int relu, T* out, int M, int C) {
  const size_t n4 = (size_t)M * C / 4;
  const float* alpha = stats + 2 * C;
  const float* beta = stats + 3 * C;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * 4;
    const int c = (int)(e % C);
    const float4 v = Vec4<T>::load(x + e);
    const float4 a = *reinterpret_cast<const float4*>(alpha + c), b = *reinterpret_cast<const float4*>(beta + c);
    float4 y = make_float4(v.x * a.x + b.x, v.y * a.y + b.y, v.z * a.z + b.z, v.w * a.w + b.w);
    if (res) y = f4add(y, Vec4<T>::load(res + e));
    if (relu) y = make_float4(fmaxf(y.x, 0.f), fmaxf(y.y, 0.f), fmaxf(y.z, 0.f), fmaxf(y.w, 0.f));
    Vec4<T>::store(out + e, y);
  }
}

// ------------------------------------------------------------------ BatchNorm backward
// g = dy * [y > 0] (written back to dy when y != null); part[chunk][c] = (sum g, sum g (x - mean))
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(T* __restrict__ dy, const T* __restrict__ y,
                                                             const T* __restrict__ x, const float* __restrict__ stats,
                                                             int M, int C, int rpc, float2* __restrict__ part) {
  __shared__ float4 red[2][16][16];
  const int tq = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int c = blockIdx.x * 64 + tq * 4;
  const int r0 = blockIdx.y * rpc, r1 = min(M, r0 + rpc);
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sd = sg;
  if (c < C) {
    const float4 mean = *reinterpret_cast<const float4*>(stats + c);
    for (int r = r0 + ty; r < r1; r += 16) {
      const size_t i = (size_t)r * C + c;
      float4 g = Vec4<T>::load(dy + i);
      if (y) {
        const float4 yv = Vec4<T>::load(y + i);
        if (!(yv.x > 0.f)) g.x = 0.f;
        if (!(yv.y > 0.f)) g.y = 0.f;
        if (!(yv.z > 0.f)) g.z = 0.f;
        if (!(yv.w > 0.f)) g.w = 0.f;
        Vec4<T>::store(dy + i, g);
      }
      const float4 xv = Vec4<T>::load(x + i);
      sg = f4add(sg, g);
      sd = make_float4(sd.x + g.x * (xv.x - mean.x), sd.y + g.y * (xv.y - mean.y), sd.z + g.z * (xv.z - mean.z),
                       sd.w + g.w * (xv.w - mean.w));
    }
  }
  red[0][ty][tq] = sg;
  red[1][ty][tq] = sd;
  __syncthreads();
  if (ty == 0 && c < C) {
    float4 a = red[0][0][tq], b = red[1][0][tq];
    for (int k = 1; k < 16; ++k) { a = f4add(a, red[0][k][tq]); b = f4add(b, red[1][k][tq]); }
    float2* o = part + (size_t)blockIdx.y * C + c;
    o[0] = make_float2(a.x, b.x);
    o[1] = make_float2(a.y, b.y);
    o[2] = make_float2(a.z, b.z);
    o[3] = make_float2(a.w, b.w);
  }
}

// dgamma += dot*invstd, dbeta += sum g; coef = (mean_g, k = dot*invstd^2/N, gamma*invstd).
// One wave per channel, double sums, fixed butterfly order.
__global__ __launch_bounds__(64) void bn_bwd_final_kernel(const float2* __restrict__ part, int nchunk, int M, int C,
                                                          const float* __restrict__ stats, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta, float* __restrict__ coef) {
  const int c = blockIdx.x, lane = threadIdx.x;
  // the tail's per-channel operands, loaded with the partials (as bn_stats_final_kernel)
  const float invstd = stats[C + c], alpha = stats[2 * C + c], dg_c = dgamma[c], db_c = dbeta[c];
  double sg = 0, dot = 0;
  float2 pv[BN_FK];  // loaded before the first add, as bn_stats_final_kernel (the same sums)
#pragma unroll
  for (int i = 0; i < BN_FK; ++i) pv[i] = lane + 64 * i < nchunk ? part[(size_t)(lane + 64 * i) * C + c] : float2{};
#pragma unroll
  for (int i = 0; i < BN_FK; ++i)
    if (lane + 64 * i < nchunk) {
      sg += pv[i].x;
      dot += pv[i].y;
    }
  for (int k = lane + 64 * BN_FK; k < nchunk; k += 64) {
    const float2 p = part[(size_t)k * C + c];
    sg += p.x;
    dot += p.y;
  }
  for (int o = 1; o < 64; o <<= 1) {
    sg += __shfl_xor(sg, o);
    dot += __shfl_xor(dot, o);
  }
  if (lane) return;
  dgamma[c] = dg_c + (float)dot * invstd;
  dbeta[c] = db_c + (float)sg;
  coef[c] = (float)(sg / M);
  coef[C + c] = (float)dot * invstd * invstd / (float)M;
  coef[2 * C + c] = alpha;
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const T* __restrict__ g, const T* __restrict__ x,
                                                           const float* __restrict__ stats,
                                                           const float* __restrict__ coef, T* __restrict__ dx, int M,
                                                           int C) {
  const size_t n4 = (size_t)M * C / 4;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const size_t e = i * 4;
    const int c = (int)(e % C);
    const float4 gv = Vec4<T>::load(g + e), xv = Vec4<T>::load(x + e);
    const float4 mu = *reinterpret_cast<const float4*>(stats + c);
    const float4 mg = *reinterpret_cast<const float4*>(coef + c);
    const float4 k = *reinterpret_cast<const float4*>(coef + C + c);
    const float4 s = *reinterpret_cast<const float4*>(coef + 2 * C + c);
    Vec4<T>::store(dx + e, make_float4(((gv.x - (xv.x - mu.x) * k.x) - mg.x) * s.x, ((gv.y - (xv.y - mu.y) * k.y) - mg.y) * s.y,
                                       ((gv.z - (xv.z - mu.z) * k.z) - mg.z) * s.z, ((gv.w - (xv.w - mu.w) * k.w) - mg.w) * s.w));
  }
}

// ------------------------------------------------------------------ avg-pool backward, axpy
template <typename T>
__global__ void avgpool2_bwd_kernel(const T* __restrict__ dy, T* __restrict__ dx, int B, int H, int W, int C) {
  const size_t n = (size_t)B * H * W * C;
  const int Ho = H / 2, Wo = W / 2;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    size_t q = i / C;
    const int xx = (int)(q % W); q /= W;
    const int yy = (int)(q % H);
    const size_t b = q / H;
    st(dx + i, ld(dy + ((b * Ho + yy / 2) * Wo + xx / 2) * C + c) / 4.0f);
  }
}

// the same element values, 4 channels per thread (C % 4 == 0) with 32-bit index arithmetic (n < 2^31): the
// per-element 64-bit divisions above held the kernel at a fifth of the HBM rate
template <typename T>
__global__ void avgpool2_bwd4_kernel(const T* __restrict__ dy, T* __restrict__ dx, int B, int H, int W, int C) {
  const int C4 = C / 4, Ho = H / 2, Wo = W / 2;
  const unsigned n4 = (unsigned)B * H * W * C4;
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
    const unsigned c4 = i % C4;
    unsigned q = i / C4;
    const unsigned xx = q % W;
    q /= W;
    const unsigned yy = q % H, b = q / H;
    const float4 v = Vec4<T>::load(dy + ((size_t)(b * Ho + yy / 2) * Wo + xx / 2) * C + 4 * c4);
    Vec4<T>::store(dx + (size_t)i * 4, make_float4(v.x / 4.0f, v.y / 4.0f, v.z / 4.0f, v.w / 4.0f));
  }
}

template <typename T>
__global__ void axpy_kernel(T* __restrict__ y, const T* __restrict__ x, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    st(y + i, ld(y + i) + ld(x + i));
}

// ------------------------------------------------------------------ min-max scale
// one workgroup per env over n = HW*C values (NHWC); the first min / max in NCHW order
// (index c*HW + p) is recorded for the backward. mm[b] = (min, max), idx[b] = NHWC indices.
template <typename T>
__global__ __launch_bounds__(256) void scale_fwd_kernel(const T* __restrict__ h, T* __restrict__ out,
                                                        float2* __restrict__ mm, int2* __restrict__ idx, int HW,
                                                        int C) {
  const int b = blockIdx.x, n = HW * C;
  const T* x = h + (size_t)b * n;
  float mn = INFINITY, mx = -INFINITY;
  int kmn = 0x7fffffff, kmx = 0x7fffffff;  // NCHW keys
  for (int i = threadIdx.x; i < n; i += 256) {
    const float v = ld(x + i);
    const int c = i % C, key = c * HW + i / C;
    if (v < mn || (v == mn && key < kmn)) { mn = v; kmn = key; }
    if (v > mx || (v == mx && key < kmx)) { mx = v; kmx = key; }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(mn, o), x2 = __shfl_xor(mx, o);
    const int k2 = __shfl_xor(kmn, o), kx2 = __shfl_xor(kmx, o);
    if (m2 < mn || (m2 == mn && k2 < kmn)) { mn = m2; kmn = k2; }
    if (x2 > mx || (x2 == mx && kx2 < kmx)) { mx = x2; kmx = kx2; }
  }
  __shared__ float smn[4], smx[4];
  __shared__ int skn[4], skx[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { smn[w] = mn; smx[w] = mx; skn[w] = kmn; skx[w] = kmx; }
  __syncthreads();
  mn = smn[0]; mx = smx[0]; kmn = skn[0]; kmx = skx[0];
  for (int k = 1; k < 4; ++k) {
    if (smn[k] < mn || (smn[k] == mn && skn[k] < kmn)) { mn = smn[k]; kmn = skn[k]; }
    if (smx[k] > mx || (smx[k] == mx && skx[k] < kmx)) { mx = smx[k]; kmx = skx[k]; }
  }
  const float den = (mx - mn) + 1e-8f;
  T* o = out + (size_t)b * n;
  for (int i = threadIdx.x; i < n; i += 256) st(o + i, (ld(x + i) - mn) / den);
  if (threadIdx.x == 0) {
    mm[b] = make_float2(mn, mx);
    idx[b] = make_int2((kmn % HW) * C + kmn / HW, (kmx % HW) * C + kmx / HW);
  }
}

// dh (=|+=) dy/den, then dh[argmin] += -sum(dy)/den - d_den, dh[argmax] += d_den with
// d_den = -sum(dy * (h - min)) / den^2 (autograd of (h - min) / (max - min + 1e-8))
template <typename T>
__global__ __launch_bounds__(256) void scale_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ h,
                                                        const float2* __restrict__ mm, const int2* __restrict__ idx,
                                                        T* dh, int n, int accumulate) {
  const int b = blockIdx.x;
  const float mn = mm[b].x, mx = mm[b].y;
  const float den = (mx - mn) + 1e-8f;
  const T* g = dy + (size_t)b * n;
  const T* x = h + (size_t)b * n;
  T* o = dh + (size_t)b * n;
  float s1 = 0.f, s2 = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float gv = ld(g + i);
    const float d = gv / den;
    s1 += d;
    s2 += gv * (ld(x + i) - mn);
    st(o + i, accumulate ? ld(o + i) + d : d);
  }
  for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off); s2 += __shfl_xor(s2, off); }
  __shared__ float r1[4], r2[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { r1[w] = s1; r2[w] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float S1 = (r1[0] + r1[1]) + (r1[2] + r1[3]);
    const float S2 = (r2[0] + r2[1]) + (r2[2] + r2[3]);
    const float dden = -(S2 / den) / den;
    const int2 k = idx[b];
    st(o + k.x, ld(o + k.x) + (-S1 - dden));
    st(o + k.y, ld(o + k.y) + dden);
  }
}

// ------------------------------------------------------------------ heads: nn.Linear on NHWC
// out[b][o] = bias[o] + sum_k w[o][k] x[b][k], k = p*C + c (weights kept in that order)
template <typename T>
__global__ __launch_bounds__(256) void linear_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ out,
                                                         int K, int O) {
  const int b = blockIdx.x;
  const T* xb = x + (size_t)b * K;
  float acc[16];
#pragma unroll
  for (int o = 0; o < 16; ++o) acc[o] = 0.f;
  for (int k = threadIdx.x; k < K; k += 256) {
    const float v = ld(xb + k);
    float wv[16];  // unconditional loads (rows >= O re-read row 0): a load under `if (o < O)` is
#pragma unroll     // waited for inside its branch, which serialised the 16 loads
    for (int o = 0; o < 16; ++o) wv[o] = w[(size_t)(o < O ? o : 0) * K + k];
#pragma unroll
    for (int o = 0; o < 16; ++o)
      if (o < O) acc[o] += v * wv[o];
  }
  __shared__ float red[4][16];
  const int w_ = threadIdx.x >> 6;
#pragma unroll
  for (int o = 0; o < 16; ++o) {
    float v = acc[o];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((threadIdx.x & 63) == 0) red[w_][o] = v;
  }
  __syncthreads();
  if (threadIdx.x < O) {
    const int o = threadIdx.x;
    out[(size_t)b * O + o] = ((red[0][o] + red[1][o]) + (red[2][o] + red[3][o])) + bias[o];
  }
}

// dx[b][k] (=|+=) sum_o dy[b][o] w[o][k]
template <typename T>
__global__ void linear_bwd_x_kernel(const float* __restrict__ dy, const float* __restrict__ w, T* dx, int B, int K,
                                    int O, int accumulate) {
  const size_t n = (size_t)B * K;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    const size_t b = i / K;
    float s = 0.f;
    for (int o = 0; o < O; ++o) s += dy[b * O + o] * w[(size_t)o * K + k];
    st(dx + i, accumulate ? ld(dx + i) + s : s);
  }
}

// part[split][o][k] = sum_{b in split} dy[b][o] x[b][k]; bpart[split][o] = sum dy[b][o]
template <typename T>
__global__ void linear_bwd_w_kernel(const float* __restrict__ dy, const T* __restrict__ x, int B, int K, int O,
                                    int rows_per_split, float* __restrict__ part, float* __restrict__ bpart) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int split = blockIdx.y;
  const int b0 = split * rows_per_split, b1 = min(B, b0 + rows_per_split);
  float acc[16];
#pragma unroll
  for (int o = 0; o < 16; ++o) acc[o] = 0.f;
  if (k < K)
    for (int b = b0; b < b1; ++b) {
      const float v = ld(x + (size_t)b * K + k);
#pragma unroll
      for (int o = 0; o < 16; ++o)
        if (o < O) acc[o] += dy[(size_t)b * O + o] * v;
    }
  if (k < K)
    for (int o = 0; o < O; ++o) part[((size_t)split * O + o) * K + k] = acc[o];
  if (blockIdx.x == 0 && threadIdx.x < O) {
    float s = 0.f;
    for (int b = b0; b < b1; ++b) s += dy[(size_t)b * O + threadIdx.x];
    bpart[(size_t)split * O + threadIdx.x] = s;
  }
}

// ------------------------------------------------------------------ loss (loss_fn, train_torch.py:33-66)
// One workgroup. Row r = (b, k) of the (B, K) targets; logits[k][b][n]. Per row: compact
// transform + two-hot over the integer supports (utils.py:30-64), log_softmax, KL terms
// t*(log t - logp) (0 where t == 0), and the logit gradient (softmax*sum(t) - t)/(B*K)/K.
// loss[0..3] = total, reward, value, policy.
constexpr int LOSS_T = 256;

MZ_DEV void two_hot(float x, float smin, float smax, int ns, float* t) {
  const float sg = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);
  const float c = sg * ((sqrtf(fabsf(x) + 1.f) - 1.f) + 0.001f * x);
  const float step = (smax - smin) / (float)(ns - 1);
  int lo = -1;  // searchsorted(right=True) - 1
  for (int i = 0; i < ns; ++i)
    if (smin + (float)i * step <= c) lo = i;
  lo = lo < 0 ? 0 : (lo > ns - 2 ? ns - 2 : lo);
  const float sl = smin + (float)lo * step, su = smin + (float)(lo + 1) * step;
  const float pl = (su - c) / ((su - sl) + 1e-10f);
  for (int i = 0; i < ns; ++i) t[i] = 0.f;
  t[lo] = pl;
  t[lo + 1] = 1.f - pl;
}

MZ_DEV double kl_row(const float* z, const float* t, int n, float scale, float* dz) {
  float m = z[0];
  for (int i = 1; i < n; ++i) m = fmaxf(m, z[i]);
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += expf(z[i] - m);
  const float ls = logf(s);
  float tsum = 0.f;
  double kl = 0.0;
  for (int i = 0; i < n; ++i) {
    const float lp = (z[i] - m) - ls;  // torch log_softmax: (x - max) - log(sum exp(x - max))
    if (t[i] > 0.f) kl += (double)(t[i] * (logf(t[i]) - lp));
    tsum += t[i];
  }
  for (int i = 0; i < n; ++i) dz[i] = (expf((z[i] - m) - ls) * tsum - t[i]) * scale;
  return kl;
}

__global__ __launch_bounds__(LOSS_T) void loss_kernel(const float* __restrict__ lr, const float* __restrict__ lv,
                                                      const float* __restrict__ lp, const float* __restrict__ rewards,
                                                      const float* __restrict__ targets,
                                                      const float* __restrict__ counts, const int32_t* slots, int B,
                                                      int K, int ns, int na, float smin, float smax,
                                                      float* __restrict__ dlr, float* __restrict__ dlv,
                                                      float* __restrict__ dlp, float* __restrict__ loss) {
  __shared__ double red[3][LOSS_T];
  const float scale = (1.f / (float)K) / (float)(B * K);
  double acc[3] = {0.0, 0.0, 0.0};
  for (int r = threadIdx.x; r < B * K; r += LOSS_T) {
    const int b = r / K, k = r - b * K;
    const size_t src = slots ? (size_t)slots[b] : (size_t)b;  // ring row of window b
    float t[16], z[16], dz[16];
    const size_t o1 = ((size_t)k * B + b) * ns, o3 = ((size_t)k * B + b) * na;
    two_hot(rewards[src * K + k], smin, smax, ns, t);
    for (int i = 0; i < ns; ++i) z[i] = lr[o1 + i];
    acc[0] += kl_row(z, t, ns, scale, dz);
    for (int i = 0; i < ns; ++i) dlr[o1 + i] = dz[i];
    two_hot(targets[src * K + k], smin, smax, ns, t);
    for (int i = 0; i < ns; ++i) z[i] = lv[o1 + i];
    acc[1] += kl_row(z, t, ns, scale, dz);
    for (int i = 0; i < ns; ++i) dlv[o1 + i] = dz[i];
    float cs = 0.f;
    for (int i = 0; i < na; ++i) cs += counts[(src * K + k) * na + i];
    for (int i = 0; i < na; ++i) { t[i] = counts[(src * K + k) * na + i] / cs; z[i] = lp[o3 + i]; }
    acc[2] += kl_row(z, t, na, scale, dz);
    for (int i = 0; i < na; ++i) dlp[o3 + i] = dz[i];
  }
  for (int j = 0; j < 3; ++j) red[j][threadIdx.x] = acc[j];
  __syncthreads();
  for (int s = LOSS_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int j = 0; j < 3; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float rl = (float)(red[0][0] / (B * K)), vl = (float)(red[1][0] / (B * K)), pl = (float)(red[2][0] / (B * K));
    loss[0] = (1.f / (float)K) * ((rl + vl) + pl);
    loss[1] = rl; loss[2] = vl; loss[3] = pl;
  }
}

// loss_kernel over many workgroups (round 5: the one-workgroup form took 159 us of the minibatch's critical path):
// a thread per row r computes its three KL terms (gradients written as loss_kernel) and stores them to
// ws[j][r]; loss_reduce_kernel then folds them exactly as loss_kernel's threads did — thread t adds rows t,
// t + LOSS_T, ... in order into its double accumulators, then the same tree — so the loss is bit-identical
//
// PRIO (mzba_learner_loss_w, prioritized replay): row (b, k)'s three KL terms and its three gradient rows are
// multiplied by weights[b] (NULL: by nothing) before the fold — by 1.0f that is exact, so all-ones weights give
// the unweighted bits — and the k = 0 row leaves td[b] = |decode_support(logit_v[0][b]) - targets[slot][0]| (NULL:
// not written), the window's new priority (Ape-X: from the learner's own value prediction).
template <bool PRIO>
__global__ __launch_bounds__(256) void loss_rows_kernel(const float* __restrict__ lr, const float* __restrict__ lv,
                                                        const float* __restrict__ lp, const float* __restrict__ rewards,
                                                        const float* __restrict__ targets,
                                                        const float* __restrict__ counts, const int32_t* slots, int B,
                                                        int K, int ns, int na, float smin, float smax,
                                                        float* __restrict__ dlr, float* __restrict__ dlv,
                                                        float* __restrict__ dlp, double* __restrict__ ws,
                                                        const float* __restrict__ weights, float* __restrict__ td) {
  const float scale = (1.f / (float)K) / (float)(B * K);
  const int r = blockIdx.x * blockDim.x + threadIdx.x, BK = B * K;
  if (r >= BK) return;
  const int b = r / K, k = r - b * K;
  const size_t src = slots ? (size_t)slots[b] : (size_t)b;
  float t[16], z[16], dz[16];
  const size_t o1 = ((size_t)k * B + b) * ns, o3 = ((size_t)k * B + b) * na;
  const bool wt = PRIO && weights;
  const float w = wt ? weights[b] : 1.f;
  two_hot(rewards[src * K + k], smin, smax, ns, t);
  for (int i = 0; i < ns; ++i) z[i] = lr[o1 + i];
  double kl = kl_row(z, t, ns, scale, dz);
  ws[r] = wt ? kl * (double)w : kl;
  for (int i = 0; i < ns; ++i) dlr[o1 + i] = wt ? dz[i] * w : dz[i];
  two_hot(targets[src * K + k], smin, smax, ns, t);
  for (int i = 0; i < ns; ++i) z[i] = lv[o1 + i];
  if (PRIO && td && k == 0) td[b] = fabsf(decode_support(z, ns, smin, smax) - targets[src * K]);
  kl = kl_row(z, t, ns, scale, dz);
  ws[BK + r] = wt ? kl * (double)w : kl;
  for (int i = 0; i < ns; ++i) dlv[o1 + i] = wt ? dz[i] * w : dz[i];
  float cs = 0.f;
  for (int i = 0; i < na; ++i) cs += counts[(src * K + k) * na + i];
  for (int i = 0; i < na; ++i) { t[i] = counts[(src * K + k) * na + i] / cs; z[i] = lp[o3 + i]; }
  kl = kl_row(z, t, na, scale, dz);
  ws[2 * BK + r] = wt ? kl * (double)w : kl;
  for (int i = 0; i < na; ++i) dlp[o3 + i] = wt ? dz[i] * w : dz[i];
}

__global__ __launch_bounds__(LOSS_T) void loss_reduce_kernel(const double* __restrict__ ws, int B, int K,
                                                             float* __restrict__ loss) {
  __shared__ double red[3][LOSS_T];
  const int BK = B * K;
  for (int j = 0; j < 3; ++j) {
    double acc = 0.0;
    int r = threadIdx.x;
    for (; r + 3 * LOSS_T < BK; r += 4 * LOSS_T) {  // four rows' loads ahead of their adds, added in row order
      const double v0 = ws[j * BK + r], v1 = ws[j * BK + r + LOSS_T], v2 = ws[j * BK + r + 2 * LOSS_T],
                   v3 = ws[j * BK + r + 3 * LOSS_T];
      acc += v0;
      acc += v1;
      acc += v2;
      acc += v3;
    }
    for (; r < BK; r += LOSS_T) acc += ws[j * BK + r];
    red[j][threadIdx.x] = acc;
  }
  __syncthreads();
  for (int s = LOSS_T / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int j = 0; j < 3; ++j) red[j][threadIdx.x] += red[j][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float rl = (float)(red[0][0] / (B * K)), vl = (float)(red[1][0] / (B * K)), pl = (float)(red[2][0] / (B * K));
    loss[0] = (1.f / (float)K) * ((rl + vl) + pl);
    loss[1] = rl; loss[2] = vl; loss[3] = pl;
  }
}

// ------------------------------------------------------------------ Adam (networks.py:268)
// g = grad + wd*p; m += (1-b1)(g - m); v = v*b2 + (1-b2)*g*g; p += (-step_size*m) / (sqrt(v)/bc2s + eps)
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ grad, float* __restrict__ m,
                            float* __restrict__ v, size_t n, float neg_step, float one_m_b1, float b2, float one_m_b2,
                            float bc2s, float eps, float wd) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float pv = p[i];
    const float g = grad[i] + wd * pv;
    const float mv = m[i] + one_m_b1 * (g - m[i]);
    const float vv = v[i] * b2 + (one_m_b2 * g) * g;
    m[i] = mv;
    v[i] = vv;
    p[i] = pv + (neg_step * mv) / (sqrtf(vv) / bc2s + eps);
  }
}

// the same with the step-dependent scalars read from device memory (sc = {neg_step, 1-b1, b2, 1-b2,
// bc2s, eps, wd}): a captured minibatch graph replays with the host refreshing sc per step
__global__ void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ grad, float* __restrict__ m,
                                float* __restrict__ v, size_t n, const float* __restrict__ sc) {
  const float neg_step = sc[0], one_m_b1 = sc[1], b2 = sc[2], one_m_b2 = sc[3], bc2s = sc[4], eps = sc[5], wd = sc[6];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float pv = p[i];
    const float g = grad[i] + wd * pv;
    const float mv = m[i] + one_m_b1 * (g - m[i]);
    const float vv = v[i] * b2 + (one_m_b2 * g) * g;
    m[i] = mv;
    v[i] = vv;
    p[i] = pv + (neg_step * mv) / (sqrtf(vv) / bc2s + eps);
  }
}

// adam_kernel's / adam_dev_kernel's update, 4 parameters per thread (n % 4 == 0, 16-B aligned arrays: one 16-B access
// per array instead of four 4-B ones); DEV: the scalars from device memory (sc), else from the arguments
template <bool DEV>
__global__ void adam4_kernel(float4* __restrict__ p, const float4* __restrict__ grad, float4* __restrict__ m,
                             float4* __restrict__ v, size_t n4, const float* __restrict__ sc, float a_neg_step,
                             float a_one_m_b1, float a_b2, float a_one_m_b2, float a_bc2s, float a_eps, float a_wd) {
  const float neg_step = DEV ? sc[0] : a_neg_step, one_m_b1 = DEV ? sc[1] : a_one_m_b1, b2 = DEV ? sc[2] : a_b2;
  const float one_m_b2 = DEV ? sc[3] : a_one_m_b2, bc2s = DEV ? sc[4] : a_bc2s, eps = DEV ? sc[5] : a_eps;
  const float wd = DEV ? sc[6] : a_wd;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 p4 = p[i], g4 = grad[i], m4 = m[i], v4 = v[i];
    float po[4], mo[4], vo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float pv = (&p4.x)[k];
      const float g = (&g4.x)[k] + wd * pv;
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

// ------------------------------------------------------------------ learner inputs
// rep input [B][HW][Cp]: channel c < L = lut[frame code], L <= c < 2L = a/3 (train_torch.py:279-293,
// 437-470), zero beyond 2L. states u8 ring [cap][L][HW], past_actions i64 ring [cap][L].
template <typename T>
__global__ void learner_input_kernel(const uint8_t* __restrict__ states, const int64_t* __restrict__ past,
                                     const int32_t* __restrict__ slots, const float* __restrict__ lut, T* __restrict__ out,
                                     int B, int L, int HW, int Cp) {
  const size_t n = (size_t)B * HW * Cp;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cp);
    const size_t q = i / Cp;
    const int p = (int)(q % HW);
    const size_t b = q / HW, s = (size_t)slots[b];
    float v = 0.f;
    if (c < L) v = lut[states[(s * L + c) * HW + p] & 7];
    else if (c < 2 * L) v = (float)past[s * L + (c - L)] / 3.0f;
    st(out + i, v);
  }
}

// dynamics input [B][HW][Cp] = [h (C channels), one-hot(a) (3), 0...] (train_torch.py:295-311)
template <typename T>
__global__ void dyn_input_kernel(const T* __restrict__ h, const int64_t* __restrict__ fut,
                                 const int32_t* __restrict__ slots, int K, int k, T* __restrict__ out, int B, int HW,
                                 int C, int A, int Cp) {
  const size_t n = (size_t)B * HW * Cp;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % Cp);
    const size_t q = i / Cp;  // b*HW + p
    const size_t b = q / HW;
    float v = 0.f;
    if (c < C) v = ld(h + q * C + c);
    else if (c < C + A) v = (fut[(size_t)slots[b] * K + k] == (int64_t)(c - C)) ? 1.f : 0.f;
    st(out + i, v);
  }
}

}  // namespace

extern "C" {

int mzba_bn_stats(int dtype, const void* x, int M, int C, float eps, float momentum, const float* gamma,
                  const float* beta, float* stats, float* run_mean, float* run_var, void* ws, long long ws_bytes,
                  hipStream_t stream) {
  MZ_CHECK_ARG(x && stats && gamma && beta && ws && M > 0 && C > 0 && C % 4 == 0 && !run_mean == !run_var, -1);
  const int rpc = BN_RPC;
  const int nchunk = (M + rpc - 1) / rpc;
  MZ_CHECK_ARG((long long)nchunk * C * (long long)sizeof(float2) <= ws_bytes, -2);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(bn_stats_partial_kernel<T>, dim3((C + 63) / 64, nchunk), dim3(256), 0, stream, (const T*)x, M,
                       C, rpc, (float2*)ws);
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3(C), dim3(64), 0, stream, (const float2*)ws, nchunk,
                       rpc, M, C, eps, momentum, gamma, beta, stats, run_mean, run_var);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_bn_stats_final(const float* part, int nchunk, int rpc, int M, int C, float eps, float momentum,
                        const float* gamma, const float* beta, float* stats, float* run_mean, float* run_var,
                        hipStream_t stream) {
  MZ_CHECK_ARG(part && stats && gamma && beta && nchunk > 0 && rpc > 0 && M > 0 && C > 0 &&
               (long long)nchunk * rpc >= M && (long long)(nchunk - 1) * rpc < M && !run_mean == !run_var, -1);
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3(C), dim3(64), 0, stream, (const float2*)part, nchunk, rpc, M, C, eps,
                     momentum, gamma, beta, stats, run_mean, run_var);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_bn_backward_final(int dtype, const void* g, const void* x, const float* stats, const float* part, int nchunk,
                           int M, int C, float* dgamma, float* dbeta, void* dx, void* ws, long long ws_bytes,
                           hipStream_t stream) {
  MZ_CHECK_ARG(g && x && stats && part && dgamma && dbeta && dx && ws && nchunk > 0 && M > 0 && C > 0 && C % 4 == 0,
               -1);
  MZ_CHECK_ARG(3LL * C * 4 <= ws_bytes, -2);
  float* coef = (float*)ws;
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(C), dim3(64), 0, stream, (const float2*)part, nchunk, M, C, stats,
                       dgamma, dbeta, coef);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(grid_for((size_t)M * C / 4)), dim3(256), 0, stream, (const T*)g,
                       (const T*)x, stats, (const float*)coef, (T*)dx, M, C);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_bn_backward_apply(int dtype, const void* g, const void* x, const float* stats, const float* coef, void* dx,
                           int M, int C, hipStream_t stream) {
  MZ_CHECK_ARG(g && x && stats && coef && dx && M > 0 && C > 0 && C % 4 == 0, -1);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(grid_for((size_t)M * C / 4)), dim3(256), 0, stream, (const T*)g,
                       (const T*)x, stats, coef, (T*)dx, M, C);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_bn_backward_coef(const float* part, int nchunk, int M, int C, const float* stats, float* dgamma, float* dbeta,
                          float* coef, hipStream_t stream) {
  MZ_CHECK_ARG(part && stats && dgamma && dbeta && coef && nchunk > 0 && M > 0 && C > 0, -1);
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(C), dim3(64), 0, stream, (const float2*)part, nchunk, M, C, stats,
                     dgamma, dbeta, coef);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_bn_apply(int dtype, const void* x, const float* stats, const void* res, int relu, void* out, int M, int C,
                  hipStream_t stream) {
  MZ_CHECK_ARG(x && stats && out && M > 0 && C > 0 && C % 4 == 0, -1);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(bn_apply_kernel<T>, dim3(grid_for((size_t)M * C / 4)), dim3(256), 0, stream, (const T*)x, stats,
                       (const T*)res, relu, (T*)out, M, C);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_bn_backward(int dtype, void* dy, const void* y, const void* x, const float* stats, int M, int C,
                     float* dgamma, float* dbeta, void* dx, void* ws, long long ws_bytes, hipStream_t stream) {
  MZ_CHECK_ARG(dy && x && stats && dgamma && dbeta && dx && ws && M > 0 && C > 0 && C % 4 == 0, -1);
  const int rpc = BN_RPC;
  const int nchunk = (M + rpc - 1) / rpc;
  MZ_CHECK_ARG((long long)nchunk * C * (long long)sizeof(float2) + 3LL * C * 4 <= ws_bytes, -2);
  float2* part = (float2*)ws;
  float* coef = (float*)((char*)ws + (size_t)nchunk * C * sizeof(float2));
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(bn_bwd_partial_kernel<T>, dim3((C + 63) / 64, nchunk), dim3(256), 0, stream, (T*)dy,
                       (const T*)y, (const T*)x, stats, M, C, rpc, part);
    hipLaunchKernelGGL(bn_bwd_final_kernel, dim3(C), dim3(64), 0, stream, (const float2*)part, nchunk,
                       M, C, stats, dgamma, dbeta, coef);
    hipLaunchKernelGGL(bn_bwd_apply_kernel<T>, dim3(grid_for((size_t)M * C / 4)), dim3(256), 0, stream, (const T*)dy,
                       (const T*)x, stats, (const float*)coef, (T*)dx, M, C);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_avgpool2_backward(int dtype, const void* dy, void* dx, int B, int H, int W, int C, hipStream_t stream) {
  MZ_CHECK_ARG(dy && dx && B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0, -1);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    if (C % 4 == 0 && (long long)B * H * W * C < (1LL << 31))
      hipLaunchKernelGGL(avgpool2_bwd4_kernel<T>, dim3(grid_for((size_t)B * H * W * C / 4)), dim3(256), 0, stream,
                         (const T*)dy, (T*)dx, B, H, W, C);
    else
      hipLaunchKernelGGL(avgpool2_bwd_kernel<T>, dim3(grid_for((size_t)B * H * W * C)), dim3(256), 0, stream,
                         (const T*)dy, (T*)dx, B, H, W, C);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_axpy(int dtype, void* y, const void* x, long long n, hipStream_t stream) {
  MZ_CHECK_ARG(y && x && n >= 0, -1);
  if (n == 0) return 0;
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(axpy_kernel<T>, dim3(grid_for((size_t)n)), dim3(256), 0, stream, (T*)y, (const T*)x, (size_t)n);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_scale_forward(int dtype, const void* h, void* out, float* minmax, int32_t* argminmax, int B, int HW, int C,
                       hipStream_t stream) {
  MZ_CHECK_ARG(h && out && minmax && argminmax && B > 0 && HW > 0 && C > 0, -1);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(scale_fwd_kernel<T>, dim3(B), dim3(256), 0, stream, (const T*)h, (T*)out, (float2*)minmax,
                       (int2*)argminmax, HW, C);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_scale_backward(int dtype, const void* dy, const void* h, const float* minmax, const int32_t* argminmax,
                        void* dh, int B, int n, int accumulate, hipStream_t stream) {
  MZ_CHECK_ARG(dy && h && minmax && argminmax && dh && B > 0 && n > 0, -1);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(scale_bwd_kernel<T>, dim3(B), dim3(256), 0, stream, (const T*)dy, (const T*)h,
                       (const float2*)minmax, (const int2*)argminmax, (T*)dh, n, accumulate);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_linear_forward(int dtype, const void* x, const float* w, const float* bias, float* out, int B, int K, int O,
                        hipStream_t stream) {
  MZ_CHECK_ARG(x && w && bias && out && B > 0 && K > 0 && O > 0 && O <= 16, -1);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(linear_fwd_kernel<T>, dim3(B), dim3(256), 0, stream, (const T*)x, w, bias, out, K, O);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

long long mzba_linear_ws_bytes(int B, int K, int O) {
  const int nsplit = B >= 64 ? 16 : 1;
  return (long long)nsplit * ((long long)O * K + O) * 4;
}

int mzba_linear_backward(int dtype, const void* x, const float* w, const float* dy, void* dx, int accumulate,
                         float* dw, float* db, int B, int K, int O, void* ws, long long ws_bytes, hipStream_t stream) {
  MZ_CHECK_ARG(x && w && dy && dw && db && ws && B > 0 && K > 0 && O > 0 && O <= 16, -1);
  MZ_CHECK_ARG(mzba_linear_ws_bytes(B, K, O) <= ws_bytes, -2);
  const int nsplit = B >= 64 ? 16 : 1;
  const int rps = (B + nsplit - 1) / nsplit;
  float* part = (float*)ws;
  float* bpart = part + (size_t)nsplit * O * K;
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    if (dx)
      hipLaunchKernelGGL(linear_bwd_x_kernel<T>, dim3(grid_for((size_t)B * K)), dim3(256), 0, stream, dy, w, (T*)dx, B,
                         K, O, accumulate);
    hipLaunchKernelGGL(linear_bwd_w_kernel<T>, dim3((K + 255) / 256, nsplit), dim3(256), 0, stream, dy, (const T*)x,
                       B, K, O, rps, part, bpart);
    mz_sum_partials2(part, bpart, nsplit, (size_t)O * K, (size_t)O, dw, db, stream);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_learner_loss(const float* logit_r, const float* logit_v, const float* logit_p, const float* rewards,
                      const float* targets, const float* counts, const int32_t* slots, int B, int K, int ns, int na,
                      float smin, float smax, float* dlogit_r, float* dlogit_v, float* dlogit_p, float* loss,
                      hipStream_t stream) {
  MZ_CHECK_ARG(logit_r && logit_v && logit_p && rewards && targets && counts && dlogit_r && dlogit_v && dlogit_p &&
                   loss && B > 0 && K > 0 && ns >= 2 && ns <= 16 && na > 0 && na <= 16,
               -1);
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(LOSS_T), 0, stream, logit_r, logit_v, logit_p, rewards, targets, counts,
                     slots, B, K, ns, na, smin, smax, dlogit_r, dlogit_v, dlogit_p, loss);
  MZ_LAUNCH_CHECK();
  return 0;
}

long long mzba_learner_loss_ws_bytes(int B, int K) { return 3LL * B * K * (long long)sizeof(double); }

int mzba_learner_loss_ws(const float* logit_r, const float* logit_v, const float* logit_p, const float* rewards,
                         const float* targets, const float* counts, const int32_t* slots, int B, int K, int ns, int na,
                         float smin, float smax, float* dlogit_r, float* dlogit_v, float* dlogit_p, float* loss,
                         void* ws, long long ws_bytes, hipStream_t stream) {
  MZ_CHECK_ARG(logit_r && logit_v && logit_p && rewards && targets && counts && dlogit_r && dlogit_v && dlogit_p &&
                   loss && ws && B > 0 && K > 0 && ns >= 2 && ns <= 16 && na > 0 && na <= 16,
               -1);
  MZ_CHECK_ARG(mzba_learner_loss_ws_bytes(B, K) <= ws_bytes && (long long)B * K < (1LL << 28), -2);
  const int BK = B * K;
  hipLaunchKernelGGL(loss_rows_kernel<false>, dim3((BK + 255) / 256), dim3(256), 0, stream, logit_r, logit_v, logit_p,
                     rewards, targets, counts, slots, B, K, ns, na, smin, smax, dlogit_r, dlogit_v, dlogit_p, (double*)ws,
                     (const float*)nullptr, (float*)nullptr);
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(LOSS_T), 0, stream, (const double*)ws, B, K, loss);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_learner_loss_w(const float* logit_r, const float* logit_v, const float* logit_p, const float* rewards,
                        const float* targets, const float* counts, const int32_t* slots, int B, int K, int ns, int na,
                        float smin, float smax, float* dlogit_r, float* dlogit_v, float* dlogit_p, float* loss,
                        void* ws, long long ws_bytes, const float* weights, float* td, hipStream_t stream) {
  MZ_CHECK_ARG(logit_r && logit_v && logit_p && rewards && targets && counts && dlogit_r && dlogit_v && dlogit_p &&
                   loss && ws && B > 0 && K > 0 && ns >= 2 && ns <= 16 && na > 0 && na <= 16,
               -1);
  MZ_CHECK_ARG(mzba_learner_loss_ws_bytes(B, K) <= ws_bytes && (long long)B * K < (1LL << 28), -2);
  const int BK = B * K;
  hipLaunchKernelGGL(loss_rows_kernel<true>, dim3((BK + 255) / 256), dim3(256), 0, stream, logit_r, logit_v, logit_p,
                     rewards, targets, counts, slots, B, K, ns, na, smin, smax, dlogit_r, dlogit_v, dlogit_p, (double*)ws,
                     weights, td);
  hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), dim3(LOSS_T), 0, stream, (const double*)ws, B, K, loss);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_adam(float* p, const float* grad, float* m, float* v, long long n, float neg_step, float one_m_b1, float b2,
              float one_m_b2, float bc2_sqrt, float eps, float weight_decay, hipStream_t stream) {
  MZ_CHECK_ARG(p && grad && m && v && n >= 0, -1);
  if (n == 0) return 0;
  const bool a16 = (((uintptr_t)p | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  if (n % 4 == 0 && a16)
    hipLaunchKernelGGL(adam4_kernel<false>, dim3(grid_for((size_t)n / 4)), dim3(256), 0, stream, (float4*)p,
                       (const float4*)grad, (float4*)m, (float4*)v, (size_t)n / 4, nullptr, neg_step, one_m_b1, b2,
                       one_m_b2, bc2_sqrt, eps, weight_decay);
  else
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, stream, p, grad, m, v, (size_t)n, neg_step,
                       one_m_b1, b2, one_m_b2, bc2_sqrt, eps, weight_decay);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_adam_dev(float* p, const float* grad, float* m, float* v, long long n, const float* scalars,
                  hipStream_t stream) {
  MZ_CHECK_ARG(p && grad && m && v && scalars && n >= 0, -1);
  if (n == 0) return 0;
  const bool a16 = (((uintptr_t)p | (uintptr_t)grad | (uintptr_t)m | (uintptr_t)v) & 15) == 0;
  if (n % 4 == 0 && a16)
    hipLaunchKernelGGL(adam4_kernel<true>, dim3(grid_for((size_t)n / 4)), dim3(256), 0, stream, (float4*)p,
                       (const float4*)grad, (float4*)m, (float4*)v, (size_t)n / 4, scalars, 0.f, 0.f, 0.f, 0.f, 0.f,
                       0.f, 0.f);
  else
    hipLaunchKernelGGL(adam_dev_kernel, dim3(grid_for((size_t)n)), dim3(256), 0, stream, p, grad, m, v, (size_t)n,
                       scalars);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_learner_input(int dtype, const uint8_t* states, const int64_t* past_actions, const int32_t* slots,
                       const float* lut8, void* out, int B, int L, int HW, int Cp, hipStream_t stream) {
  MZ_CHECK_ARG(states && past_actions && slots && lut8 && out && B > 0 && L > 0 && HW > 0 && Cp >= 2 * L, -1);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(learner_input_kernel<T>, dim3(grid_for((size_t)B * HW * Cp)), dim3(256), 0, stream, states,
                       past_actions, slots, lut8, (T*)out, B, L, HW, Cp);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_dyn_input(int dtype, const void* h, const int64_t* future_actions, const int32_t* slots, int K, int k,
                   void* out, int B, int HW, int C, int A, int Cp, hipStream_t stream) {
  MZ_CHECK_ARG(h && future_actions && slots && out && B > 0 && HW > 0 && C > 0 && A >= 0 && k >= 0 && k < K &&
                   Cp >= C + A,
               -1);
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(dyn_input_kernel<T>, dim3(grid_for((size_t)B * HW * Cp)), dim3(256), 0, stream, (const T*)h,
                       future_actions, slots, K, k, (T*)out, B, HW, C, A, Cp);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

}  // extern "C"
