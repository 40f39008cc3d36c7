// Weight hand-off on the device: the acting nets' packs written straight from the learner's f32 master
// weights and BatchNorm running statistics, with the bits the host packer (mzba/agent.py:PackedNets) produces.
//
// The work is a job table in device memory (mzba/refresh.py builds it once per learner / pack pair): one job writes
// one destination tensor, or one slice of a concatenated one.
//   pack_fold_bn_kernel   per BatchNorm: alpha = gamma / sqrt(var + 1e-5), beta' = beta - mean alpha, in f64, once
//                         (as the host computes them once per BN), into a scratch buffer the pack launch reads;
//   pack_fold_kernel      a thread produces 8 consecutive destination elements (one 16-byte store for bf16 / fp16) of
//                         a weight job: in every layout they are 8 consecutive source channels of one (co, tap), two
//                         aligned 16-byte loads; or one element of a bias / action-table job. A workgroup finds its
//                         job by a search of the table's prefix array of first workgroups (as replay_write_kernel
//                         finds its env).
// Arithmetic: f64, one operation at a time (-ffp-contract=off, no fma), then f64 -> f32 -> bf16 / fp16, each round to
// nearest even: numpy's f64 fold followed by torch.tensor(x, dtype=float32).to(bfloat16).
#include "common.h"

namespace {

struct PfBn {
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* var;
  double* out;  // alpha[C], then beta'[C]
  int C, pad_;
};

enum { PF_PLAIN = 0, PF_LAT = 1, PF_LAT16 = 2, PF_BIAS = 3, PF_ACT = 4 };
enum { PF_F32 = 0, PF_BF16 = 1, PF_FP16 = 2 };

// weight jobs: w [cout][taps][cin_src] (f32), channels [c_first, c_first + c_used) -> the destination's channels
//   [0, c_used) of cin_dst (the rest zero); tperm: the destination's taps run (dx, dy) (3x3 only)
// PF_BIAS: w = the conv / Linear bias [cout]; PF_ACT: w = the dynamics ConvBlock's weight, c_first = its first action
//   channel, A actions, H x W latent, taps = ks * ks: act_bias[y W + x][a][co]
struct PfJob {
  const float* w;
  const double* ab;  // the BN's alpha[cout], beta'[cout], or null (no BatchNorm)
  void* dst;
  long long off;     // first destination element
  int kind, otype, cout, taps, cin_src, c_first, c_used, cin_dst, tperm, H, W, A;
};
static_assert(sizeof(PfJob) == 80 && sizeof(PfBn) == 48, "mzba/refresh.py writes these records");

__global__ __launch_bounds__(256) void pack_fold_bn_kernel(const PfBn* __restrict__ bns, const int32_t* __restrict__ first,
                                                           int nbn) {
  const int blk = blockIdx.x;
  int lo = 0, hi = nbn;  // last b with first[b] <= blk
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= blk) lo = mid; else hi = mid;
  }
  const PfBn b = bns[lo];
  const int c = (blk - first[lo]) * 256 + threadIdx.x;
  if (c >= b.C) return;
  const double alpha = __ddiv_rn((double)b.gamma[c], __dsqrt_rn((double)b.var[c] + 1e-5));
  const double m = (double)b.mean[c] * alpha;
  b.out[c] = alpha;
  b.out[b.C + c] = (double)b.beta[c] - m;
}

MZ_DEV uint16_t pf_half(float f) { return __builtin_bit_cast(uint16_t, (_Float16)f); }

__global__ __launch_bounds__(256) void pack_fold_kernel(const PfJob* __restrict__ jobs, const int32_t* __restrict__ first,
                                                        int njobs) {
  const int blk = blockIdx.x;
  int lo = 0, hi = njobs;  // last j with first[j] <= blk
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (first[mid] <= blk) lo = mid; else hi = mid;
  }
  const PfJob j = jobs[lo];
  const long long u = (long long)(blk - first[lo]) * 256 + threadIdx.x;

  if (j.kind == PF_BIAS) {
    if (u >= j.cout) return;
    double v = (double)j.w[u];
    if (j.ab) {
      v = v * j.ab[u];
      v = v + j.ab[j.cout + u];
    }
    ((float*)j.dst)[j.off + u] = (float)v;
    return;
  }
  if (j.kind == PF_ACT) {
    const long long n = (long long)j.H * j.W * j.A * j.cout;
    if (u >= n) return;
    const int co = (int)(u % j.cout), a = (int)(u / j.cout % j.A), p = (int)(u / ((long long)j.cout * j.A));
    const int y = p / j.W, x = p - y * j.W;
    int ks = 1;
    while (ks * ks < j.taps) ++ks;
    const int pad = ks / 2;
    const double alpha = j.ab ? j.ab[co] : 1.0;
    double s = 0.0;
    for (int ky = 0; ky < ks; ++ky)
      for (int kx = 0; kx < ks; ++kx) {
        const int sy = y + ky - pad, sx = x + kx - pad;
        if (sy < 0 || sy >= j.H || sx < 0 || sx >= j.W) continue;
        double t = (double)j.w[((size_t)co * j.taps + ky * ks + kx) * j.cin_src + j.c_first + a];
        if (j.ab) t = t * alpha;
        s = s + t;
      }
    ((float*)j.dst)[j.off + u] = (float)s;
    return;
  }

  // weight jobs: 8 destination elements = channels [ci, ci + 8) of (co, tap)
  const int Cd = j.cin_dst;
  const long long units = (long long)j.cout * j.taps * (Cd / 8);
  if (u >= units) return;
  int co, tap, ci;
  if (j.kind == PF_PLAIN) {  // [co][tap][Cd]
    const int g = Cd / 8;
    ci = (int)(u % g) * 8;
    const long long t = u / g;
    tap = (int)(t % j.taps);
    co = (int)(t / j.taps);
  } else if (j.kind == PF_LAT) {  // pack_lat: [ct][kh][tap][c][h][r][8], ci = kh Cd/2 + 16 c + 8 h, co = 32 ct + r
    const int nh = Cd / 32;
    const int r = (int)(u % 32), h = (int)(u / 32 % 2), c = (int)(u / 64 % nh);
    const long long t = u / (64 * nh);
    tap = (int)(t % j.taps);
    const int kh = (int)(t / j.taps % 2), ct = (int)(t / (2 * j.taps));
    co = ct * 32 + r;
    ci = kh * (Cd / 2) + c * 16 + h * 8;
  } else {  // pack_lat16: [ct][s][q][r][8], k = 32 s + 8 q = tap' Cd + ci, co = 16 ct + r
    const int ns = j.taps * Cd / 32;
    const int r = (int)(u % 16), q = (int)(u / 16 % 4), s = (int)(u / 64 % ns), ct = (int)(u / (64LL * ns));
    const int k = s * 32 + q * 8;
    const int tp = k / Cd;
    ci = k - tp * Cd;
    tap = j.tperm ? (tp % 3) * 3 + tp / 3 : tp;  // taps in (dx, dy) order
    co = ct * 16 + r;
  }
  float x[8];
  const float* src = j.w + ((size_t)co * j.taps + tap) * j.cin_src + j.c_first + ci;
  if (ci + 8 <= j.c_used) {
    const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = ci + i < j.c_used ? src[i] : 0.f;
  }
  float f[8];
  if (j.ab) {
    const double alpha = j.ab[co];
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = ci + i < j.c_used ? (float)((double)x[i] * alpha) : 0.f;  // padding stays +0
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = x[i];
  }
  const long long d = j.off + u * 8;
  if (j.otype == PF_F32) {
    float4* o = reinterpret_cast<float4*>((float*)j.dst + d);
    o[0] = float4{f[0], f[1], f[2], f[3]};
    o[1] = float4{f[4], f[5], f[6], f[7]};
  } else {
    uint32_t p[4];
    if (j.otype == PF_BF16) {
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) p[i] = (uint32_t)pf_half(f[2 * i]) | ((uint32_t)pf_half(f[2 * i + 1]) << 16);
    }
    *reinterpret_cast<uint4*>((uint16_t*)j.dst + d) = uint4{p[0], p[1], p[2], p[3]};
  }
}

}  // namespace

extern "C" {

int mzba_pack_fold_job_bytes(void) { return (int)sizeof(PfJob); }
int mzba_pack_fold_bn_bytes(void) { return (int)sizeof(PfBn); }

int mzba_pack_fold_bn(const void* bns, const int32_t* first, int nbn, int nblocks, hipStream_t stream) {
  MZ_CHECK_ARG(bns && first && nbn > 0 && nblocks >= nbn, -1);
  hipLaunchKernelGGL(pack_fold_bn_kernel, dim3(nblocks), dim3(256), 0, stream, (const PfBn*)bns, first, nbn);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_pack_fold(const void* jobs, const int32_t* first, int njobs, int nblocks, hipStream_t stream) {
  MZ_CHECK_ARG(jobs && first && njobs > 0 && nblocks >= njobs, -1);
  hipLaunchKernelGGL(pack_fold_kernel, dim3(nblocks), dim3(256), 0, stream, (const PfJob*)jobs, first, njobs);
  MZ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
