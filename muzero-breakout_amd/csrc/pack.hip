// Every device weight pack: the f32 master weights [Cout][taps][Cin] rewritten into the orders the conv kernels read.
//
// Two packed orders exist, each stated once here (pack_unit_lat / pack_unit_lat16) and once on the host
// (mzba/agent.py pack_lat / pack_lat16 / pack_tower_conv). Both hold a logical W'[n][tap][c] (n < N rows, c < Cc) in
// units of 8 consecutive c:
//   pack_lat   (conv_lat's 32-column fragments)   out[ct][kh][tap][cc][h][r][8] = W'[32 ct + r][tap][kh Cc/2 + 16 cc + 8 h ..]
//   pack_lat16 (tower / band / halo, 16 columns)  out[ct][s][q][r][8] = W'[16 ct + r] at k = 32 s + 8 q = tap' Cc + c;
//              with the tap permutation tap' runs (dx, dy): tap = (tap' % 3) * 3 + tap' / 3 (3x3 only)
// Three kernels write them; each keeps only its own source addressing, fold and store:
//   conv_wt_kernel          the learner's plain cast / flipped transpose (no packed order);
//   conv_pack_kernel        one pack per launch, per element, W' = w or its flipped transpose (mzba_conv_pack_bf16);
//   conv_pack_multi_kernel  the learner's per-minibatch packs, up to PK_MAX per launch, a unit per thread;
//   pack_fold_kernel        the weight hand-off (below): a job table, BatchNorm folded in f64.
#include "common.h"

namespace {

struct PackSrc {
  int n, tap, c;  // row, tap and first channel of W' behind one destination unit
};

// destination unit u of the pack_lat order
template <typename I>
MZ_DEV PackSrc pack_unit_lat(I u, int taps, int Cc) {
  const int r = (int)(u % 32); u /= 32;
  const int h = (int)(u % 2); u /= 2;
  const int cc = (int)(u % (Cc / 32)); u /= Cc / 32;
  const int tap = (int)(u % taps); u /= taps;
  const int kh = (int)(u % 2), ct = (int)(u / 2);
  return {32 * ct + r, tap, kh * (Cc / 2) + 16 * cc + 8 * h};
}

// destination unit u of the pack_lat16 order; tperm: taps in (dx, dy) order
template <typename I>
MZ_DEV PackSrc pack_unit_lat16(I u, int taps, int Cc, bool tperm) {
  const int r = (int)(u % 16); u /= 16;
  const int q = (int)(u % 4); u /= 4;
  const int ns = taps * Cc / 32;
  const int s = (int)(u % ns), ct = (int)(u / ns);
  const int k = 32 * s + 8 * q, tp = k / Cc;
  return {16 * ct + r, tperm ? (tp % 3) * 3 + tp / 3 : tp, k - tp * Cc};
}

// ------------------------------------------------------------------ the learner's packs
// wt[ci][tap][co] = w[co][taps-1-tap][ci] for ci < cin_used (input-gradient conv), or a plain
// cast wt = w (mode 0). w: f32 master [Cout][taps][Cin].
template <typename T>
__global__ void conv_wt_kernel(const float* __restrict__ w, T* __restrict__ wt, int Cout, int taps, int Cin,
                               int cin_used, int flip) {
  const size_t n = flip ? (size_t)cin_used * taps * Cout : (size_t)Cout * taps * Cin;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (!flip) {
      st(wt + i, w[i]);
    } else {
      const int co = (int)(i % Cout);
      const size_t q = i / Cout;
      const int tap = (int)(q % taps), ci = (int)(q / taps);
      st(wt + i, w[((size_t)co * taps + (taps - 1 - tap)) * Cin + ci]);
    }
  }
}

// bf16 weight packs for the latent / band conv kernels, straight from the f32 master weights:
// logical W'[n][tap][c] = flip ? w[c][taps-1-tap][n] : w[n][tap][c] (n < N rows, c < Cc).
// layout 1: the pack_lat order (conv_lat); layout 2: the pack_lat16 order with taps in (dx, dy) (tower / band, 3x3).
// `pad` zero elements follow (the kernels' weight-ring overrun).
__global__ void conv_pack_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int Cout, int taps, int Cin,
                                 int N, int Cc, int flip, int layout, size_t pad) {
  const size_t n_el = (size_t)N * taps * Cc;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_el + pad; i += (size_t)gridDim.x * blockDim.x) {
    if (i >= n_el) { out[i] = 0; continue; }
    const PackSrc u = layout == 1 ? pack_unit_lat(i / 8, taps, Cc) : pack_unit_lat16(i / 8, taps, Cc, true);
    const int n = u.n, tap = u.tap, c = u.c + (int)(i % 8);
    const float v = flip ? w[((size_t)c * taps + (taps - 1 - tap)) * Cin + n] : w[((size_t)n * taps + tap) * Cin + c];
    out[i] = f32_to_bf16(v);
  }
}

// Many packs in one launch (the learner's per-minibatch packs of every conv: one launch per PK_MAX of them instead of
// one each): blockIdx.y = job, a thread per 8 consecutive output elements (8 consecutive c of one (n, tap): Cc % 32
// == 0 and pad % 8 == 0), the same element values as conv_pack_kernel, one 16-B store.
struct PackJob {
  const float* w;
  bf16_t* out;
  int Cout, taps, Cin, N, Cc, flip, layout, pad;
};
constexpr int PK_MAX = 32;
struct PackJobs {
  PackJob j[PK_MAX];
};
__global__ __launch_bounds__(256) void conv_pack_multi_kernel(PackJobs js) {
  const PackJob& jb = js.j[blockIdx.y];
  const int taps = jb.taps, Cc = jb.Cc, Cin = jb.Cin;
  const int n_el = jb.N * taps * Cc, ng = (n_el + jb.pad) / 8;
  for (int g8 = blockIdx.x * blockDim.x + threadIdx.x; g8 < ng; g8 += gridDim.x * blockDim.x) {
    const int i = 8 * g8;
    uint4 o = make_uint4(0, 0, 0, 0);
    if (i < n_el) {
      const PackSrc u = jb.layout == 1 ? pack_unit_lat(g8, taps, Cc) : pack_unit_lat16(g8, taps, Cc, true);
      const int n = u.n, tap = u.tap, c = u.c;
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        v[j] = jb.flip ? jb.w[((size_t)(c + j) * taps + (taps - 1 - tap)) * Cin + n] : jb.w[((size_t)n * taps + tap) * Cin + c + j];
      o = make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7]));
    }
    *reinterpret_cast<uint4*>(jb.out + i) = o;
  }
}

// ------------------------------------------------------------------ weight hand-off
// The acting nets' packs written straight from the learner's f32 master weights and BatchNorm running statistics,
// with the bits the host packer (mzba/agent.py:PackedNets) produces.
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
  } else {
    const PackSrc p = j.kind == PF_LAT ? pack_unit_lat(u, j.taps, Cd) : pack_unit_lat16(u, j.taps, Cd, j.tperm != 0);
    co = p.n;
    tap = p.tap;
    ci = p.c;
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

int mzba_conv_wpack(int dtype, const float* w, void* wt, int Cout, int taps, int Cin, int cin_used, int flip,
                    hipStream_t stream) {
  MZ_CHECK_ARG(w && wt && Cout > 0 && taps > 0 && Cin > 0 && cin_used > 0 && cin_used <= Cin, -1);
  const size_t n = flip ? (size_t)cin_used * taps * Cout : (size_t)Cout * taps * Cin;
  return dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(conv_wt_kernel<T>, dim3(grid_for(n)), dim3(256), 0, stream, w, (T*)wt, Cout, taps, Cin,
                       cin_used, flip);
    MZ_LAUNCH_CHECK();
    return 0;
  });
}

int mzba_conv_pack_bf16(const float* w, void* out, int Cout, int taps, int Cin, int N, int Cc, int flip, int layout,
                        long long pad, hipStream_t stream) {
  MZ_CHECK_ARG(w && out && Cout > 0 && Cin > 0 && N > 0 && Cc > 0 && pad >= 0 && (layout == 1 || layout == 2), -1);
  MZ_CHECK_ARG(layout != 1 || (N % 32 == 0 && Cc % 32 == 0), -2);
  MZ_CHECK_ARG(layout != 2 || (taps == 9 && N % 16 == 0 && Cc % 32 == 0), -3);
  MZ_CHECK_ARG(flip ? (N <= Cin && Cc == Cout) : (N == Cout && Cc <= Cin), -4);
  const size_t n = (size_t)N * taps * Cc + (size_t)pad;
  hipLaunchKernelGGL(conv_pack_kernel, dim3(grid_for(n)), dim3(256), 0, stream, w, (bf16_t*)out, Cout, taps, Cin, N, Cc,
                     flip, layout, (size_t)pad);
  MZ_LAUNCH_CHECK();
  return 0;
}

// njobs packs, each the arguments of one mzba_conv_pack_bf16 call: w[j], out[j] (16-B aligned) and
// prm[8 j ..] = {Cout, taps, Cin, N, Cc, flip, layout, pad}; the same outputs as the njobs separate calls, in
// launches of PK_MAX jobs
int mzba_conv_pack_bf16_multi(const float* const* w, void* const* out, const int* prm, int njobs, hipStream_t stream) {
  MZ_CHECK_ARG(w && out && prm && njobs > 0, -1);
  for (int j0 = 0; j0 < njobs; j0 += PK_MAX) {
    PackJobs js{};
    const int nj = njobs - j0 < PK_MAX ? njobs - j0 : PK_MAX;
    for (int k = 0; k < nj; ++k) {
      const int* p = prm + 8 * (j0 + k);
      const int Cout = p[0], taps = p[1], Cin = p[2], N = p[3], Cc = p[4], flip = p[5], layout = p[6], pad = p[7];
      MZ_CHECK_ARG(w[j0 + k] && out[j0 + k] && ((uintptr_t)out[j0 + k] & 15) == 0 && Cout > 0 && Cin > 0 && N > 0 &&
                       Cc > 0 && pad >= 0 && pad % 8 == 0 && (layout == 1 || layout == 2), -1);
      MZ_CHECK_ARG(layout != 1 || (N % 32 == 0 && Cc % 32 == 0), -2);
      MZ_CHECK_ARG(layout != 2 || (taps == 9 && N % 16 == 0 && Cc % 32 == 0), -3);
      MZ_CHECK_ARG(flip ? (N <= Cin && Cc == Cout) : (N == Cout && Cc <= Cin), -4);
      MZ_CHECK_ARG((long long)N * taps * Cc + pad < (1LL << 31), -5);
      js.j[k] = PackJob{w[j0 + k], (bf16_t*)out[j0 + k], Cout, taps, Cin, N, Cc, flip, layout, pad};
    }
    hipLaunchKernelGGL(conv_pack_multi_kernel, dim3(64, nj), dim3(256), 0, stream, js);
    MZ_LAUNCH_CHECK();
  }
  return 0;
}

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
