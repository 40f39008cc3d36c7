// The learner's conv weight gradient: dW[co][tap][ci] = sum_m dY[m][co] X_tap[m][ci] (+ the conv bias gradient) on
// NHWC activations, split over m into deterministic partials that sum_partials2_kernel reduces into the
// gradient buffer in split order.
//   conv_wgrad_kernel / conv_wgrad_bf16_kernel  per-tap 64 x 64 tiles (f32 / bf16), one launch pair per segment;
//   conv_wgrad_img_kernel                       bf16 3x3 over whole zero-bordered images (form 0, A/B);
//   conv_wgrad_px_kernel                        bf16 3x3 over pixel rows (forms 1 - 3; 2 is the default);
//   wgrad_img_plan / wgrad_px_plan              the two whole-image kernels' shapes, splits and LDS;
//   wgrad_core                                  picks the kernel (mzba_conv_wgrad_set_variant / _set_form, thread-local).
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;

// ------------------------------------------------------------------ conv weight gradient
// One workgroup: a 64 (co) x 64 (ci) tile of one tap over a chunk of m rows, 4 waves as 2x2 of
// 32x32 (2x2 MFMA 16x16 tiles). K = m in steps of 16 rows staged through LDS.
// f32: v_mfma_f32_16x16x4_f32 (lane: row l&15, k = l>>4). bf16: rows are widened to f32 in LDS.
constexpr int WG_ROWS = 16, WG_LD = 80;  // LDS row stride (floats): 16-bank shift per k row

template <typename T>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, int B,
                                                         int H, int W, int Cin, int Cout, int ks, int rows_per_split,
                                                         float* __restrict__ part, float* __restrict__ bpart) {
  __shared__ float la[2][WG_ROWS][WG_LD];  // dY tile [m][co]
  __shared__ float lb[2][WG_ROWS][WG_LD];  // X tile  [m][ci]
  const int taps = ks * ks, pad = ks / 2;
  const int nci = (Cin + 63) / 64;
  int t = blockIdx.x;
  const int cit = t % nci; t /= nci;
  const int tap = t % taps; t /= taps;
  const int cot = t;
  const int split = blockIdx.y;
  const int HW = H * W, M = B * HW;
  const int m0 = split * rows_per_split, m1 = min(M, m0 + rows_per_split);
  const int ky = tap / ks - pad, kx = tap % ks - pad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  // staging: thread -> (row lr = tid >> 4, 4 channels at 4*(tid & 15))
  const int lr = tid >> 4, lc = (tid & 15) * 4;
  const int co_s = cot * 64 + lc, ci_s = cit * 64 + lc;
  float4 va, vb;
  auto load = [&](int mb) {
    const int m = mb + lr;
    va = make_float4(0.f, 0.f, 0.f, 0.f);
    vb = va;
    if (m < m1) {
      const int b = m / HW, p = m - b * HW, yy = p / W, xx = p - yy * W;
      const T* d = dy + (size_t)m * Cout + co_s;
      if (co_s < Cout) va = make_float4(ld(d), ld(d + 1), ld(d + 2), ld(d + 3));
      const int sy = yy + ky, sx = xx + kx;
      if (ci_s < Cin && sy >= 0 && sy < H && sx >= 0 && sx < W) {
        const T* s = x + ((size_t)b * HW + sy * W + sx) * Cin + ci_s;
        vb = make_float4(ld(s), ld(s + 1), ld(s + 2), ld(s + 3));
      }
    }
  };
  auto store = [&](int buf) {
    *reinterpret_cast<float4*>(&la[buf][lr][lc]) = va;
    *reinterpret_cast<float4*>(&lb[buf][lr][lc]) = vb;
  };
  const bool do_bias = bpart && tap == 0 && cit == 0;
  typedef __attribute__((ext_vector_type(4))) float f4;
  f4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};
  const int nsteps = (m1 - m0 + WG_ROWS - 1) / WG_ROWS;
  if (nsteps > 0) {
    load(m0);
    store(0);
  }
  __syncthreads();
  const int fr = lane & 15, fk = lane >> 4;
  float4 bacc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (do_bias) { bacc.x += va.x; bacc.y += va.y; bacc.z += va.z; bacc.w += va.w; }
    if (s + 1 < nsteps) load(m0 + (s + 1) * WG_ROWS);
#pragma unroll
    for (int kk = 0; kk < WG_ROWS / 4; ++kk) {
      const int r = kk * 4 + fk;
      float a[2], bb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = la[buf][r][wr * 32 + i * 16 + fr];
#pragma unroll
      for (int j = 0; j < 2; ++j) bb[j] = lb[buf][r][wc * 32 + j * 16 + fr];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], bb[j], acc[i][j], 0, 0, 0);
    }
    if (s + 1 < nsteps) store(buf ^ 1);
    __syncthreads();
  }
  // D[row = co 4*fk + r][col = ci fr] of each 16x16 tile
  const size_t K = (size_t)taps * Cin;
  float* outp = part + (size_t)split * Cout * K;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ci = cit * 64 + wc * 32 + j * 16 + fr;
      if (ci >= Cin) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = cot * 64 + wr * 32 + i * 16 + 4 * fk + r;
        if (co < Cout) outp[(size_t)co * K + (size_t)tap * Cin + ci] = acc[i][j][r];
      }
    }
  if (do_bias) {  // reduce the 16 row lanes of each channel group through LDS
    __shared__ float4 bred[16][16];
    bred[lr][tid & 15] = bacc;
    __syncthreads();
    if (tid < 16) {
      float4 s = bred[0][tid];
      for (int r = 1; r < 16; ++r) { s.x += bred[r][tid].x; s.y += bred[r][tid].y; s.z += bred[r][tid].z; s.w += bred[r][tid].w; }
      const int co = cot * 64 + tid * 4;
      float* bp = bpart + (size_t)split * Cout;
      if (co < Cout) { bp[co] = s.x; bp[co + 1] = s.y; bp[co + 2] = s.z; bp[co + 3] = s.w; }
    }
  }
}

// bf16: v_mfma_f32_16x16x32_bf16 with both operands read by ds_read_b64_tr_b16 from row-major
// [m][channel] LDS tiles (rows staged straight from HBM, 16-B chunks). A = dY^T (co x m), B = X_tap
// (m x ci). Lane group g (lanes 16g..16g+15) takes k rows {4g..4g+3} and {16+4g..16+4g+3} of each
// 32-row k step (the same permutation for A and B); a 160-B row stride makes each 32-lane half's
// eight rows hit disjoint banks.
constexpr int WB_M = 64, WB_LD = 80;  // rows per stage, bf16 per LDS row
typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s lds_v4s;

MZ_DEV bf16x8_t tr_frag(const bf16_t* base) {  // base: this lane's address for the first 4 rows
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(base));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(base + 16 * WB_LD));
  typedef short v8s __attribute__((ext_vector_type(8)));
  const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, r);  // bit pattern, not a numeric short -> bf16 conversion
}

__global__ __launch_bounds__(256) void conv_wgrad_bf16_kernel(const bf16_t* __restrict__ x,
                                                              const bf16_t* __restrict__ dy, int B, int H, int W,
                                                              int Cin, int Cout, int ks, int rows_per_split,
                                                              float* __restrict__ part, float* __restrict__ bpart) {
  __shared__ __attribute__((aligned(16))) bf16_t la[2][WB_M][WB_LD];
  __shared__ __attribute__((aligned(16))) bf16_t lb[2][WB_M][WB_LD];
  __shared__ float bred[32][64];
  const int taps = ks * ks, pad = ks / 2;
  const int nci = (Cin + 63) / 64;
  int t = blockIdx.x;
  const int cit = t % nci; t /= nci;
  const int tap = t % taps; t /= taps;
  const int cot = t;
  const int split = blockIdx.y;
  const int HW = H * W, M = B * HW;
  const int m0 = split * rows_per_split, m1 = min(M, m0 + rows_per_split);
  const int ky = tap / ks - pad, kx = tap % ks - pad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;
  // staging: chunk c = tid + 256u (u = 0, 1): row c >> 3, 8 channels at 8*(c & 7)
  const int ch = tid & 7;
  const int co_s = cot * 64 + ch * 8, ci_s = cit * 64 + ch * 8;
  uint4 va[2], vb[2];
  auto load = [&](int mb) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = mb + ((tid + 256 * u) >> 3);
      va[u] = make_uint4(0, 0, 0, 0);
      vb[u] = va[u];
      if (m < m1) {
        const int b = m / HW, p = m - b * HW, yy = p / W, xx = p - yy * W;
        if (co_s < Cout) va[u] = *reinterpret_cast<const uint4*>(dy + (size_t)m * Cout + co_s);
        const int sy = yy + ky, sx = xx + kx;
        if (ci_s < Cin && sy >= 0 && sy < H && sx >= 0 && sx < W)
          vb[u] = *reinterpret_cast<const uint4*>(x + ((size_t)b * HW + sy * W + sx) * Cin + ci_s);
      }
    }
  };
  const bool do_bias = bpart && tap == 0 && cit == 0;
  float bacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bacc[j] = 0.f;
  auto store = [&](int buf) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int r = (tid + 256 * u) >> 3;
      *reinterpret_cast<uint4*>(&la[buf][r][ch * 8]) = va[u];
      *reinterpret_cast<uint4*>(&lb[buf][r][ch * 8]) = vb[u];
      if (do_bias) {
        const bf16_t* e = reinterpret_cast<const bf16_t*>(&va[u]);
#pragma unroll
        for (int j = 0; j < 8; ++j) bacc[j] += bf16_to_f32(e[j]);
      }
    }
  };
  f32x4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int nsteps = (m1 - m0 + WB_M - 1) / WB_M;
  if (nsteps > 0) {
    load(m0);
    store(0);
  }
  __syncthreads();
  // transposed-read lane address: group g = lane >> 4 takes rows 4g + q, q = (lane & 15) >> 2,
  // columns 4p.. (p = lane & 3) of its 16-column block
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  for (int s = 0; s < nsteps; ++s) {
    const int buf = s & 1;
    if (s + 1 < nsteps) load(m0 + (s + 1) * WB_M);
#pragma unroll
    for (int kk = 0; kk < WB_M / 32; ++kk) {
      const int row = kk * 32 + 4 * g + q;
      bf16x8_t a[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = tr_frag(&la[buf][row][wr * 32 + i * 16 + 4 * pp]);
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[j] = tr_frag(&lb[buf][row][wc * 32 + j * 16 + 4 * pp]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (s + 1 < nsteps) store(buf ^ 1);
    __syncthreads();
  }
  const size_t K = (size_t)taps * Cin;
  float* outp = part + (size_t)split * Cout * K;
  const int fr = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ci = cit * 64 + wc * 32 + j * 16 + fr;
      if (ci >= Cin) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int co = cot * 64 + wr * 32 + i * 16 + 4 * fk + r;
        if (co < Cout) outp[(size_t)co * K + (size_t)tap * Cin + ci] = acc[i][j][r];
      }
    }
  if (do_bias) {  // 32 row lanes per channel group -> column sums
#pragma unroll
    for (int j = 0; j < 8; ++j) bred[tid >> 3][ch * 8 + j] = bacc[j];
    __syncthreads();
    if (tid < 64) {
      float sum = 0.f;
      for (int r = 0; r < 32; ++r) sum += bred[r][tid];
      const int co = cot * 64 + tid;
      if (co < Cout) bpart[(size_t)split * Cout + co] = sum;
    }
  }
}

// bf16 3x3 weight gradient over whole images: one workgroup = a 64 (co) x 64 (ci) tile for ALL 9
// taps, over E envs per LDS stage. Each env's image is staged once with a zero border (Hp = H + 2,
// Wp = W + 2 rows of 64 channels); the contraction index k runs over the H x Wp interior-row
// positions (border columns carry dY = 0), so tap (dy, dx) is the constant row offset
// dy * Wp + dx into the bordered X image: every 4-row transposed-read block stays contiguous and
// dY / X are read from HBM once per tile instead of once per tap.
constexpr int WI_LD = 80;        // bf16 per LDS row (160 B, the transposed-read bank layout above)
constexpr int WI_LEAD = 8;       // zero rows before the X images (tap offsets reach -Wp - 1)
constexpr int WI_PF = 24;        // staging chunks per 256 threads (KS + XR <= 768 rows)

// up to WG_MAXSEG (x, dY) segments of Bseg envs each form one contraction (env b = seg * Bseg + b'):
// the K unrolled uses of one latent conv reduce in a single launch (learner._flush_wgrad)
constexpr int WG_MAXSEG = 8;
struct WgImg {
  int B, H, W, Cin, Cout, E, KS, XR, stages_per_split;
  int Bseg;
  const bf16_t* xs[WG_MAXSEG];
  const bf16_t* dys[WG_MAXSEG];
};

MZ_DEV bf16x8_t tr_frag_at(const bf16_t* lo_base, const bf16_t* hi_base) {
  const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(lo_base));
  const v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(hi_base));
  typedef short v8s __attribute__((ext_vector_type(8)));
  const v8s r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, r);
}

// 8 waves: waves 4 tg .. 4 tg + 3 own taps [5 tg, min(9, 5 tg + 5)) of the tile (two waves per
// SIMD to hide the LDS read latency; the tap groups write disjoint partials, so no reduction)
constexpr int WI_NT = 512;
constexpr int WI_PFN = WI_PF * 256 / WI_NT;  // staging chunks per thread
constexpr size_t WI_LDS_MAX = 140 * 1024;     // dynamic LDS (+ 16 KB static bias scratch <= 160 KB)
template <bool PF>
__global__ __launch_bounds__(WI_NT) void conv_wgrad_img_kernel(WgImg a, float* __restrict__ part,
                                                               float* __restrict__ bpart) {
  extern __shared__ __attribute__((aligned(16))) bf16_t lds_img[];
  bf16_t* ldy = lds_img;                                   // [KS][WI_LD]
  bf16_t* lx = lds_img + (size_t)(a.KS + WI_LEAD) * WI_LD;  // [XR + 64][WI_LD], preceded by WI_LEAD zero rows
  __shared__ float bred[WI_NT / 8][64];
  const int H = a.H, W = a.W, Wp = W + 2, Hp = H + 2, HWp = H * Wp, HpWp = Hp * Wp;
  const int nci = (a.Cin + 63) / 64;
  const int cit = blockIdx.x % nci, cot = blockIdx.x / nci;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tg = wave >> 2, wr = (wave >> 1) & 1, wc = wave & 1;
  const int tap0 = 5 * tg, ntap = tg ? 4 : 5;
  const int ch = tid & 7;  // 16-B chunk (8 channels) every staging chunk of this thread holds
  const int co_s = cot * 64 + ch * 8, ci_s = cit * 64 + ch * 8;
  const bool do_bias = bpart && cit == 0;
  float bacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bacc[j] = 0.f;
  // zero the lead rows and the tail margin of the X region once
  for (int i = tid; i < WI_LEAD * 8; i += WI_NT)
    *reinterpret_cast<uint4*>(lds_img + (size_t)(a.KS + i / 8) * WI_LD + (i & 7) * 8) = make_uint4(0, 0, 0, 0);
  for (int i = tid; i < 64 * 8; i += WI_NT)
    *reinterpret_cast<uint4*>(lx + (size_t)(a.XR + i / 8) * WI_LD + (i & 7) * 8) = make_uint4(0, 0, 0, 0);
  f32x4_t acc[5][2][2];
#pragma unroll
  for (int t = 0; t < 5; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int nst_total = (a.B + a.E - 1) / a.E;
  const int st0 = blockIdx.y * a.stages_per_split, st1 = min(nst_total, st0 + a.stages_per_split);
  // stage staging through registers. PF: the next stage's HBM loads are in flight during this
  // stage's MFMAs (WI_PF chunks of 16 B per thread cover KS + XR rows x 8 chunks); otherwise the
  // stage is loaded in batches of WI_PF chunks after the previous one is consumed.
  // A stage = E consecutive envs of one segment (the planner makes E divide Bseg), so a chunk's
  // source is the stage's env-0 base + an offset that is the same for every stage: the per-chunk
  // index math (divisions by the bordered geometry) runs once per thread, not once per stage.
  const int nchunk = (a.KS + a.XR) * 8;
  const size_t img_x = (size_t)H * W * a.Cin, img_dy = (size_t)H * W * a.Cout;
  int soff[WI_PFN];     // element offset from the stage's env-0 base, -1 = zero chunk
  uint32_t sdy = 0u;    // bit u: chunk u is a dY chunk
  for (int u = 0; u < WI_PFN; ++u) {
    int off = -1;
    const int i = u * WI_NT + tid;
    if (i < a.KS * 8) {  // dY rows: k = e*HWp + y*Wp + xp (xp in 1..W real, 0 / W+1 border)
      const int r = i >> 3;
      const int e = r / HWp, w = r - e * HWp, y = w / Wp, xp = w - y * Wp;
      if (e < a.E && xp >= 1 && xp <= W && co_s < a.Cout) off = (int)(e * img_dy + (size_t)(y * W + xp - 1) * a.Cout + co_s);
      sdy |= 1u << u;
    } else if (i < nchunk) {  // X rows: bordered images, row e*HpWp + yp*Wp + xp
      const int r = (i >> 3) - a.KS;
      const int e = r / HpWp, rem = r - e * HpWp, yp = rem / Wp, xp = rem - yp * Wp;
      if (yp >= 1 && yp <= H && xp >= 1 && xp <= W && ci_s < a.Cin)
        off = (int)(e * img_x + (size_t)((yp - 1) * W + xp - 1) * a.Cin + ci_s);
    }
    soff[u] = off;
  }
  uint4 pf[WI_PFN];
  auto load_chunks = [&](int st, int base) {
    const int b0 = st * a.E, sg = b0 / a.Bseg, bl = b0 - sg * a.Bseg;
    const bf16_t* xb = a.xs[sg] + (size_t)bl * img_x;
    const bf16_t* db = a.dys[sg] + (size_t)bl * img_dy;
    if (base == 0) {
      // unconditional loads (zero chunks read the stage base, then select): a load under a
      // branch is waited for inside the branch, which serialised the 12 loads of a stage
#pragma unroll
      for (int u = 0; u < WI_PFN; ++u)
        pf[u] = *reinterpret_cast<const uint4*>(((sdy >> u) & 1u ? db : xb) + (soff[u] >= 0 ? soff[u] : 0));
#pragma unroll
      for (int u = 0; u < WI_PFN; ++u)
        if (soff[u] < 0) pf[u] = make_uint4(0, 0, 0, 0);
      return;
    }
#pragma unroll
    for (int u = 0; u < WI_PFN; ++u) {  // batched (non-PF) plans: chunks beyond the first batch
      const int i = base + u * WI_NT + tid;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (i < a.KS * 8) {
        const int r = i >> 3;
        const int e = r / HWp, w = r - e * HWp, y = w / Wp, xp = w - y * Wp;
        if (e < a.E && xp >= 1 && xp <= W && co_s < a.Cout)
          v = *reinterpret_cast<const uint4*>(db + e * img_dy + (size_t)(y * W + xp - 1) * a.Cout + co_s);
      } else if (i < nchunk) {
        const int r = (i >> 3) - a.KS;
        const int e = r / HpWp, rem = r - e * HpWp, yp = rem / Wp, xp = rem - yp * Wp;
        if (yp >= 1 && yp <= H && xp >= 1 && xp <= W && ci_s < a.Cin)
          v = *reinterpret_cast<const uint4*>(xb + e * img_x + (size_t)((yp - 1) * W + xp - 1) * a.Cin + ci_s);
      }
      pf[u] = v;
    }
  };
  auto store_chunks = [&](int base) {
#pragma unroll
    for (int u = 0; u < WI_PFN; ++u) {
      const int i = base + u * WI_NT + tid;
      if (i < a.KS * 8) {
        *reinterpret_cast<uint4*>(ldy + (size_t)(i >> 3) * WI_LD + ch * 8) = pf[u];
        if (do_bias) {
          const bf16_t* h = reinterpret_cast<const bf16_t*>(&pf[u]);
#pragma unroll
          for (int j = 0; j < 8; ++j) bacc[j] += bf16_to_f32(h[j]);
        }
      } else if (i < nchunk) {
        *reinterpret_cast<uint4*>(lx + (size_t)((i >> 3) - a.KS) * WI_LD + ch * 8) = pf[u];
      }
    }
  };
  if (PF && st0 < st1) load_chunks(st0, 0);
  for (int st = st0; st < st1; ++st) {
    __syncthreads();  // previous stage fully consumed
    if (PF) {
      store_chunks(0);
    } else {
      for (int base = 0; base < nchunk; base += WI_PFN * WI_NT) {
        load_chunks(st, base);
        store_chunks(base);
      }
    }
    __syncthreads();
    if (PF && st + 1 < st1) load_chunks(st + 1, 0);
    for (int ks = 0; ks < a.KS / 32; ++ks) {
      // this lane's transposed-read rows for the two 4-row blocks of k step ks
      const int r0 = ks * 32 + 4 * g + q, r1 = r0 + 16;
      const int e0 = min(r0 / HWp, a.E - 1), e1 = min(r1 / HWp, a.E - 1);
      const int x0 = e0 * HpWp + Wp + (r0 - e0 * HWp), x1 = e1 * HpWp + Wp + (r1 - e1 * HWp);
      bf16x8_t af[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int c = wr * 32 + i * 16 + 4 * pp;
        af[i] = tr_frag_at(ldy + (size_t)r0 * WI_LD + c, ldy + (size_t)r1 * WI_LD + c);
      }
      // B fragments one tap ahead: tap t + 1's transposed reads are in flight during tap t's MFMAs
      auto bload = [&](int t, bf16x8_t (&b)[2]) {
        const int off = (t / 3 - 1) * Wp + (t % 3 - 1);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int c = wc * 32 + j * 16 + 4 * pp;
          b[j] = tr_frag_at(lx + (ptrdiff_t)(x0 + off) * WI_LD + c, lx + (ptrdiff_t)(x1 + off) * WI_LD + c);
        }
      };
      bf16x8_t bcur[2], bnxt[2];
      bload(tap0, bcur);
#pragma unroll
      for (int tt = 0; tt < 5; ++tt) {
        if (tt < ntap) {  // wave-uniform: tap group 1 has 4 taps
          if (tt + 1 < ntap) bload(tap0 + tt + 1, bnxt);
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[tt][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bcur[j], acc[tt][i][j], 0, 0, 0);
          if (tt + 1 < ntap) { bcur[0] = bnxt[0]; bcur[1] = bnxt[1]; }
        }
      }
    }
  }
  const size_t K = (size_t)9 * a.Cin;
  float* outp = part + (size_t)blockIdx.y * a.Cout * K;
  const int fr = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int tt = 0; tt < 5; ++tt)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int t = tap0 + tt;
        const int ci = cit * 64 + wc * 32 + j * 16 + fr;
        if (tt >= ntap) continue;
        if (ci >= a.Cin) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = cot * 64 + wr * 32 + i * 16 + 4 * fk + r;
          if (co < a.Cout) outp[(size_t)co * K + (size_t)t * a.Cin + ci] = acc[tt][i][j][r];
        }
      }
  if (do_bias) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) bred[tid >> 3][ch * 8 + j] = bacc[j];
    __syncthreads();
    if (tid < 64) {
      float sum = 0.f;
      for (int r = 0; r < WI_NT / 8; ++r) sum += bred[r][tid];
      const int co = cot * 64 + tid;
      if (co < a.Cout) bpart[(size_t)blockIdx.y * a.Cout + co] = sum;
    }
  }
}

// geometry of the image-stage weight gradient (E envs per stage within the LDS budget)
struct WgPlan {
  WgImg a;
  int nsplit;
  size_t lds;
  bool pf;  // the whole stage fits the register prefetch
};
// B = all envs (nseg * Bseg); a stage's E envs never straddle a segment (E divides Bseg)
static bool wgrad_img_plan(int B, int Bseg, int H, int W, int Cin, int Cout, WgPlan& p) {
  const int Wp = W + 2, HWp = H * Wp, HpWp = (H + 2) * Wp;
  if (HWp % 4 || Bseg <= 0 || B % Bseg) return false;
  int E = 1;
  auto rows = [&](int e) { return ((e * HWp + 31) / 32 * 32) + WI_LEAD + e * HpWp + 64; };
  auto staged = [&](int e) { return (e * HWp + 31) / 32 * 32 + e * HpWp; };
  while (E < 16 && Bseg % (E * 2) == 0 && (size_t)rows(E * 2) * WI_LD * 2 <= WI_LDS_MAX && staged(E * 2) * 8 <= WI_PF * 256) E *= 2;
  if ((size_t)rows(E) * WI_LD * 2 > WI_LDS_MAX) return false;
  p.pf = staged(E) * 8 <= WI_PF * 256;
  const int tiles = ((Cout + 63) / 64) * ((Cin + 63) / 64);
  const int stages = (B + E - 1) / E;
  // one workgroup per CU (two per CU measured slower: the extra split partials cost more)
  int nsplit = (256 + tiles - 1) / tiles;
  if (nsplit > stages) nsplit = stages;
  const int sps = (stages + nsplit - 1) / nsplit;
  nsplit = (stages + sps - 1) / sps;
  p.a = WgImg{B, H, W, Cin, Cout, E, (E * HWp + 31) / 32 * 32, E * HpWp, sps, Bseg, {}, {}};
  p.nsplit = nsplit;
  p.lds = (size_t)rows(E) * WI_LD * 2;
  return true;
}

// bf16 3x3 weight gradient over pixel rows (round 6): the whole-image kernel's tiling (64 co x 64 ci,
// all 9 taps, 8 waves) without the zero border. The contraction index k runs over the E * HW real
// pixels of a stage — row e * HW + p of dY and of X, which is how E consecutive envs already lie in
// HBM — padded to a multiple of 32 with zero dY rows. Tap (dy, dx) of k row r is X row r + dy * W + dx,
// or the zero row XR where the tap leaves the image: each lane hands its own row address to the
// transposed read, with the 9-tap validity of its two k rows from a per-workgroup mask table (the same
// for every stage). Against the bordered kernel: 20 instead of 28 k per 4x5 image (the border columns'
// MFMAs and staging rows are gone), twice the envs per stage (10 k steps between barriers instead of 7),
// no per-step divisions, and an XCD-aware workgroup order (the 16 tiles of one env range share an L2).
struct WgPx {
  int B, H, W, Cin, Cout, E, KS, XR, stages_per_split, Bseg, tiles, remap;
  const bf16_t* xs[WG_MAXSEG];
  const bf16_t* dys[WG_MAXSEG];
};

// WF (the waves' share of the 64 x 64 x 9 tile; 2 = WF 1 with its k steps software-pipelined): 0 = 32 co x
// 32 ci x 5 / 4 taps per wave (2 A + 10 B fragment
// reads per 20 MFMAs); 1 = 64 co x 32 ci x 3 / 2 taps per wave (taps {0,1,2}, {3,4}, {5,6}, {7,8}; 4 A + 6 / 4 B
// reads per 24 / 16 MFMAs: 29 % fewer LDS fragment reads per stage). A SIMD holds waves w and w + 4, so each
// SIMD runs one 3-tap and one 2-tap wave (40 MFMAs per k step, as WF 0) or two 2-tap waves. Every output
// element is the same chain of the same MFMAs over the same fragments in both forms: the same bits.
template <int WF>
__global__ __launch_bounds__(WI_NT) void conv_wgrad_px_kernel(WgPx a, float* __restrict__ part,
                                                              float* __restrict__ bpart) {
  constexpr int NT = WF ? 3 : 5, NI = WF ? 4 : 2;  // taps and 16-row co fragments per wave
  extern __shared__ __attribute__((aligned(16))) bf16_t lds_img[];
  bf16_t* ldy = lds_img;                                      // [KS][WI_LD]
  bf16_t* lx = lds_img + (size_t)a.KS * WI_LD;                // [XR + 1][WI_LD], row XR = zeros
  uint16_t* tmask = reinterpret_cast<uint16_t*>(lx + (size_t)(a.XR + 1) * WI_LD);  // [KS]
  __shared__ float bred[WI_NT / 8][64];
  const int H = a.H, W = a.W, HW = H * W, NR = a.E * HW;
  const int nci = (a.Cin + 63) / 64;
  // workgroup -> (tile, split). remap: workgroup ids congruent mod 8 run on one XCD; they take
  // consecutive split-major work items, so the tiles of one env range read its X / dY through one L2
  int tile = blockIdx.x, split = blockIdx.y;
  if (a.remap) {
    const int L = blockIdx.x + blockIdx.y * gridDim.x, per = (gridDim.x * gridDim.y) >> 3;
    const int Lp = (L & 7) * per + (L >> 3);
    tile = Lp % a.tiles;
    split = Lp / a.tiles;
  }
  const int cit = tile % nci, cot = tile / nci;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wc = wave & 1;
  const int tg = WF ? wave >> 1 : wave >> 2, wr = WF ? 0 : (wave >> 1) & 1;
  const int tap0 = WF ? (tg ? 2 * tg + 1 : 0) : 5 * tg, ntap = WF ? (tg ? 2 : 3) : (tg ? 4 : 5);
  const int ch = tid & 7;
  const int co_s = cot * 64 + ch * 8, ci_s = cit * 64 + ch * 8;
  const bool do_bias = bpart && cit == 0;
  float bacc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) bacc[j] = 0.f;
  if (tid < 8) *reinterpret_cast<uint4*>(lx + (size_t)a.XR * WI_LD + tid * 8) = make_uint4(0, 0, 0, 0);
  for (int r = tid; r < a.KS; r += WI_NT) {  // bit t: tap t of pixel row r stays inside its image
    uint32_t m = 0u;
    if (r < NR) {
      const int p = r % HW, y = p / W, x = p - (p / W) * W;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int sy = y + t / 3 - 1, sx = x + t % 3 - 1;
        if (sy >= 0 && sy < H && sx >= 0 && sx < W) m |= 1u << t;
      }
    }
    tmask[r] = (uint16_t)m;
  }
  f32x4_t acc[NT][NI][2];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int g = lane >> 4, q = (lane & 15) >> 2, pp = lane & 3;
  const int nst_total = a.B / a.E;
  const int st0 = split * a.stages_per_split, st1 = min(nst_total, st0 + a.stages_per_split);
  // every chunk of a stage in one register batch (the planner guarantees (KS + XR) * 8 <= WI_PFN * WI_NT):
  // the next stage's loads are in flight during this stage's MFMAs. Offsets from the stage's env-0 base
  // are the same for every stage.
  const int nchunk = (a.KS + a.XR) * 8;
  // chunk u of a stage: offset from the stage's env-0 base, -1 for a zero chunk (WF 1 recomputes it per stage
  // instead of holding WI_PFN offsets in registers beside its larger accumulator set)
  auto chunk_off = [&](int u) {
    int off = -1;
    const int i = u * WI_NT + tid;
    if (i < a.KS * 8) {
      const int r = i >> 3;
      if (r < NR && co_s < a.Cout) off = r * a.Cout + co_s;
    } else if (i < nchunk) {
      const int r = (i >> 3) - a.KS;
      if (ci_s < a.Cin) off = r * a.Cin + ci_s;
    }
    return off;
  };
  int soff[WF ? 1 : WI_PFN];
  if constexpr (!WF) {
#pragma unroll
    for (int u = 0; u < WI_PFN; ++u) soff[u] = chunk_off(u);
  }
  uint4 pf[WI_PFN];
  auto load_stage = [&](int st) {
    const int b0 = st * a.E, sg = b0 / a.Bseg, bl = b0 - sg * a.Bseg;
    const bf16_t* xb = a.xs[sg] + (size_t)bl * HW * a.Cin;
    const bf16_t* db = a.dys[sg] + (size_t)bl * HW * a.Cout;
    int offs[WI_PFN];
#pragma unroll
    for (int u = 0; u < WI_PFN; ++u) {
      if constexpr (WF) offs[u] = chunk_off(u);
      else offs[u] = soff[u];
    }
#pragma unroll
    for (int u = 0; u < WI_PFN; ++u)
      pf[u] = *reinterpret_cast<const uint4*>((u * WI_NT + tid < a.KS * 8 ? db : xb) + (offs[u] >= 0 ? offs[u] : 0));
#pragma unroll
    for (int u = 0; u < WI_PFN; ++u)
      if (offs[u] < 0) pf[u] = make_uint4(0, 0, 0, 0);
  };
  auto store_stage = [&]() {
#pragma unroll
    for (int u = 0; u < WI_PFN; ++u) {
      const int i = u * WI_NT + tid;
      if (i < a.KS * 8) {
        *reinterpret_cast<uint4*>(ldy + (size_t)(i >> 3) * WI_LD + ch * 8) = pf[u];
        if (do_bias) {
          const bf16_t* h = reinterpret_cast<const bf16_t*>(&pf[u]);
#pragma unroll
          for (int j = 0; j < 8; ++j) bacc[j] += bf16_to_f32(h[j]);
        }
      } else if (i < nchunk) {
        *reinterpret_cast<uint4*>(lx + (size_t)((i >> 3) - a.KS) * WI_LD + ch * 8) = pf[u];
      }
    }
  };
  if (st0 < st1) load_stage(st0);
  for (int st = st0; st < st1; ++st) {
    __syncthreads();  // previous stage fully consumed (first pass: the zero row and mask table written)
    store_stage();
    __syncthreads();
    if (st + 1 < st1) load_stage(st + 1);
    if constexpr (WF == 2) {
      // the k steps software-pipelined: the last tap's MFMAs of step ks interleave the A fragments and the
      // first tap's B fragments of step ks + 1 (each register refilled right after the last MFMA reading it),
      // so a step no longer opens on a full LDS round trip. The same MFMAs in the same order per element.
      const int nks = a.KS / 32;
      int r0 = 4 * g + q, r1 = r0 + 16;
      uint32_t m0 = tmask[r0], m1 = tmask[r1];
      auto afrag = [&](int i, int s0, int s1) {
        const int c = i * 16 + 4 * pp;
        return tr_frag_at(ldy + (size_t)s0 * WI_LD + c, ldy + (size_t)s1 * WI_LD + c);
      };
      auto bload = [&](int t, int s0, int s1, uint32_t k0, uint32_t k1, bf16x8_t (&b)[2]) {
        const int off = (t / 3 - 1) * W + (t % 3 - 1);
        const int x0 = (k0 >> t) & 1u ? s0 + off : a.XR, x1 = (k1 >> t) & 1u ? s1 + off : a.XR;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int c = wc * 32 + j * 16 + 4 * pp;
          b[j] = tr_frag_at(lx + (size_t)x0 * WI_LD + c, lx + (size_t)x1 * WI_LD + c);
        }
      };
      bf16x8_t af[NI], bcur[2], bnxt[2];
#pragma unroll
      for (int i = 0; i < NI; ++i) af[i] = afrag(i, r0, r1);
      bload(tap0, r0, r1, m0, m1, bcur);
      for (int ks = 0; ks < nks; ++ks) {
        // the last step re-reads its own rows (valid addresses, results unused): no branches in the loop
        const int step = ks + 1 < nks ? 32 : 0;
        const int n0 = r0 + step, n1 = r1 + step;
        const uint32_t nm0 = tmask[n0], nm1 = tmask[n1];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          if (tt < ntap) {  // wave-uniform
            if (tt + 1 < ntap) {
              bload(tap0 + tt + 1, r0, r1, m0, m1, bnxt);
#pragma unroll
              for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                  acc[tt][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bcur[j], acc[tt][i][j], 0, 0, 0);
              bcur[0] = bnxt[0];
              bcur[1] = bnxt[1];
            } else {
#pragma unroll
              for (int i = 0; i < NI; ++i) {
#pragma unroll
                for (int j = 0; j < 2; ++j)
                  acc[tt][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bcur[j], acc[tt][i][j], 0, 0, 0);
                af[i] = afrag(i, n0, n1);
              }
              bload(tap0, n0, n1, nm0, nm1, bcur);
            }
          }
        }
        r0 = n0;
        r1 = n1;
        m0 = nm0;
        m1 = nm1;
      }
    } else {
      for (int ks = 0; ks < a.KS / 32; ++ks) {
        const int r0 = ks * 32 + 4 * g + q, r1 = r0 + 16;
        const uint32_t m0 = tmask[r0], m1 = tmask[r1];
        bf16x8_t af[NI];
  #pragma unroll
        for (int i = 0; i < NI; ++i) {
          const int c = wr * 32 + i * 16 + 4 * pp;
          af[i] = tr_frag_at(ldy + (size_t)r0 * WI_LD + c, ldy + (size_t)r1 * WI_LD + c);
        }
        auto bload = [&](int t, bf16x8_t (&b)[2]) {
          const int off = (t / 3 - 1) * W + (t % 3 - 1);
          const int x0 = (m0 >> t) & 1u ? r0 + off : a.XR, x1 = (m1 >> t) & 1u ? r1 + off : a.XR;
  #pragma unroll
          for (int j = 0; j < 2; ++j) {
            const int c = wc * 32 + j * 16 + 4 * pp;
            b[j] = tr_frag_at(lx + (size_t)x0 * WI_LD + c, lx + (size_t)x1 * WI_LD + c);
          }
        };
        bf16x8_t bcur[2], bnxt[2];
        bload(tap0, bcur);
  #pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          if (tt < ntap) {  // wave-uniform: the last tap group(s) have one tap fewer
            if (tt + 1 < ntap) bload(tap0 + tt + 1, bnxt);
  #pragma unroll
            for (int i = 0; i < NI; ++i)
  #pragma unroll
              for (int j = 0; j < 2; ++j)
                acc[tt][i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bcur[j], acc[tt][i][j], 0, 0, 0);
            if (tt + 1 < ntap) { bcur[0] = bnxt[0]; bcur[1] = bnxt[1]; }
          }
        }
      }
    }
  }
  const size_t K = (size_t)9 * a.Cin;
  float* outp = part + (size_t)split * a.Cout * K;
  const int fr = lane & 15, fk = lane >> 4;
#pragma unroll
  for (int tt = 0; tt < NT; ++tt)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int t = tap0 + tt;
        const int ci = cit * 64 + wc * 32 + j * 16 + fr;
        if (tt >= ntap) continue;
        if (ci >= a.Cin) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int co = cot * 64 + wr * 32 + i * 16 + 4 * fk + r;
          if (co < a.Cout) outp[(size_t)co * K + (size_t)t * a.Cin + ci] = acc[tt][i][j][r];
        }
      }
  if (do_bias) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) bred[tid >> 3][ch * 8 + j] = bacc[j];
    __syncthreads();
    if (tid < 64) {
      float sum = 0.f;
      for (int r = 0; r < WI_NT / 8; ++r) sum += bred[r][tid];
      const int co = cot * 64 + tid;
      if (co < a.Cout) bpart[(size_t)split * a.Cout + co] = sum;
    }
  }
}

struct WgPxPlan {
  WgPx a;
  int nsplit;
  size_t lds;
};
// B = all envs (nseg * Bseg); E (envs per stage) divides Bseg, so a stage never straddles a segment and
// every stage is full; false when one env's stage does not fit the register batch or the LDS budget
static bool wgrad_px_plan(int B, int Bseg, int H, int W, int Cin, int Cout, WgPxPlan& p) {
  const int HW = H * W;
  if (HW <= 0 || Bseg <= 0 || B % Bseg) return false;
  auto ksr = [&](int e) { return (e * HW + 31) / 32 * 32; };
  auto bytes = [&](int e) { return (size_t)(ksr(e) + e * HW + 1) * WI_LD * 2 + (size_t)ksr(e) * 2; };
  auto fits = [&](int e) { return bytes(e) <= WI_LDS_MAX && (ksr(e) + e * HW) * 8 <= WI_PFN * WI_NT; };
  if (!fits(1)) return false;
  int E = 1;
  while (E < 64 && Bseg % (E * 2) == 0 && fits(E * 2)) E *= 2;
  const int tiles = ((Cout + 63) / 64) * ((Cin + 63) / 64);
  const int stages = B / E;
  int nsplit = (256 + tiles - 1) / tiles;  // one workgroup per CU
  if (nsplit > stages) nsplit = stages;
  const int sps = (stages + nsplit - 1) / nsplit;
  nsplit = (stages + sps - 1) / sps;
  p.a = WgPx{B, H, W, Cin, Cout, E, ksr(E), E * HW, sps, Bseg, tiles, (tiles * nsplit) % 8 == 0, {}, {}};
  p.nsplit = nsplit;
  p.lds = bytes(E);
  return true;
}

// the weight and bias partials of one split weight-gradient launch, summed in one launch: acc[i] += sum_s
// part[s][i] for i < n, bacc[j] += sum_s bpart[s][j] for j < nb, each element in split order (round 4: one launch
// instead of one per buffer, the same sums)
constexpr int SP_FK = 16;
__global__ void sum_partials2_kernel(const float* __restrict__ part, const float* __restrict__ bpart, int nsplit,
                                     size_t n, size_t nb, float* __restrict__ acc, float* __restrict__ bacc) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n + nb; i += (size_t)gridDim.x * blockDim.x) {
    const bool w = i < n;
    const float* p = w ? part + i : bpart + (i - n);
    const size_t st = w ? n : nb;
    // the first SP_FK partials loaded before the first add (a rolled loop waited one round trip per split); the
    // adds keep split order
    float* dst = w ? acc + i : bacc + (i - n);
    const float a0 = *dst;  // loaded with the partials (read after the sum it was one more round trip)
    float v[SP_FK];
#pragma unroll
    for (int k = 0; k < SP_FK; ++k) v[k] = k < nsplit ? p[(size_t)k * st] : 0.f;
    float s = v[0];
#pragma unroll
    for (int k = 1; k < SP_FK; ++k)
      if (k < nsplit) s += v[k];
    for (int k = SP_FK; k < nsplit; ++k) s += p[(size_t)k * st];
    *dst = a0 + s;
  }
}

}  // namespace

void mz_sum_partials2(const float* part, const float* bpart, int nsplit, size_t n, size_t nb, float* acc, float* bacc,
                      hipStream_t stream) {
  hipLaunchKernelGGL(sum_partials2_kernel, dim3(grid_for(n + nb)), dim3(256), 0, stream, part, bpart, nsplit, n, nb, acc,
                     bacc);
}

extern "C" {

static long long wgrad_splits(long long M, long long tiles) {
  long long nsplit = (512 + tiles - 1) / tiles;  // >= 2 workgroups per CU
  const long long maxs = (M + 255) / 256;        // >= 256 rows per split
  if (nsplit > maxs) nsplit = maxs;
  return nsplit < 1 ? 1 : nsplit;
}

static thread_local int g_wgrad_img = 1;
// 1 (default): bf16 3x3 weight gradients on the whole-image kernel where it wins (see
// wgrad_img_eligible); 2: whole-image kernel for every supported shape; 0: per-tap kernel only
int mzba_conv_wgrad_set_variant(int v) {
  if (v < 0 || v > 2) return -1;
  g_wgrad_img = v;
  return 0;
}
// which whole-image kernel: 2 (default) pixel rows with 64-co wave tiles (conv_wgrad_px_kernel<1>), 1 pixel
// rows with 32-co wave tiles (conv_wgrad_px_kernel<0>, the same bits, 3-6 % slower per launch), 0 zero-bordered
// images (conv_wgrad_img_kernel, the round-5 form); 1 and 0 for A/B; 3 = form 2 with the k steps
// software-pipelined (conv_wgrad_px_kernel<2>, the same bits)
static thread_local int g_wgrad_form = 2;
int mzba_conv_wgrad_set_form(int v) {
  if (v < 0 || v > 3) return -1;
  g_wgrad_form = v;
  return 0;
}

long long mzba_conv_wgrad_ws_bytes(int B, int H, int W, int Cin, int Cout, int ks) {
  const long long M = (long long)B * H * W;
  const long long tiles = (long long)((Cout + 63) / 64) * ((Cin + 63) / 64) * ks * ks;
  long long n = wgrad_splits(M, tiles);
  WgPlan p;
  if (ks == 3 && Cin % 8 == 0 && Cout % 8 == 0 && wgrad_img_plan(B, 1, H, W, Cin, Cout, p) && p.nsplit > n) n = p.nsplit;
  WgPxPlan px;
  if (ks == 3 && Cin % 8 == 0 && Cout % 8 == 0 && wgrad_px_plan(B, 1, H, W, Cin, Cout, px) && px.nsplit > n) n = px.nsplit;
  return n * ((long long)Cout * ks * ks * Cin + Cout) * 4;
}

// a whole-image kernel for nseg segments of B envs (its plan may still refuse the shape)
static bool wgrad_img_eligible(int dtype, int nseg, int B, int H, int W, int Cin, int Cout, int ks) {
  // it wins where an image has many pixels per tap re-read (8x10: 138 vs 277 us, 16x20: 153 vs
  // 283 us at B = 512) and, at 4x5, once the K unrolled uses of a conv reduce in one launch
  // (per-tap kernel: 80 us per use; 5 x 512 at 256 -> 256: 188 vs 401 us, and 362 vs 464 us for
  // the dynamics ConvBlock's 264 input channels; tools/bench_wgrad_segs.py)
  if (dtype != 1 || ks != 3 || !g_wgrad_img || Cin % 8 || Cout % 8) return false;
  return H * W >= 64 || g_wgrad_img == 2 || nseg * B >= 2048;
}

static int wgrad_core(int dtype, const void* const* xs, const void* const* dys, int nseg, int B, int H, int W, int Cin,
                      int Cout, int ks, float* dw, float* db, void* ws, long long ws_bytes, hipStream_t stream) {
  MZ_CHECK_ARG(xs && dys && dw && ws && B > 0 && nseg >= 1 && nseg <= WG_MAXSEG && (ks == 1 || ks == 3) &&
               Cin % 4 == 0 && Cout % 4 == 0, -1);
  MZ_CHECK_ARG(dtype == 0 || (Cin % 8 == 0 && Cout % 8 == 0), -1);
  MZ_CHECK_ARG(dtype == 0 || dtype == 1, -9);
  for (int i = 0; i < nseg; ++i) MZ_CHECK_ARG(xs[i] && dys[i], -1);
  MZ_CHECK_ARG(mzba_conv_wgrad_ws_bytes(nseg * B, H, W, Cin, Cout, ks) <= ws_bytes, -2);
  WgPxPlan pxp;
  if (g_wgrad_form >= 1 && wgrad_img_eligible(dtype, nseg, B, H, W, Cin, Cout, ks) &&
      wgrad_px_plan(nseg * B, B, H, W, Cin, Cout, pxp)) {
    for (const void* k : {reinterpret_cast<const void*>(&conv_wgrad_px_kernel<0>),
                          reinterpret_cast<const void*>(&conv_wgrad_px_kernel<1>),
                          reinterpret_cast<const void*>(&conv_wgrad_px_kernel<2>)}) {
      const hipError_t e = mz_set_lds_max_once(k, (int)WI_LDS_MAX);
      if (e != hipSuccess) return (int)e;
    }
    for (int i = 0; i < nseg; ++i) {
      pxp.a.xs[i] = (const bf16_t*)xs[i];
      pxp.a.dys[i] = (const bf16_t*)dys[i];
    }
    const size_t nwi = (size_t)Cout * 9 * Cin;
    float* ipart = (float*)ws;
    float* ibpart = db ? ipart + (size_t)pxp.nsplit * nwi : nullptr;
    if (g_wgrad_form == 3)
      hipLaunchKernelGGL(conv_wgrad_px_kernel<2>, dim3(pxp.a.tiles, pxp.nsplit), dim3(WI_NT), pxp.lds, stream, pxp.a,
                         ipart, ibpart);
    else if (g_wgrad_form == 2)
      hipLaunchKernelGGL(conv_wgrad_px_kernel<1>, dim3(pxp.a.tiles, pxp.nsplit), dim3(WI_NT), pxp.lds, stream, pxp.a,
                         ipart, ibpart);
    else
      hipLaunchKernelGGL(conv_wgrad_px_kernel<0>, dim3(pxp.a.tiles, pxp.nsplit), dim3(WI_NT), pxp.lds, stream, pxp.a,
                         ipart, ibpart);
    const size_t nbi = db ? (size_t)Cout : 0;
    hipLaunchKernelGGL(sum_partials2_kernel, dim3(grid_for(nwi + nbi)), dim3(256), 0, stream, (const float*)ipart,
                       (const float*)ibpart, pxp.nsplit, nwi, nbi, dw, db);
    MZ_LAUNCH_CHECK();
    return 0;
  }
  WgPlan ip;
  if (wgrad_img_eligible(dtype, nseg, B, H, W, Cin, Cout, ks) && wgrad_img_plan(nseg * B, B, H, W, Cin, Cout, ip)) {
    // the 16x20 images need more than the default 64 KB of dynamic LDS
    for (const void* k : {reinterpret_cast<const void*>(&conv_wgrad_img_kernel<false>),
                          reinterpret_cast<const void*>(&conv_wgrad_img_kernel<true>)}) {
      const hipError_t e = mz_set_lds_max_once(k, (int)WI_LDS_MAX);
      if (e != hipSuccess) return (int)e;
    }
    ip.a.Bseg = B;
    for (int i = 0; i < nseg; ++i) {
      ip.a.xs[i] = (const bf16_t*)xs[i];
      ip.a.dys[i] = (const bf16_t*)dys[i];
    }
    const size_t nwi = (size_t)Cout * 9 * Cin;
    float* ipart = (float*)ws;
    float* ibpart = db ? ipart + (size_t)ip.nsplit * nwi : nullptr;
    const dim3 grid(((Cout + 63) / 64) * ((Cin + 63) / 64), ip.nsplit);
    if (ip.pf)
      hipLaunchKernelGGL(conv_wgrad_img_kernel<true>, grid, dim3(WI_NT), ip.lds, stream, ip.a, ipart, ibpart);
    else
      hipLaunchKernelGGL(conv_wgrad_img_kernel<false>, grid, dim3(WI_NT), ip.lds, stream, ip.a, ipart, ibpart);
    const size_t nbi = db ? (size_t)Cout : 0;
    hipLaunchKernelGGL(sum_partials2_kernel, dim3(grid_for(nwi + nbi)), dim3(256), 0, stream, (const float*)ipart,
                       (const float*)ibpart, ip.nsplit, nwi, nbi, dw, db);
    MZ_LAUNCH_CHECK();
    return 0;
  }
  // per-tap tile kernels, one launch pair per segment (accumulated into dw / db in segment order)
  const long long M = (long long)B * H * W;
  const long long tiles = (long long)((Cout + 63) / 64) * ((Cin + 63) / 64) * ks * ks;
  const long long nsplit = wgrad_splits(M, tiles);
  const int step = dtype ? WB_M : WG_ROWS;
  const int rps = (int)(((M + nsplit - 1) / nsplit + step - 1) / step * step);
  const size_t nw = (size_t)Cout * ks * ks * Cin;
  float* part = (float*)ws;
  float* bpart = db ? part + nsplit * nw : nullptr;
  for (int i = 0; i < nseg; ++i) {
    if (dtype == 1)
      hipLaunchKernelGGL(conv_wgrad_bf16_kernel, dim3((unsigned)tiles, (unsigned)nsplit), dim3(256), 0, stream,
                         (const bf16_t*)xs[i], (const bf16_t*)dys[i], B, H, W, Cin, Cout, ks, rps, part, bpart);
    else
      hipLaunchKernelGGL(conv_wgrad_kernel<float>, dim3((unsigned)tiles, (unsigned)nsplit), dim3(256), 0, stream,
                         (const float*)xs[i], (const float*)dys[i], B, H, W, Cin, Cout, ks, rps, part, bpart);
    const size_t nb = db ? (size_t)Cout : 0;
    hipLaunchKernelGGL(sum_partials2_kernel, dim3(grid_for(nw + nb)), dim3(256), 0, stream, (const float*)part,
                       (const float*)bpart, (int)nsplit, nw, nb, dw, db);
  }
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_conv_wgrad(int dtype, const void* x, const void* dy, int B, int H, int W, int Cin, int Cout, int ks,
                    float* dw, float* db, void* ws, long long ws_bytes, hipStream_t stream) {
  return wgrad_core(dtype, &x, &dy, 1, B, H, W, Cin, Cout, ks, dw, db, ws, ws_bytes, stream);
}

int mzba_conv_wgrad_segs(int dtype, const void* const* xs, const void* const* dys, int nseg, int B, int H, int W,
                         int Cin, int Cout, int ks, float* dw, float* db, void* ws, long long ws_bytes,
                         hipStream_t stream) {
  return wgrad_core(dtype, xs, dys, nseg, B, H, W, Cin, Cout, ks, dw, db, ws, ws_bytes, stream);
}

}  // extern "C"
