// Prioritized replay over the sink archive: priorities in sink-row space, sampled through a
// three-level prefix.
//
// q f32[T B], indexed row * B + env like the sink's tensors: q = p^alpha at the root record of every window of a kept
// segment, exactly 0 at every other row. A root's row does not move when other slabs are appended, so nothing is
// re-indexed; row_window (replay_dev.h) turns a drawn row into the archive's window index of the moment.
//   aprio_init_kernel        q of the rows of one slab: a root gets p = |value - n-step target| + eps, the rest 0;
//   aprio_rows_kernel        row_window for a list of rows (the lookup on its own);
//   the sampler, replay_prio.hip's stratified inverse-CDF with one more level, in five launches:
//     aprio_partials_kernel    a wave per 1024-row block: its f64 sum `part` and its last row with q > 0;
//     aprio_block_scan_kernel  a wave per super-block of 1024 blocks: R[b] = R[b - 1] + part[b] from 0, in place;
//     aprio_super_scan_kernel  one wave: G[g] = G[g - 1] + R[last block of g] over the <= 2048 super-blocks;
//     aprio_sample_kernel      a wave per sample: binary search of G, of R, then the block's own prefix; the lookup;
//     prio_weight_kernel       importance weights over the batch's largest (prio_dev.h).
// Every sum is f64 in one fixed order (no atomics). With lane l of a block's wave owning rows 16 l .. 16 l + 15,
//   C[i] = G[g - 1] + (R[b - 1] + (off_l + s_k)),  R[b] = R[b - 1] + off_64,  G[g] = G[g - 1] + R[last],
// so a lane's last C is the next lane's base, a block's last C is G[g - 1] + R[b], the next block's base, and a
// super-block's last C is G[g]: C never decreases, C[i] > C[i - 1] only where q[i] > 0, and "the first i with
// C[i] > t" is found by the same comparison at every level and is always a live row.
#include "prio_dev.h"
#include "replay_dev.h"

namespace {

constexpr int SB = 1024;       // blocks per super-block
constexpr int MAX_SUP = 2048;  // super-blocks of 2^31 rows
// The sampler's draw: Philox (sample j, stream 7, step, 0). Streams 0-3 are in common.h, 4 in replay_prio.hip, 5 in
// gumbel.hip, 6 in replay.hip.
constexpr int MZ_STREAM_ARCHIVE_PRIO = 7;

// one thread per (row, env) of rows [row0, row0 + nrows): consecutive threads, consecutive envs of one row
__global__ __launch_bounds__(256) void aprio_init_kernel(ReplayRecords r, SegTable tb, const int32_t* __restrict__ offs,
                                                         const int32_t* __restrict__ totals, float* __restrict__ q,
                                                         int row0, int nrows, int K, const float* __restrict__ dpow,
                                                         float alpha, float eps) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)nrows * r.B) return;
  const int i = (int)((long long)row0 * r.B + e);  // < T B < 2^31
  int seg;
  const int j = row_window(tb, offs, totals, r.B, K, r.T * r.B, i, seg);
  float v = 0.f;
  if (j >= 0) {
    const int b = tb.col(0)[seg], t0 = tb.col(1)[seg];
    const float z = nstep_target(r, b, t0, j - tb.col(5)[seg], tb.col(2)[seg], dpow);
    v = prio_q(fabsf(r.value[i] - z), eps, alpha);
  }
  q[i] = v;
}

__global__ __launch_bounds__(256) void aprio_rows_kernel(SegTable tb, const int32_t* __restrict__ offs,
                                                         const int32_t* __restrict__ totals, int B, int K, int n_rows,
                                                         const int32_t* __restrict__ rows, int n,
                                                         int32_t* __restrict__ idx_out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  int seg;
  idx_out[j] = row_window(tb, offs, totals, B, K, n_rows, rows[j], seg);
}

// block b's rows start at q + b PB (16-byte aligned, b PB < n_rows < 2^31) and load16 sees the rows left from
// there on as its cap, so no row index is formed past n_rows
__global__ __launch_bounds__(256) void aprio_partials_kernel(const float* __restrict__ q, int n_rows, int nblk,
                                                             double* __restrict__ part, int32_t* __restrict__ lastpos) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= nblk) return;  // whole waves leave; no barrier below
  const int r0 = b * PB;
  float v[16];
  double s[16], full;
  load16(q + r0, n_rows - r0, 0, lane, v);
  block_prefix(v, lane, s, full);
  int last = -1;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (v[k] > 0.f) last = r0 + lane * 16 + k;
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  if (lane == 0) { part[b] = full; lastpos[b] = last; }
}

// A wave per super-block g, lane l owning its blocks [16 l, 16 l + 16): R[b] = R[b - 1] + part[b] exactly, from 0 at
// the super-block's first block, in place (prio_scan_kernel's turn-taking: lanes continue from the lane before).
// sup[g] = R[last block of g], suplast[g] = the super-block's last row with q > 0 (-1: none).
__global__ __launch_bounds__(256) void aprio_block_scan_kernel(double* __restrict__ part,
                                                               const int32_t* __restrict__ lastpos, int nblk, int nsup,
                                                               double* __restrict__ sup, int32_t* __restrict__ suplast) {
  const int lane = threadIdx.x & 63, g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= nsup) return;  // whole waves leave; no barrier below
  const int bg = g * SB, cntg = min(SB, nblk - bg);
  const int b0 = min(lane * 16, cntg), cnt = min(b0 + 16, cntg) - b0;
  double p[16];
  int last = -1;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    p[k] = k < cnt ? part[bg + b0 + k] : 0.0;
    if (k < cnt) last = max(last, lastpos[bg + b0 + k]);
  }
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
    if (k < cnt) part[bg + b0 + k] = p[k];
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  // lanes past the last block added zeros: run is R[last block of g] on every lane
  if (lane == 0) { sup[g] = run; suplast[g] = last; }
}

// one wave: lane l owns super-blocks [l per, (l + 1) per), per <= 32; G[g] = G[g - 1] + sup[g] exactly, in place.
// suplast[nsup] = the last row of all with q > 0 (-1: none).
__global__ __launch_bounds__(64) void aprio_super_scan_kernel(double* __restrict__ sup, int32_t* __restrict__ suplast,
                                                              int nsup) {
  constexpr int PER = MAX_SUP / 64;
  const int lane = threadIdx.x, per = (nsup + 63) / 64;
  const int g0 = min(lane * per, nsup), cnt = min(g0 + per, nsup) - g0;
  double p[PER];
  int last = -1;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    p[k] = k < cnt ? sup[g0 + k] : 0.0;
    if (k < cnt) last = max(last, suplast[g0 + k]);
  }
  double run = 0.0;
  for (int l = 0; l < 64; ++l) {
    if (l == lane) {
#pragma unroll
      for (int k = 0; k < PER; ++k) { run = run + p[k]; p[k] = run; }
    }
    run = shfl_f64(run, l);
  }
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (k < cnt) sup[g0 + k] = p[k];
  for (int o = 32; o > 0; o >>= 1) last = max(last, __shfl_xor(last, o, 64));
  if (lane == 0) suplast[nsup] = last;
}

// u_j = (x0 2^21 + (x1 >> 11)) 2^-53: 53 random bits, every f64 in [0, 1) of that grid, so a stratum of more than
// 2^24 rows is still reached row by row
MZ_DEV double uniform53(uint32_t j, uint32_t step, uint64_t seed) {
  const u32x4 x = philox4x32(j, MZ_STREAM_ARCHIVE_PRIO, step, 0, seed);
  return ((double)x.x * 2097152.0 + (double)(x.y >> 11)) * 0x1p-53;
}

// A sample is unusable where S == 0 and where the lookup says that its row is no root (q > 0 there only after an
// append between a sample and its update): rows = idx = -1, prob = 0, raw = 0, which the weights' max leaves out.
__global__ __launch_bounds__(256) void aprio_sample_kernel(const float* __restrict__ q, int n_rows, int nblk, int nsup,
                                                           int n, float beta, int n_live, SegTable tb,
                                                           const int32_t* __restrict__ offs,
                                                           const int32_t* __restrict__ totals, int B, int K,
                                                           uint64_t seed, uint32_t step,
                                                           const uint32_t* __restrict__ step_dev,
                                                           const double* __restrict__ u_in, const double* __restrict__ R,
                                                           const double* __restrict__ G,
                                                           const int32_t* __restrict__ suplast,
                                                           int32_t* __restrict__ rows, int32_t* __restrict__ idx,
                                                           float* __restrict__ prob, double* __restrict__ raw) {
  const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= n) return;  // whole waves leave; no barrier below
  if (step_dev) step = step_dev[0];
  const double u = u_in ? u_in[j] : uniform53((uint32_t)j, step, seed);
  const double S = G[nsup - 1];
  const double t = (((double)j + u) / (double)n) * S;
  int row;
  if (!(t < S)) {
    row = suplast[nsup];  // rounding put t at or beyond S: the last live row; S == 0: -1
  } else {
    int lo = 0, hi = nsup - 1;  // first super-block with G[g] > t (G[nsup - 1] = S > t)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (G[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int bg = lo * SB;
    const double gb = lo ? G[lo - 1] : 0.0;
    lo = 0; hi = min(SB, nblk - bg) - 1;  // its first block with gb + R[b] > t (gb + R[last] = G[g] > t)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (gb + R[bg + mid] > t) hi = mid; else lo = mid + 1;
    }
    const int b = bg + lo, r0 = b * PB;
    const double rb = lo ? R[b - 1] : 0.0;
    float v[16];
    double s[16], full;
    load16(q + r0, n_rows - r0, 0, lane, v);
    const double off = block_prefix(v, lane, s, full);
    // gb + (rb + (off + s[15])) of lane 63 is gb + R[b] > t: some lane fires
    const unsigned long long m = __ballot(gb + (rb + (off + s[15])) > t);
    const int hit = m ? __ffsll((long long)m) - 1 : 63;
    int k = 0;
    if (lane == hit) {
      while (k < 15 && !(gb + (rb + (off + s[k])) > t)) ++k;
    }
    const int at = hit * 16 + __shfl(k, hit, 64);
    // at >= the rows left is unreachable while load16 reads 0 past n_rows; keeps every later read inside
    row = at < n_rows - r0 ? r0 + at : suplast[nsup];
  }
  if (lane == 0) {
    bool ok = row >= 0;
    int w = -1, N = n_live;
    if (tb.w) {
      int seg;
      N = totals[1];
      if (ok) w = row_window(tb, offs, totals, B, K, n_rows, row, seg);
      ok = w >= 0;
    }
    ok = ok && N > 0;
    const double pr = ok ? (double)q[row] / S : 0.0;
    rows[j] = ok ? row : -1;
    if (idx) idx[j] = ok ? w : -1;
    prob[j] = (float)pr;
    raw[j] = !ok ? 0.0 : beta == 0.f ? 1.0 : pow((double)N * pr, -(double)beta);
  }
}

struct SampleWs { long long R, lastpos, G, suplast, raw, bytes; int nblk, nsup; };
SampleWs sample_ws(long long n_rows, long long n) {
  SampleWs w;
  w.nblk = (int)((n_rows + PB - 1) / PB);
  w.nsup = (w.nblk + SB - 1) / SB;
  w.R = 0;
  w.lastpos = w.R + align16((long long)w.nblk * 8);
  w.G = w.lastpos + align16((long long)w.nblk * 4);
  w.suplast = w.G + align16((long long)w.nsup * 8);
  w.raw = w.suplast + align16(((long long)w.nsup + 1) * 4);
  w.bytes = w.raw + align16(n * 8);
  return w;
}

bool table_ok(const int32_t* table, int nmax, const int32_t* offs, const int32_t* totals, int B, int K) {
  return table && offs && totals && nmax >= 0 && B > 0 && K > 0;
}

}  // namespace

extern "C" {

int mzba_archive_row_windows(const int32_t* table, int nmax, const int32_t* offs, const int32_t* totals, int B, int K,
                             int n_rows, const int32_t* rows, int n, int32_t* idx_out, hipStream_t stream) {
  MZ_CHECK_ARG(table_ok(table, nmax, offs, totals, B, K) && n_rows >= 0 && n_rows % B == 0 && n >= 0, -1);
  if (n == 0) return 0;
  MZ_CHECK_ARG(rows && idx_out, -1);
  SegTable tb{const_cast<int32_t*>(table), nmax};
  hipLaunchKernelGGL(aprio_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, tb, offs, totals, B, K, n_rows,
                     rows, n, idx_out);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_archive_priority_init(const mzba_sink* sink, const int32_t* table, int nmax, const int32_t* offs,
                               const int32_t* totals, float* q, int row0, int nrows, int K, const float* dpow,
                               float alpha, float eps, hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && (long long)sink->T * sink->B <= 0x7fffffffLL &&
                   table_ok(table, nmax, offs, totals, sink->B, K) && q && dpow && sink->reward && sink->values &&
                   alpha >= 0.f && eps >= 0.f, -1);
  MZ_CHECK_ARG(row0 >= 0 && nrows >= 0 && (long long)row0 + nrows <= sink->T, -1);
  if (nrows == 0) return 0;
  SegTable tb{const_cast<int32_t*>(table), nmax};
  const long long cells = (long long)nrows * sink->B;
  hipLaunchKernelGGL(aprio_init_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, stream,
                     records(*sink, nullptr), tb, offs, totals, q, row0, nrows, K, dpow, alpha, eps);
  MZ_LAUNCH_CHECK();
  return 0;
}

long long mzba_archive_sample_ws_bytes(int n_rows, int n) {
  if (n_rows <= 0 || n <= 0) return -1;
  return sample_ws(n_rows, n).bytes;
}

int mzba_archive_sample(const float* q, int n_rows, int n, float beta, int n_live, const int32_t* table, int nmax,
                        const int32_t* offs, const int32_t* totals, int B, int K, uint64_t seed, uint32_t step,
                        const uint32_t* step_dev, const double* u_in, int32_t* rows, int32_t* idx, float* prob,
                        float* weight, void* ws, long long ws_bytes, hipStream_t stream) {
  MZ_CHECK_ARG(q && rows && prob && weight && ws && n_rows > 0 && n > 0 && n <= (1 << 20) && beta >= 0.f, -1);
  if (table) {  // rows are looked up: N is the table's window count, read on the device
    MZ_CHECK_ARG(table_ok(table, nmax, offs, totals, B, K) && idx && n_rows % B == 0, -1);
  } else {      // the plain row sampler
    MZ_CHECK_ARG(n_live > 0 && n_live <= n_rows, -3);
  }
  const SampleWs w = sample_ws(n_rows, n);
  MZ_CHECK_ARG(((uintptr_t)q & 15) == 0 && ((uintptr_t)ws & 15) == 0 && w.bytes <= ws_bytes && w.nsup <= MAX_SUP, -2);
  char* base = (char*)ws;
  double *R = (double*)(base + w.R), *G = (double*)(base + w.G), *raw = (double*)(base + w.raw);
  int32_t *lastpos = (int32_t*)(base + w.lastpos), *suplast = (int32_t*)(base + w.suplast);
  SegTable tb{const_cast<int32_t*>(table), table ? nmax : 0};
  hipLaunchKernelGGL(aprio_partials_kernel, dim3((w.nblk + 3) / 4), dim3(256), 0, stream, q, n_rows, w.nblk, R,
                     lastpos);
  hipLaunchKernelGGL(aprio_block_scan_kernel, dim3((w.nsup + 3) / 4), dim3(256), 0, stream, R,
                     (const int32_t*)lastpos, w.nblk, w.nsup, G, suplast);
  hipLaunchKernelGGL(aprio_super_scan_kernel, dim3(1), dim3(64), 0, stream, G, suplast, w.nsup);
  hipLaunchKernelGGL(aprio_sample_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, q, n_rows, w.nblk, w.nsup, n, beta,
                     n_live, tb, offs, totals, B, K, seed, step, step_dev, u_in, (const double*)R, (const double*)G,
                     (const int32_t*)suplast, rows, idx, prob, raw);
  hipLaunchKernelGGL(prio_weight_kernel, dim3(1), dim3(256), 0, stream, (const double*)raw, n, weight);
  MZ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
