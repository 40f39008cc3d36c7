// Episode statistics of a streamed sink on the device: returns, lengths, a return histogram, the
// calibration of the searched root values against the discounted return, and the search's mean value and target
// entropy, accumulated into one device block with no host read.
//
// Segments as in replay.hip: env b's rows from a non-zero start word up to the row before the next one, or up to T;
// the records are the masked rows, L of them. A segment is closed if another start word follows it, the last one iff
// done[b] || hlen[b] >= cap_len. An episode is a closed segment with L >= 1; per env they are numbered in row order and
// episode i is counted iff first_n == 0 || i < first_n.
//   episode_stats_env_kernel   one thread per env (lanes read consecutive envs of a row), two walks of its column:
//       forward  (start, mask, reward; 9 bytes a row, the plan's reads): R = the f32 sum of the rewards in row order
//                (for_each_kept_segment's sum), L, the histogram bin, ep_ret / ep_len, and the number of episodes;
//       backward (start, mask, reward, values, counts; 37 bytes a row): G_t = r_t + gamma G_{t+1} in double from 0
//                past the last record, the value error e_t = values[t] - G_t of episodes with L < cap_len, the value sum
//                and the entropy of counts / sum(counts). A segment's sums are committed at its start word, when L and
//                its episode number (the forward count minus the episodes already met) are known.
//       The env's partial sums go to the workspace, 45 words of 8 bytes per env, word w of env b at [w][b].
//   episode_stats_fold_kernel  one workgroup: thread i adds envs i, i + 256, ... in that order, a fixed tree over the
//       256 threads adds those, thread 0 (the histogram: threads 0..31) adds the fold to the block.
// No floating-point atomics: the same sink gives the same bits on every run, whatever the launch shape of the first
// kernel. Rows outside a segment's records are not read (but for start and mask). Compiled with -ffp-contract=off.
#include <float.h>
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {

// workspace words per env: i64 sums, then f64 sums, then the packed extremes
enum {
  W_EPISODES = 0, W_CAPPED, W_ROWS, W_VERR_ROWS, W_HIST,  // i64; 32 histogram bins from W_HIST on
  W_F64 = W_HIST + 32,                                    // ret_sum, ret_sq, verr_sum, verr_abs, verr_sq, value_sum,
  N_F64 = 7,                                              //   entropy_sum
  W_RET_MM = W_F64 + N_F64,                               // {ret_min, ret_max} f32 x 2
  W_LEN_MM,                                               // {len_min, len_max} i32 x 2
  W_WORDS
};
constexpr int FT = 256;

struct StatsArgs {
  const uint32_t* start;  // [T][B]
  const uint8_t* mask;    // [T][B]
  const float* reward;    // [T][B]
  const float* values;    // [T][B]
  const int64_t* counts;  // [T][B][3]
  const uint8_t* done;    // [B]
  const int32_t* hlen;    // [B]
  int T, B, cap_len, first_n, ep_n;
  double gamma, hist_lo, hist_step;
  float* ep_ret;          // [B][ep_n] or NULL
  int32_t* ep_len;        // [B][ep_n] or NULL
};

// -sum p ln p of p = c / sum(c) in double; 0 ln 0 = 0; a row with sum(c) <= 0 gives 0
MZ_DEV double row_entropy(const int64_t* __restrict__ c) {
  const int64_t c0 = c[0], c1 = c[1], c2 = c[2];
  const int64_t n = c0 + c1 + c2;
  if (n <= 0) return 0.0;
  const double dn = (double)n;
  double h = 0.0;
  if (c0 > 0) { const double p = (double)c0 / dn; h = h - p * log(p); }
  if (c1 > 0) { const double p = (double)c1 / dn; h = h - p * log(p); }
  if (c2 > 0) { const double p = (double)c2 / dn; h = h - p * log(p); }
  return h;
}

__global__ __launch_bounds__(256) void episode_stats_env_kernel(StatsArgs a, uint64_t* __restrict__ ws) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= a.B) return;
  const size_t B = a.B;
  int64_t* wi = reinterpret_cast<int64_t*>(ws);
  double* wd = reinterpret_cast<double*>(ws);
  for (int k = 0; k < 32; ++k) wi[(size_t)(W_HIST + k) * B + b] = 0;
  const bool tail_closed = a.done[b] != 0 || a.hlen[b] >= a.cap_len;

  // ---- forward: returns, lengths, the histogram, the per-env lists, the number of episodes
  int64_t episodes = 0, capped = 0, rows = 0;
  double ret_sum = 0.0, ret_sq = 0.0;
  float ret_min = FLT_MAX, ret_max = -FLT_MAX;
  int len_min = INT_MAX, len_max = 0;
  int nep = 0, nout = 0;  // episodes met (counted or not); counted ones written to ep_ret / ep_len
  {
    int t0 = -1, L = 0;
    float s = 0.f;
    auto close = [&](bool closed) {
      if (t0 < 0 || !closed || L < 1) return;
      if (a.first_n == 0 || nep < a.first_n) {
        const double R = (double)s;
        ++episodes; rows += L; capped += L >= a.cap_len ? 1 : 0;
        ret_sum = ret_sum + R; ret_sq = ret_sq + R * R;
        ret_min = s < ret_min ? s : ret_min; ret_max = s > ret_max ? s : ret_max;
        len_min = L < len_min ? L : len_min; len_max = L > len_max ? L : len_max;
        const double x = floor((R - a.hist_lo) / a.hist_step);
        const int bin = x > 0.0 ? (x < 31.0 ? (int)x : 31) : 0;
        wi[(size_t)(W_HIST + bin) * B + b] += 1;
        if (nout < a.ep_n) {
          if (a.ep_ret) a.ep_ret[(size_t)b * a.ep_n + nout] = s;
          if (a.ep_len) a.ep_len[(size_t)b * a.ep_n + nout] = L;
          ++nout;
        }
      }
      ++nep;
    };
    for (int t = 0; t < a.T; ++t) {  // lanes of a wave read consecutive envs of row t
      const size_t i = (size_t)t * B + b;
      if (a.start[i]) {
        close(true);
        t0 = t; L = 0; s = 0.f;
      }
      if (t0 >= 0 && a.mask[i]) {
        s = s + a.reward[i];  // for_each_kept_segment's sum (replay.hip)
        ++L;
      }
    }
    close(tail_closed);
    for (int k = nout; k < a.ep_n; ++k) {
      if (a.ep_ret) a.ep_ret[(size_t)b * a.ep_n + k] = 0.f;
      if (a.ep_len) a.ep_len[(size_t)b * a.ep_n + k] = 0;
    }
  }

  // ---- backward: G_t, the value error, the value and entropy sums
  int64_t verr_rows = 0;
  double verr_sum = 0.0, verr_abs = 0.0, verr_sq = 0.0, value_sum = 0.0, entropy_sum = 0.0;
  if (nep > 0) {
    int k = nep, L = 0;
    bool last = true;
    double G = 0.0, es = 0.0, ea = 0.0, eq = 0.0, vs = 0.0, hs = 0.0;
    for (int t = a.T - 1; t >= 0 && k > 0; --t) {
      const size_t i = (size_t)t * B + b;
      const uint32_t w = a.start[i];
      if (a.mask[i]) {
        const double v = (double)a.values[i];
        G = (double)a.reward[i] + a.gamma * G;
        const double e = v - G;
        es = es + e; ea = ea + fabs(e); eq = eq + e * e;
        vs = vs + v;
        hs = hs + row_entropy(a.counts + i * 3);
        ++L;
      }
      if (w) {
        if ((!last || tail_closed) && L >= 1) {
          --k;
          if (a.first_n == 0 || k < a.first_n) {
            value_sum = value_sum + vs; entropy_sum = entropy_sum + hs;
            if (L < a.cap_len) {  // a true terminal: the return past the last record is 0
              verr_rows += L;
              verr_sum = verr_sum + es; verr_abs = verr_abs + ea; verr_sq = verr_sq + eq;
            }
          }
        }
        last = false;
        L = 0; G = 0.0; es = ea = eq = vs = hs = 0.0;
      }
    }
  }

  wi[(size_t)W_EPISODES * B + b] = episodes;
  wi[(size_t)W_CAPPED * B + b] = capped;
  wi[(size_t)W_ROWS * B + b] = rows;
  wi[(size_t)W_VERR_ROWS * B + b] = verr_rows;
  wd[(size_t)(W_F64 + 0) * B + b] = ret_sum;
  wd[(size_t)(W_F64 + 1) * B + b] = ret_sq;
  wd[(size_t)(W_F64 + 2) * B + b] = verr_sum;
  wd[(size_t)(W_F64 + 3) * B + b] = verr_abs;
  wd[(size_t)(W_F64 + 4) * B + b] = verr_sq;
  wd[(size_t)(W_F64 + 5) * B + b] = value_sum;
  wd[(size_t)(W_F64 + 6) * B + b] = entropy_sum;
  reinterpret_cast<float2*>(ws)[(size_t)W_RET_MM * B + b] = make_float2(ret_min, ret_max);
  reinterpret_cast<int2*>(ws)[(size_t)W_LEN_MM * B + b] = make_int2(len_min, len_max);
}

// sh[0] = f over the 256 entries, the same tree on every run
template <typename T, typename F>
MZ_DEV T fold_tree(T* sh, T mine, F f) {
  const int tid = threadIdx.x;
  __syncthreads();  // the previous fold's sh[0] has been read
  sh[tid] = mine;
  __syncthreads();
  for (int o = FT / 2; o > 0; o >>= 1) {
    if (tid < o) sh[tid] = f(sh[tid], sh[tid + o]);
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(FT) void episode_stats_fold_kernel(const uint64_t* __restrict__ ws, int nB,
                                                                mzba_episode_stats* __restrict__ blk) {
  __shared__ int64_t shi[FT];
  __shared__ double shd[FT];
  __shared__ float shf[FT];
  __shared__ int shn[FT];
  const int tid = threadIdx.x;
  const size_t B = nB;
  const int64_t* wi = reinterpret_cast<const int64_t*>(ws);
  const double* wd = reinterpret_cast<const double*>(ws);
  const auto addi = [](int64_t x, int64_t y) { return x + y; };
  const auto addd = [](double x, double y) { return x + y; };

  int64_t isum[4];
  for (int w = 0; w < 4; ++w) {
    int64_t m = 0;
    for (int b = tid; b < nB; b += FT) m += wi[(size_t)w * B + b];
    isum[w] = fold_tree(shi, m, addi);
  }
  for (int k = 0; k < 32; ++k) {
    int64_t m = 0;
    for (int b = tid; b < nB; b += FT) m += wi[(size_t)(W_HIST + k) * B + b];
    const int64_t h = fold_tree(shi, m, addi);
    if (tid == k) blk->hist[k] += h;
  }
  double dsum[N_F64];
  for (int w = 0; w < N_F64; ++w) {
    double m = 0.0;
    for (int b = tid; b < nB; b += FT) m = m + wd[(size_t)(W_F64 + w) * B + b];
    dsum[w] = fold_tree(shd, m, addd);
  }
  float fmin_ = FLT_MAX, fmax_ = -FLT_MAX;
  int lmin = INT_MAX, lmax = 0;
  for (int b = tid; b < nB; b += FT) {
    const float2 r = reinterpret_cast<const float2*>(ws)[(size_t)W_RET_MM * B + b];
    const int2 l = reinterpret_cast<const int2*>(ws)[(size_t)W_LEN_MM * B + b];
    fmin_ = r.x < fmin_ ? r.x : fmin_; fmax_ = r.y > fmax_ ? r.y : fmax_;
    lmin = l.x < lmin ? l.x : lmin; lmax = l.y > lmax ? l.y : lmax;
  }
  fmin_ = fold_tree(shf, fmin_, [](float x, float y) { return y < x ? y : x; });
  fmax_ = fold_tree(shf, fmax_, [](float x, float y) { return y > x ? y : x; });
  lmin = fold_tree(shn, lmin, [](int x, int y) { return y < x ? y : x; });
  lmax = fold_tree(shn, lmax, [](int x, int y) { return y > x ? y : x; });

  if (tid == 0 && isum[W_EPISODES] > 0) {
    if (blk->episodes == 0) {  // a zeroed block: the extremes are this call's
      blk->ret_min = fmin_; blk->ret_max = fmax_; blk->len_min = lmin; blk->len_max = lmax;
    } else {
      blk->ret_min = fmin_ < blk->ret_min ? fmin_ : blk->ret_min;
      blk->ret_max = fmax_ > blk->ret_max ? fmax_ : blk->ret_max;
      blk->len_min = lmin < blk->len_min ? lmin : blk->len_min;
      blk->len_max = lmax > blk->len_max ? lmax : blk->len_max;
    }
    blk->episodes += isum[W_EPISODES];
    blk->capped += isum[W_CAPPED];
    blk->rows += isum[W_ROWS];
    blk->verr_rows += isum[W_VERR_ROWS];
    blk->ret_sum = blk->ret_sum + dsum[0];
    blk->ret_sq = blk->ret_sq + dsum[1];
    blk->verr_sum = blk->verr_sum + dsum[2];
    blk->verr_abs = blk->verr_abs + dsum[3];
    blk->verr_sq = blk->verr_sq + dsum[4];
    blk->value_sum = blk->value_sum + dsum[5];
    blk->entropy_sum = blk->entropy_sum + dsum[6];
  }
}

}  // namespace

extern "C" {

long long mzba_stream_episode_stats_ws_bytes(int B) {
  return B > 0 ? (long long)W_WORDS * 8 * B : -1;
}

int mzba_stream_episode_stats(const mzba_sink* sink, const uint8_t* done, const int32_t* hlen, int cap_len,
                              int first_n, double gamma, double hist_lo, double hist_step, mzba_episode_stats* block,
                              float* ep_ret, int32_t* ep_len, int ep_n, void* ws, long long ws_bytes,
                              hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && sink->start && sink->mask && sink->reward && sink->values &&
               sink->counts && done && hlen && block && ws, -1);
  MZ_CHECK_ARG(cap_len >= 1 && first_n >= 0 && ep_n >= 0 && hist_step > 0.0 && hist_lo == hist_lo && gamma == gamma,
               -1);
  MZ_CHECK_ARG(ws_bytes >= mzba_stream_episode_stats_ws_bytes(sink->B) && ((uintptr_t)ws & 7) == 0 &&
               ((uintptr_t)block & 7) == 0, -1);
  const StatsArgs a{sink->start, sink->mask, sink->reward, sink->values, sink->counts, done, hlen, sink->T, sink->B,
                    cap_len, first_n, ep_n, gamma, hist_lo, hist_step, ep_ret, ep_len};
  hipLaunchKernelGGL(episode_stats_env_kernel, dim3((sink->B + 255) / 256), dim3(256), 0, stream, a,
                     static_cast<uint64_t*>(ws));
  hipLaunchKernelGGL(episode_stats_fold_kernel, dim3(1), dim3(FT), 0, stream, static_cast<const uint64_t*>(ws),
                     sink->B, block);
  MZ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
