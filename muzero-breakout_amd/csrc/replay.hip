// Replay ingest on the device (replay_buffer.py:96-165).
//
// The acting loop's sink already holds, per step t and env b, the recorded action, reward,
// visit counts, root value and frame (u8 gray code) of every env still live at t (a prefix of
// the episode), plus the episode's first frame g(s0). ReplayBuffer.save_observation_trajectory
// turns each trajectory of length L > K + 1 (train_torch.py:223-225) into L - K + 1 windows:
// 32 past actions, 32 frames (31 padding frames g(s0) + the records, so frames run one behind
// the actions), K future actions / rewards / visit counts / values, the reward sum and K
// n-step value targets with the reference's f32 op order and its discount**K quirk.
//   replay_plan_kernel  (one workgroup): per-env length, reward sum, window counts, exclusive scan;
//   replay_write_kernel (one workgroup per surviving window): writes the window into a FIFO ring
//                        of fixed-size rows (frames stay u8 codes: 10 KB per window at 16x20);
//   replay_states_kernel: gathers a batch of windows' frames as f32 grayscale (the learner's input).
// A streamed sink (several episodes per env) goes through stream_count / stream_scan / stream_fill
// (a flat segment table) and stream_write_kernel, which shares write_window with replay_write_kernel;
// stream_gather_kernel writes a list of the table's windows, given or drawn, for the sink archive.
#include "replay_dev.h"

namespace {

struct ReplayRing {
  int64_t* past_actions;   // [cap][hist]
  int64_t* future_actions; // [cap][K]
  uint8_t* states;         // [cap][hist][HW]
  float* rewards;          // [cap][K]
  float* counts;           // [cap][K][3]
  float* values;           // [cap][K]
  float* targets;          // [cap][K]
  float* reward_sum;       // [cap]
  int cap;
};

constexpr int PT = 1024;

// lengths / reward sums / window offsets of the B trajectories (min_len: trajectories with
// length <= min_len are skipped, train_torch.py:224)
__global__ __launch_bounds__(PT) void replay_plan_kernel(ReplayRecords r, int K, int min_len, int32_t* lens,
                                                         float* rsum, int32_t* offsets) {
  __shared__ int32_t part[PT];
  const int tid = threadIdx.x;
  const int per = (r.B + PT - 1) / PT;
  int mine = 0;
  for (int u = 0; u < per; ++u) {
    const int b = tid * per + u;
    if (b >= r.B) break;
    int L = 0;
    float s = 0.f;
    for (int t = 0; t < r.T; ++t) {  // the recorded steps are a prefix of the episode
      if (r.mask[(size_t)t * r.B + b]) {
        s = s + r.reward[(size_t)t * r.B + b];  // ObservationTrajectory.reward_sum (replay_buffer.py:34)
        ++L;
      }
    }
    lens[b] = L;
    rsum[b] = s;
    mine += L > min_len && L >= K ? L - K + 1 : 0;
  }
  part[tid] = mine;
  __syncthreads();
  for (int o = 1; o < PT; o <<= 1) {  // inclusive scan over the per-thread sums
    const int v = tid >= o ? part[tid - o] : 0;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - mine;
  for (int u = 0; u < per; ++u) {
    const int b = tid * per + u;
    if (b >= r.B) break;
    offsets[b] = run;
    const int L = lens[b];
    run += L > min_len && L >= K ? L - K + 1 : 0;
  }
  if (tid == PT - 1) offsets[r.B] = part[PT - 1];
}

// window s of a trajectory of L records whose first record is sink row t0 of env b -> ring row `slot`;
// frame0_chunk(q) = 16-B chunk q of the trajectory's g(s0). FULL = false (the reanalyse rewrite): only
// the fields a new search changes, counts, values and targets, are written, by the same statements
template <bool FULL = true, typename F0>
MZ_DEV void write_window(const ReplayRecords& r, const ReplayRing& g, int b, int t0, int s, int L, float rsum,
                         size_t slot, int K, int hist, const float* __restrict__ dpow, F0 frame0_chunk) {
  const int tid = threadIdx.x;
  const size_t B = r.B;
  if (tid < hist) {  // actions[s + tid] of the padded list: 32 zeros, then the records
    const int i = s + tid;
    if (FULL) g.past_actions[slot * hist + tid] = i < hist ? 0 : (int64_t)r.action[(size_t)(t0 + i - hist) * B + b];
  } else if (tid < hist + K) {
    const int i = tid - hist, t = t0 + s + i;  // records [s, s + K) (the padded lists' [s + 32, s + 32 + K))
    if (FULL) {
      g.future_actions[slot * K + i] = (int64_t)r.action[(size_t)t * B + b];
      g.rewards[slot * K + i] = r.reward[(size_t)t * B + b];
    }
    g.values[slot * K + i] = r.value[(size_t)t * B + b];
    for (int a = 0; a < 3; ++a) g.counts[(slot * K + i) * 3 + a] = (float)r.counts[((size_t)t * B + b) * 3 + a];
    g.targets[slot * K + i] = nstep_target(r, b, t0, s + i, L, dpow);
  } else if (FULL && tid == hist + K) {
    g.reward_sum[slot] = rsum;
  }
  if (!FULL) return;
  // frames: the padded states list = 31 x g(s0), then the recorded frames
  const int chunks = r.HW / 16;
  uint8_t* dst = g.states + slot * hist * r.HW;
  for (int c = tid; c < hist * chunks; c += 256) {
    const int f = c / chunks, q = c - f * chunks, i = s + f;
    const uint4 v = i < hist - 1 ? frame0_chunk(q)
                                 : *reinterpret_cast<const uint4*>(r.frame + ((size_t)(t0 + i - (hist - 1)) * B + b) * r.HW + q * 16);
    *reinterpret_cast<uint4*>(dst + (size_t)f * r.HW + q * 16) = v;
  }
}

// one workgroup per window j in [j0, n): env by binary search of offsets, ring slot (head + j) % cap
__global__ __launch_bounds__(256) void replay_write_kernel(ReplayRecords r, ReplayRing g, const int32_t* __restrict__ lens,
                                                           const float* __restrict__ rsum,
                                                           const int32_t* __restrict__ offsets, int K, int hist,
                                                           const float* __restrict__ dpow, int head, int j0) {
  const int j = j0 + blockIdx.x;
  int lo = 0, hi = r.B;  // last b with offsets[b] <= j
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= j) lo = mid; else hi = mid;
  }
  const int b = lo;
  const uint8_t* f0 = r.frame0 + (size_t)b * r.HW;
  write_window(r, g, b, 0, j - offsets[b], lens[b], rsum[b], ((size_t)head + j) % g.cap, K, hist, dpow,
               [f0](int q) { return *reinterpret_cast<const uint4*>(f0 + q * 16); });
}

// replay_write_kernel's windows j in [j0, n) again after the sink's counts and values changed: the three fields that
// follow them, nothing else of the slot
__global__ __launch_bounds__(256) void replay_rewrite_kernel(ReplayRecords r, ReplayRing g, const int32_t* __restrict__ lens,
                                                             const float* __restrict__ rsum,
                                                             const int32_t* __restrict__ offsets, int K, int hist,
                                                             const float* __restrict__ dpow, int head, int j0) {
  const int j = j0 + blockIdx.x;
  int lo = 0, hi = r.B;  // last b with offsets[b] <= j
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offsets[mid] <= j) lo = mid; else hi = mid;
  }
  const int b = lo;
  write_window<false>(r, g, b, 0, j - offsets[b], lens[b], rsum[b], ((size_t)head + j) % g.cap, K, hist, dpow,
                      [](int) { return make_uint4(0, 0, 0, 0); });
}

// ---------------------------------------------------------------- streamed sinks (streaming acting)
// A streamed sink holds several episodes per env: a segment is env b's rows from a non-zero start word (common.h) up
// to the row before the next one, or up to T; its records are the masked rows (a prefix). The last segment of an env
// is closed iff done[b] || hlen[b] >= cap_len at the end of the stage; an open one is kept only with keep_tail. Kept
// segments (the length rule of replay_plan_kernel) are ordered by env, then by start row.
struct StreamPlan {
  const uint32_t* start;  // [T][B]
  const uint8_t* done;    // [B] at the end of the stage
  const int32_t* hlen;    // [B]
  int cap_len, keep_tail, K, min_len;
};

// f(t0, L, reward sum, start word) for every kept segment of env b, in row order
template <typename F>
MZ_DEV void for_each_kept_segment(const ReplayRecords& r, const StreamPlan& p, int b, F f) {
  int t0 = -1, L = 0;
  float s = 0.f;
  uint32_t w0 = 0;
  for (int t = 0; t < r.T; ++t) {  // lanes of a wave read consecutive envs of row t
    const size_t i = (size_t)t * r.B + b;
    const uint32_t w = p.start[i];
    if (w) {
      if (t0 >= 0 && L > p.min_len && L >= p.K) f(t0, L, s, w0);
      t0 = t; L = 0; s = 0.f; w0 = w;
    }
    if (t0 >= 0 && r.mask[i]) {
      s = s + r.reward[i];  // ObservationTrajectory.reward_sum (replay_buffer.py:34)
      ++L;
    }
  }
  const bool closed = p.done[b] != 0 || p.hlen[b] >= p.cap_len;
  if (t0 >= 0 && (closed || p.keep_tail) && L > p.min_len && L >= p.K) f(t0, L, s, w0);
}

// one thread per env: cnt[b] = (kept segments, their windows)
__global__ __launch_bounds__(256) void stream_count_kernel(ReplayRecords r, StreamPlan p, int32_t* __restrict__ cnt) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= r.B) return;
  int ns = 0, nw = 0;
  for_each_kept_segment(r, p, b, [&](int, int L, float, uint32_t) { ++ns; nw += L - p.K + 1; });
  cnt[2 * b] = ns; cnt[2 * b + 1] = nw;
}

// one workgroup: offs[b] = exclusive scan of cnt over the envs (both columns), offs[B] = the totals
__global__ __launch_bounds__(PT) void stream_scan_kernel(const int32_t* __restrict__ cnt, int32_t* __restrict__ offs, int B) {
  __shared__ int32_t ps[PT], pw[PT];
  const int tid = threadIdx.x;
  const int per = (B + PT - 1) / PT;
  int ms = 0, mw = 0;
  for (int u = 0; u < per; ++u) {
    const int b = tid * per + u;
    if (b >= B) break;
    ms += cnt[2 * b]; mw += cnt[2 * b + 1];
  }
  ps[tid] = ms; pw[tid] = mw;
  __syncthreads();
  for (int o = 1; o < PT; o <<= 1) {
    const int vs = tid >= o ? ps[tid - o] : 0, vw = tid >= o ? pw[tid - o] : 0;
    __syncthreads();
    ps[tid] += vs; pw[tid] += vw;
    __syncthreads();
  }
  int rs = ps[tid] - ms, rw = pw[tid] - mw;
  for (int u = 0; u < per; ++u) {
    const int b = tid * per + u;
    if (b >= B) break;
    offs[2 * b] = rs; offs[2 * b + 1] = rw;
    rs += cnt[2 * b]; rw += cnt[2 * b + 1];
  }
  if (tid == PT - 1) { offs[2 * B] = ps[PT - 1]; offs[2 * B + 1] = pw[PT - 1]; }
}

// one thread per env: its kept segments into the table from offs[b] on
__global__ __launch_bounds__(256) void stream_fill_kernel(ReplayRecords r, StreamPlan p, const int32_t* __restrict__ offs,
                                                          SegTable tb) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= r.B) return;
  int si = offs[2 * b], wo = offs[2 * b + 1];
  for_each_kept_segment(r, p, b, [&](int t0, int L, float s, uint32_t w0) {
    if (si < tb.nmax) {
      tb.col(0)[si] = b; tb.col(1)[si] = t0; tb.col(2)[si] = L; tb.col(3)[si] = __float_as_int(s);
      tb.col(4)[si] = (int32_t)w0; tb.col(5)[si] = wo;
    }
    ++si; wo += L - p.K + 1;
  });
  if (b == r.B - 1 && si <= tb.nmax) tb.col(5)[si] = wo;
}

// the last segment of woff[0, nseg) with woff[seg] <= j (nseg > 0)
MZ_DEV int segment_of(const int32_t* __restrict__ woff, int nseg, int j) {
  int lo = 0, hi = nseg;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (woff[mid] <= j) lo = mid; else hi = mid;
  }
  return lo;
}

// window j of the table -> ring row `slot`: the body of both streamed writers
template <bool FULL>
MZ_DEV void write_table_window(const ReplayRecords& r, const ReplayRing& g, const SegTable& tb, int nseg, int j,
                               size_t slot, int H, int W, int pw, int brick_rows, int K, int hist,
                               const float* __restrict__ dpow) {
  const int32_t* woff = tb.col(5);
  const int lo = segment_of(woff, nseg, j);
  int paddle, bx, by;
  mz_start_unpack((uint32_t)tb.col(4)[lo], paddle, bx, by);
  write_window<FULL>(r, g, tb.col(0)[lo], tb.col(1)[lo], j - woff[lo], tb.col(2)[lo], __int_as_float(tb.col(3)[lo]),
                     slot, K, hist, dpow,
                     [=](int q) { return mz_s0_chunk(q * 16, H, W, pw, brick_rows, paddle, bx, by); });
}

// one workgroup per window j in [j0, n): segment by binary search of the table's window offsets. FULL = false: the
// same windows again after the sink's counts and values changed (write_window<false>; no frame is rendered)
template <bool FULL>
__global__ __launch_bounds__(256) void stream_write_kernel(ReplayRecords r, ReplayRing g, SegTable tb, int nseg, int H, int W,
                                                           int pw, int brick_rows, int K, int hist,
                                                           const float* __restrict__ dpow, int head, int j0) {
  const int j = j0 + blockIdx.x;
  write_table_window<FULL>(r, g, tb, nseg, j, ((size_t)head + j) % g.cap, H, W, pw, brick_rows, K, hist, dpow);
}

// The archive's draw: Philox (request i, stream 6, step, 0). Streams 0-3 are in common.h, 4 in
// replay_prio.hip, 5 in gumbel.hip.
constexpr int MZ_STREAM_ARCHIVE = 6;

// stream_write_kernel for a list of windows: workgroup i writes window j = idx[i] of the table into ring row
// slot0 + i; without idx, j = (x * N) >> 32 with x the full 32-bit Philox word (N may exceed 2^24). The segment and
// window counts are read from totals = {segments, windows} (stream_plan's offs[B]) on the device, so a captured
// launch follows a table that is planned again. A window outside [0, N), or an empty table, returns before any read
// of the sink or of the table's body and leaves its ring row alone; idx_out (optional) gets j, or -1 for those.
__global__ __launch_bounds__(256) void stream_gather_kernel(ReplayRecords r, ReplayRing g, SegTable tb,
                                                            const int32_t* __restrict__ totals,
                                                            const int32_t* __restrict__ idx, uint64_t seed, uint32_t step,
                                                            const uint32_t* __restrict__ step_dev, int H, int W, int pw,
                                                            int brick_rows, int K, int hist,
                                                            const float* __restrict__ dpow, int slot0,
                                                            int32_t* __restrict__ idx_out) {
  const int i = blockIdx.x;
  const int nseg = totals[0], N = totals[1];
  int j = -1;
  if (idx) {
    j = idx[i];
  } else if (N > 0) {
    if (step_dev) step = step_dev[0];
    j = (int)(((uint64_t)mz_u32((uint32_t)i, MZ_STREAM_ARCHIVE, step, 0, seed) * (uint32_t)N) >> 32);
  }
  const bool ok = nseg > 0 && nseg <= tb.nmax && N > 0 && j >= 0 && j < N;
  if (idx_out && threadIdx.x == 0) idx_out[i] = ok ? j : -1;
  if (!ok) return;
  write_table_window<true>(r, g, tb, nseg, j, (size_t)slot0 + i, H, W, pw, brick_rows, K, hist, dpow);
}

// batch gather of window frames as f32 grayscale: out[n][hist][HW] = lut[code & 7]
__global__ __launch_bounds__(256) void replay_states_kernel(const uint8_t* __restrict__ states, const int32_t* __restrict__ slots,
                                                            const float* __restrict__ lut, float* __restrict__ out,
                                                            int hist, int HW) {
  const int n = blockIdx.x;
  const uint8_t* src = states + (size_t)slots[n] * hist * HW;
  float* dst = out + (size_t)n * hist * HW;
  float l[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) l[i] = lut[i];
  const int c4 = hist * HW / 4;
  for (int c = threadIdx.x; c < c4; c += 256) {
    const uint32_t w = reinterpret_cast<const uint32_t*>(src)[c];
    float4 v = {l[w & 7], l[(w >> 8) & 7], l[(w >> 16) & 7], l[(w >> 24) & 7]};
    reinterpret_cast<float4*>(dst)[c] = v;
  }
}

// the kernels' view of the ABI's ring (include/mzba.h); records() of its sink is in replay_dev.h
ReplayRing ring_view(const mzba_replay_ring& g) {
  return {g.past_actions, g.future_actions, g.states, g.rewards, g.counts, g.values, g.targets, g.reward_sum, g.cap};
}

// what both writers ask of the ring and of the window range
bool ring_ok(const mzba_replay_ring* g, int head, int n_windows) {
  return g && g->K > 0 && g->hist >= 2 && g->hist + g->K < 256 && g->cap > 0 && head >= 0 && head < g->cap &&
         n_windows >= 0 && g->past_actions && g->future_actions && g->states && g->rewards && g->counts && g->values &&
         g->targets && g->reward_sum;
}

}  // namespace

extern "C" {

int mzba_replay_plan(const mzba_sink* sink, const uint8_t* frame0, int K, int min_len, int32_t* lens, float* rsum,
                     int32_t* offsets, hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && sink->HW > 0 && K > 0 && sink->mask && sink->reward && lens &&
               rsum && offsets, -1);
  hipLaunchKernelGGL(replay_plan_kernel, dim3(1), dim3(PT), 0, stream, records(*sink, frame0), K, min_len, lens,
                     rsum, offsets);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_replay_write(const mzba_sink* sink, const uint8_t* frame0, const int32_t* lens, const float* rsum,
                      const int32_t* offsets, int n_windows, const mzba_replay_ring* ring, int head,
                      const float* dpow, hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && sink->HW % 16 == 0 && ring_ok(ring, head, n_windows), -1);
  MZ_CHECK_ARG(dpow && sink->action && sink->reward && sink->counts && sink->values && sink->frame && frame0 && lens &&
               rsum && offsets, -1);
  if (n_windows == 0) return 0;
  const int j0 = n_windows > ring->cap ? n_windows - ring->cap : 0;  // older windows would be evicted at once
  hipLaunchKernelGGL(replay_write_kernel, dim3(n_windows - j0), dim3(256), 0, stream, records(*sink, frame0),
                     ring_view(*ring), lens, rsum, offsets, ring->K, ring->hist, dpow, head, j0);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_replay_rewrite(const mzba_sink* sink, const uint8_t* frame0, const int32_t* lens, const float* rsum,
                        const int32_t* offsets, int n_windows, int j_first, const mzba_replay_ring* ring, int head,
                        const float* dpow, hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && ring_ok(ring, head, n_windows) && j_first >= 0, -1);
  MZ_CHECK_ARG(dpow && sink->reward && sink->counts && sink->values && lens && rsum && offsets, -1);
  int j0 = n_windows > ring->cap ? n_windows - ring->cap : 0;  // the windows the write kept
  if (j_first > j0) j0 = j_first;                              // minus those evicted since
  if (j0 >= n_windows) return 0;
  hipLaunchKernelGGL(replay_rewrite_kernel, dim3(n_windows - j0), dim3(256), 0, stream, records(*sink, frame0),
                     ring_view(*ring), lens, rsum, offsets, ring->K, ring->hist, dpow, head, j0);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_replay_stream_plan(const mzba_sink* sink, const uint8_t* done, const int32_t* hlen, int K, int min_len,
                            int cap_len, int keep_tail, int32_t* cnt, int32_t* offs, int32_t* table, int nmax,
                            hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && K > 0 && sink->reward && sink->mask && sink->start && done &&
               hlen && cnt && offs && table, -1);
  const int B = sink->B;
  // a kept segment holds at least max(min_len + 1, K) of its env's T rows
  const int keep = (min_len + 1 > K ? min_len + 1 : K);
  MZ_CHECK_ARG(nmax >= 0 && (long long)nmax >= (long long)B * (sink->T / keep), -2);
  const ReplayRecords r = records(*sink, nullptr);
  StreamPlan p{sink->start, done, hlen, cap_len, keep_tail, K, min_len};
  SegTable tb{table, nmax};
  const dim3 grid((B + 255) / 256);
  hipLaunchKernelGGL(stream_count_kernel, grid, dim3(256), 0, stream, r, p, cnt);
  hipLaunchKernelGGL(stream_scan_kernel, dim3(1), dim3(PT), 0, stream, cnt, offs, B);
  hipLaunchKernelGGL(stream_fill_kernel, grid, dim3(256), 0, stream, r, p, offs, tb);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_replay_stream_write(const mzba_sink* sink, int H, int W, int paddle_width, int brick_rows,
                             const int32_t* table, int nmax, int n_segments, int n_windows,
                             const mzba_replay_ring* ring, int head, const float* dpow, hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && H > 0 && W > 0 && H <= 256 && W <= 256 && (H * W) % 16 == 0 &&
               sink->HW == H * W && ring_ok(ring, head, n_windows) && n_segments >= 0 && n_segments <= nmax &&
               n_segments <= n_windows, -1);
  MZ_CHECK_ARG(dpow && sink->action && sink->reward && sink->counts && sink->values && sink->frame && table, -1);
  if (n_windows == 0) return 0;
  MZ_CHECK_ARG(n_segments > 0, -1);
  SegTable tb{const_cast<int32_t*>(table), nmax};
  const int j0 = n_windows > ring->cap ? n_windows - ring->cap : 0;  // older windows would be evicted at once
  hipLaunchKernelGGL(stream_write_kernel<true>, dim3(n_windows - j0), dim3(256), 0, stream, records(*sink, nullptr),
                     ring_view(*ring), tb, n_segments, H, W, paddle_width, brick_rows, ring->K, ring->hist, dpow, head,
                     j0);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_replay_stream_gather(const mzba_sink* sink, int H, int W, int paddle_width, int brick_rows,
                              const int32_t* table, int nmax, const int32_t* totals, const int32_t* idx, int n,
                              uint64_t seed, uint32_t step, const uint32_t* step_dev, const mzba_replay_ring* ring,
                              int slot0, const float* dpow, int32_t* idx_out, hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && H > 0 && W > 0 && H <= 256 && W <= 256 && (H * W) % 16 == 0 &&
               sink->HW == H * W && ring_ok(ring, 0, n) && nmax >= 0, -1);
  // rows, and with them windows (a segment of L rows gives at most L), are indexed in 32 bits
  MZ_CHECK_ARG((long long)sink->T * sink->B <= 0x7fffffffLL, -1);
  MZ_CHECK_ARG(slot0 >= 0 && (long long)slot0 + n <= ring->cap, -1);  // row slot0 + i: no modulo
  MZ_CHECK_ARG(dpow && sink->action && sink->reward && sink->counts && sink->values && sink->frame && table && totals,
               -1);
  if (n == 0) return 0;
  SegTable tb{const_cast<int32_t*>(table), nmax};
  hipLaunchKernelGGL(stream_gather_kernel, dim3(n), dim3(256), 0, stream, records(*sink, nullptr), ring_view(*ring), tb,
                     totals, idx, seed, step, step_dev, H, W, paddle_width, brick_rows, ring->K, ring->hist, dpow, slot0,
                     idx_out);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_replay_stream_rewrite(const mzba_sink* sink, const int32_t* table, int nmax, int n_segments, int n_windows,
                               int j_first, const mzba_replay_ring* ring, int head, const float* dpow,
                               hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && ring_ok(ring, head, n_windows) && j_first >= 0 &&
               n_segments >= 0 && n_segments <= nmax && n_segments <= n_windows, -1);
  MZ_CHECK_ARG(dpow && sink->reward && sink->counts && sink->values && table, -1);
  int j0 = n_windows > ring->cap ? n_windows - ring->cap : 0;  // the windows the write kept
  if (j_first > j0) j0 = j_first;                              // minus those evicted since
  if (j0 >= n_windows) return 0;
  MZ_CHECK_ARG(n_segments > 0, -1);
  SegTable tb{const_cast<int32_t*>(table), nmax};
  hipLaunchKernelGGL(stream_write_kernel<false>, dim3(n_windows - j0), dim3(256), 0, stream, records(*sink, nullptr),
                     ring_view(*ring), tb, n_segments, 0, 0, 0, 0, ring->K, ring->hist, dpow, head, j0);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_replay_states(const uint8_t* states, const int32_t* slots, int n, const float* lut8, float* out, int hist,
                       int HW, hipStream_t stream) {
  MZ_CHECK_ARG(states && lut8 && n >= 0 && hist > 0 && (hist * HW) % 4 == 0, -1);
  if (n == 0) return 0;  // an empty batch: its slots and out tensors have no storage, so no pointers
  MZ_CHECK_ARG(slots && out, -1);
  hipLaunchKernelGGL(replay_states_kernel, dim3(n), dim3(256), 0, stream, states, slots, lut8, out, hist, HW);
  MZ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
