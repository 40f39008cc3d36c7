// The sink's records, the streamed plan's segment table, the n-step target and the row <-> window lookup, shared by the
// replay writers (replay.hip) and the archive's priorities (archive_prio.hip). Every f32 expression is evaluated op by
// op in the reference's order (-ffp-contract=off); see replay.hip.
#pragma once
#include "common.h"

namespace {

struct ReplayRecords {
  const uint8_t* action;   // [T][B]
  const float* reward;     // [T][B]
  const uint8_t* mask;     // [T][B] recorded (not prev_done)
  const int64_t* counts;   // [T][B][3]
  const float* value;      // [T][B]
  const uint8_t* frame;    // [T][B][HW]
  const uint8_t* frame0;   // [B][HW]
  int T, B, HW;
};

// host: the kernels' view of the ABI's sink (include/mzba.h)
inline ReplayRecords records(const mzba_sink& s, const uint8_t* frame0) {
  return {s.action, s.reward, s.mask, s.counts, s.values, s.frame, frame0, s.T, s.B, s.HW};
}

// the flat segment table, six columns of nmax + 1 words: env, start row, length, reward sum (f32 bits), start word,
// window offset (exclusive scan over the kept segments; entry [number of segments] = the number of windows)
struct SegTable {
  int32_t* w; int nmax;
  MZ_DEV int32_t* col(int k) const { return w + (size_t)k * (nmax + 1); }
};

// n-step target (replay_buffer.py:137-151) of record `cur` of a trajectory of L records whose first record is sink row
// t0 of env b: bootstrap td_steps = 10 ahead, scaled by discount**K; dpow[k] = f32(discount**k) (python double pow,
// host table), dpow[T + 1] = f32(discount**K)
MZ_DEV float nstep_target(const ReplayRecords& r, int b, int t0, int cur, int L, const float* __restrict__ dpow) {
  const size_t B = r.B;
  const int boot = cur + 10;
  float v;
  if (boot < L) {
    v = r.value[(size_t)(t0 + boot) * B + b] * dpow[r.T + 1];
    for (int k = 0; k < boot - cur; ++k) v = v + dpow[k] * r.reward[(size_t)(t0 + cur + k) * B + b];
  } else {
    v = dpow[0] * r.reward[(size_t)(t0 + cur) * B + b];  // python 0.0 + the first term is that term
    for (int k = 1; k < L - cur; ++k) v = v + dpow[k] * r.reward[(size_t)(t0 + cur + k) * B + b];
  }
  return v;
}

// Sink row i = t * B + b -> the window whose root record it is, or -1. Env b's kept segments are
// the table entries [offs[2 b], offs[2 b + 2]) (stream_plan's exclusive scan), ordered by start row: the last one with
// start row t0 <= t, s = t - t0, a root iff s <= L - K, window woff[seg] + s; `seg` gets that segment. A row outside
// [0, n_rows), nseg = totals[0] outside [1, nmax] and an empty or out-of-table range return before any read of the
// table's body.
MZ_DEV int row_window(const SegTable& tb, const int32_t* __restrict__ offs, const int32_t* __restrict__ totals, int B,
                      int K, int n_rows, int i, int& seg) {
  seg = -1;
  if (i < 0 || i >= n_rows) return -1;
  const int nseg = totals[0];
  if (nseg <= 0 || nseg > tb.nmax) return -1;
  const int t = i / B, b = i - t * B;
  int lo = offs[2 * b], hi = offs[2 * b + 2];
  if (lo < 0 || hi > nseg || lo >= hi) return -1;
  const int32_t* t0s = tb.col(1);
  if (t0s[lo] > t) return -1;
  while (hi - lo > 1) {  // last segment of [lo, hi) with t0 <= t
    const int mid = (lo + hi) >> 1;
    if (t0s[mid] <= t) lo = mid; else hi = mid;
  }
  const int s = t - t0s[lo];
  if (s > tb.col(2)[lo] - K) return -1;
  seg = lo;
  return tb.col(5)[lo] + s;
}

}  // namespace
