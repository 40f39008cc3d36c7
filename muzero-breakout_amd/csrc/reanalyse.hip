// Reanalyse: re-search the rows of a recorded trajectory sink with the current net.
//
// The acting loop builds the representation input of step t from the env's history ring (env.hip,
// build_rep_input_kernel). The ring is gone once the episode ends, but the sink keeps every step's action and
// frame, and an env recorded at row t was recorded at every row before it (mask is a prefix), so the ring's
// content at step t is a function of the sink's rows < t and g(s0):
//   F = (L - 1) x g(s0), then the frames of rows 0 .. t - 1;  A = L x pad_action, then the actions of rows 0 .. t - 1
//   channels 0 .. L - 2 : the last L - 1 entries of F       (source row t + c - (L - 1), g(s0) when negative)
//   channel  L - 1      : the current frame = row t - 1's   (g(s0) at t = 0; the newest frame appears twice)
//   channels L .. 2L - 1: the last L entries of A, a / 3 in f32 (source row t + c - 2L, pad_action when negative)
//   channels 2L .. Cs-1 : zero
//   sink_rep_input_kernel    the gather: NHWC [B][HW][Cs] f32 / bf16, the layout of mzba_build_rep_input;
//   record_masked_kernel     mzba_record_results for the envs recorded at row t only.
// A streamed sink holds several episodes per env, and the restart kernel refills the ring with pad
// actions and g(s0), so the history of env b at row t stops at t0 = the greatest row <= t with a start word: the same
// F and A with "rows t0 .. t - 1" and the g(s0) of that word; a source row r comes from the sink iff r >= t0. The
// kernel's Older parameter says where the older ones come from (FromFrame0: row 0 and a stored g(s0); FromOrigin: t0
// from a (T, B) origin table filled once per sink, sink_origin_kernel, and g(s0) rendered from the word at that row).
#include "common.h"

namespace {

constexpr int RUN = 128;  // pixels of one env per workgroup: every source row's run is one 128-B line's worth

// convert_to_grayscale (train_torch.py:334-358) of gray code i (bit0 paddle, bit1 ball, bit2 brick): the arithmetic of
// build_rep_input_kernel's table (env.hip); constant-folded, the table lives in immediates
MZ_DEV constexpr float gray_value(int i) {
  const float pv = (i & 1) ? 1.f : 0.f, bv = (i & 2) ? 1.f : 0.f, kv = (i & 4) ? 1.f : 0.f;
  const float v = (pv * 0.3f + bv * 1.0f) + kv * 0.6f;
  return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}

// four gray codes (one per byte of `codes`) -> their four values in T, 16 / 8 bytes
template <typename T> struct Gray4;
// f32: a select tree per code
template <> struct Gray4<float> {
  static MZ_DEV void convert(uint32_t codes, uint32_t* w) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t c = codes >> (8 * k);
      const float lo = (c & 2) ? ((c & 1) ? gray_value(3) : gray_value(2)) : ((c & 1) ? gray_value(1) : gray_value(0));
      const float hi = (c & 2) ? ((c & 1) ? gray_value(7) : gray_value(6)) : ((c & 1) ? gray_value(5) : gray_value(4));
      w[k] = __float_as_uint((c & 4) ? hi : lo);
    }
  }
};
// bf16: the table's 8 low bytes and 8 high bytes are the two 8-byte sources of a byte permute whose selector is the
// four codes themselves (v_perm_b32: selector k takes byte k of {S0, S1}, S1 the low dword); two more interleave the
// low and high bytes. Four instructions and a mask for four values.
template <> struct Gray4<bf16_t> {
  static MZ_DEV void convert(uint32_t codes, uint32_t* w) {
    uint32_t lo[2] = {0, 0}, hi[2] = {0, 0};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t h = f32_to_bf16(gray_value(i));
      lo[i >> 2] |= (h & 0xffu) << (8 * (i & 3));
      hi[i >> 2] |= (h >> 8) << (8 * (i & 3));
    }
    const uint32_t sel = codes & 0x07070707u;
    const uint32_t l4 = __builtin_amdgcn_perm(lo[1], lo[0], sel), h4 = __builtin_amdgcn_perm(hi[1], hi[0], sel);
    w[0] = __builtin_amdgcn_perm(h4, l4, 0x05010400u);
    w[1] = __builtin_amdgcn_perm(h4, l4, 0x07030602u);
  }
};

// byte (pixel px of the run, channel c) of the LDS image: S bytes per pixel (S % 8 == 0), 8 bytes of padding per 16
// pixels so that the 8 lanes that hold one source row's 16-pixel chunks write 8 different banks
MZ_DEV int img_at(int px, int c, int S) { return px * S + (px >> 4) * 8 + c; }

// i / d for i d < 2^32 with inv = 0xffffffff / d + 1 (d >= 2; d == 1 has no such inv)
MZ_DEV int div_by(int i, int d, uint32_t inv) { return d == 1 ? i : (int)__umulhi((uint32_t)i, inv); }

// where a source row older than the env's episode comes from
struct FromFrame0 {  // a lockstep sink: the episode starts at row 0, its g(s0) is stored as u8 [B][HW]
  static constexpr bool streamed = false;
  const uint8_t* frame0;
};
struct FromOrigin {  // a streamed sink: the episode starts at row origin[t][b] (sink_origin_kernel), whose start word
  static constexpr bool streamed = true;  // (u32 [T][B]) renders g(s0)
  const uint32_t* start;
  const int32_t* origin;
  int H, W, pw, brick_rows;
};

// One workgroup = one run of up to RUN pixels of env b. Streamed sinks only: t0 and its start word, one word each, the
// same for the whole workgroup. Phase 1: the L source rows' runs, 16 B per lane (rendered from the start word for a
// row < t0), scattered into an LDS image [pixel][channel] of gray codes; the Cs - L channels that do not depend on the
// pixel (action planes, zero padding) once, in the output's element type. Phase 2, 16-B chunks of the NHWC output:
// first the FC chunks per pixel that hold frame channels (a lane reads its chunk's codes with one LDS read, 8 channels
// of one pixel in bf16, 4 in f32, and converts them), then the Cs / EPT - FC chunks per pixel that are the plane values
// as they stand. Whole waves take one kind or the other, and consecutive lanes store consecutive chunks of a pixel.
template <typename T, typename Older>
__global__ __launch_bounds__(256) void sink_rep_input_kernel(
    const uint8_t* __restrict__ action, const uint8_t* __restrict__ frame, const Older older,
    T* __restrict__ out, int rows, int B, int HW, int L, int S, int pad_action, int t_arg,
    const int32_t* __restrict__ ctx, int Cs, int runs, uint32_t inv_fc, uint32_t inv_pc) {
  constexpr int EPT = 16 / (int)sizeof(T);  // elements of a 16-B chunk
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int t = ctx ? ctx[2] : t_arg;
  if (t < 0 || t >= rows) return;  // a device row outside the sink: nothing is read, nothing written
  const int tid = threadIdx.x;
  const int b = blockIdx.x / runs, p0 = (blockIdx.x - b * runs) * RUN;
  const int npix = min(RUN, HW - p0), nch = npix >> 4;
  T* const plane = reinterpret_cast<T*>(lds);                       // [Cs], channels < L unused (zero)
  uint8_t* const img = lds + (size_t)Cs * sizeof(T);                // Cs % 8 == 0: 16-B aligned
  int t0 = 0, paddle = 0, bx = 0, by = 0;  // source rows < t0 are pad actions and g(s0)
  if constexpr (Older::streamed) {  // two uniform loads, no LDS and no barrier
    t0 = min(max(older.origin[(size_t)t * B + b], 0), t);  // whatever the table holds, a row of the sink
    mz_start_unpack(older.start[(size_t)t0 * B + b], paddle, bx, by);
  }
  for (int c = tid; c < Cs; c += 256) {
    float v = 0.f;
    if (c >= L && c < 2 * L) {
      const int r = t + c - 2 * L;
      const int a = r < t0 ? pad_action : (int)action[(size_t)r * B + b];
      v = (float)a / 3.0f;
    }
    st(plane + c, v);
  }
  const uint32_t inv_nch = 0xffffffffu / (uint32_t)nch + 1u;
  for (int i = tid; i < L * nch; i += 256) {
    const int c = div_by(i, nch, inv_nch), q = i - c * nch;
    const int r = c < L - 1 ? t + c - (L - 1) : t - 1;  // r <= t - 1 < rows
    uint4 v;
    if constexpr (Older::streamed) {
      v = r < t0 ? mz_s0_chunk(p0 + q * 16, older.H, older.W, older.pw, older.brick_rows, paddle, bx, by)
                 : *reinterpret_cast<const uint4*>(frame + ((size_t)r * B + b) * HW + p0 + q * 16);
    } else {
      const uint8_t* src = r < 0 ? older.frame0 + (size_t)b * HW : frame + ((size_t)r * B + b) * HW;
      v = *reinterpret_cast<const uint4*>(src + p0 + q * 16);
    }
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) img[img_at(q * 16 + k, c, S)] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  }
  __syncthreads();
  const int FC = (L + EPT - 1) / EPT, PC = Cs / EPT - FC;
  T* const obase = out + ((size_t)b * HW + p0) * Cs;
  union Chunk { uint4 q; uint32_t w[4]; T e[EPT]; };
  for (int j = tid; j < npix * FC; j += 256) {
    const int px = div_by(j, FC, inv_fc), c0 = (j - px * FC) * EPT;
    Chunk o;  // S >= the next multiple of 8 above L: the reads stay inside the pixel's S bytes
    Gray4<T>::convert(*reinterpret_cast<const uint32_t*>(img + img_at(px, c0, S)), o.w);
    if constexpr (EPT == 8) Gray4<T>::convert(*reinterpret_cast<const uint32_t*>(img + img_at(px, c0 + 4, S)), o.w + 2);
    if (c0 + EPT > L) {  // L % EPT != 0: the last frame chunk's tail holds the first action planes
      Chunk pl;
      pl.q = *reinterpret_cast<const uint4*>(plane + c0);
#pragma unroll
      for (int e = 0; e < EPT; ++e)
        if (c0 + e >= L) o.e[e] = pl.e[e];
    }
    *reinterpret_cast<uint4*>(obase + (size_t)px * Cs + c0) = o.q;
  }
  for (int j = tid; j < npix * PC; j += 256) {
    const int px = div_by(j, PC, inv_pc), c0 = (FC + j - px * PC) * EPT;
    *reinterpret_cast<uint4*>(obase + (size_t)px * Cs + c0) = *reinterpret_cast<const uint4*>(plane + c0);
  }
}

// origin[t][b] = the greatest row r <= t with a start word of env b (0 when there is none); one thread per
// env walks its column, lanes of a wave read consecutive envs of a row
__global__ __launch_bounds__(256) void sink_origin_kernel(const uint32_t* __restrict__ start, int32_t* __restrict__ origin,
                                                          int rows, int B) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  int t0 = 0;
  for (int t = 0; t < rows; ++t) {
    if (start[(size_t)t * B + b]) t0 = t;
    origin[(size_t)t * B + b] = t0;
  }
}

// record_results_kernel (mcts.hip) for the envs recorded at row t; the other rows keep what the acting loop left
__global__ void record_masked_kernel(const int64_t* __restrict__ counts, const float* __restrict__ values,
                                     const uint8_t* __restrict__ mask, int64_t* __restrict__ rec_counts,
                                     float* __restrict__ rec_values, int rows, int B, int t_arg,
                                     const int32_t* __restrict__ ctx) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const long long t = ctx ? ctx[2] : t_arg;
  if (t < 0 || t >= rows || !mask[t * B + b]) return;
  rec_counts[(t * B + b) * 3 + 0] = counts[b * 3 + 0];
  rec_counts[(t * B + b) * 3 + 1] = counts[b * 3 + 1];
  rec_counts[(t * B + b) * 3 + 2] = counts[b * 3 + 2];
  rec_values[t * B + b] = values[b];
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the checks and the launch both gathers share
template <typename Older>
int launch_sink_rep_input(const mzba_sink& sink, Older older, int L, int pad_action, int t, const int32_t* ctx, void* out,
                          int out_bf16, int Cs, hipStream_t stream) {
  MZ_CHECK_ARG(sink.T > 0 && sink.B > 0 && sink.HW > 0 && sink.HW % 16 == 0 && sink.action && sink.frame && out, -1);
  MZ_CHECK_ARG(L >= 2 && Cs >= 2 * L && Cs % 8 == 0 && pad_action >= 0 && pad_action < 3, -1);
  MZ_CHECK_ARG(ctx || (t >= 0 && t < sink.T), -1);
  MZ_CHECK_ARG(aligned16(sink.frame) && aligned16(out), -1);  // 16-B loads and stores
  const int S = (L + 7) / 8 * 8;
  const size_t lds = (size_t)Cs * (out_bf16 ? 2 : 4) + (size_t)RUN * S + RUN / 16 * 8;
  const int runs = (sink.HW + RUN - 1) / RUN;
  const int ept = out_bf16 ? 8 : 4, FC = (L + ept - 1) / ept, PC = Cs / ept - FC;  // div_by's reciprocals
  const uint32_t inv_fc = FC > 1 ? 0xffffffffu / (uint32_t)FC + 1u : 0u, inv_pc = PC > 1 ? 0xffffffffu / (uint32_t)PC + 1u : 0u;
  MZ_CHECK_ARG(lds <= 64 * 1024 && (long long)sink.B * runs < (1LL << 31), -1);
  const dim3 grid((unsigned)(sink.B * runs));
  if (out_bf16)
    hipLaunchKernelGGL((sink_rep_input_kernel<bf16_t, Older>), grid, dim3(256), lds, stream, sink.action, sink.frame,
                       older, (bf16_t*)out, sink.T, sink.B, sink.HW, L, S, pad_action, t, ctx, Cs, runs, inv_fc, inv_pc);
  else
    hipLaunchKernelGGL((sink_rep_input_kernel<float, Older>), grid, dim3(256), lds, stream, sink.action, sink.frame,
                       older, (float*)out, sink.T, sink.B, sink.HW, L, S, pad_action, t, ctx, Cs, runs, inv_fc, inv_pc);
  MZ_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" {

int mzba_sink_rep_input(const mzba_sink* sink, const uint8_t* frame0, int L, int pad_action, int t,
                        const int32_t* ctx, void* out, int out_bf16, int Cs, hipStream_t stream) {
  MZ_CHECK_ARG(sink && frame0 && aligned16(frame0), -1);
  return launch_sink_rep_input(*sink, FromFrame0{frame0}, L, pad_action, t, ctx, out, out_bf16, Cs, stream);
}

int mzba_sink_origin(const mzba_sink* sink, int32_t* origin, hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->T > 0 && sink->B > 0 && sink->start && origin, -1);
  hipLaunchKernelGGL(sink_origin_kernel, dim3((sink->B + 255) / 256), dim3(256), 0, stream, sink->start, origin, sink->T,
                     sink->B);
  MZ_LAUNCH_CHECK();
  return 0;
}

int mzba_sink_rep_input_stream(const mzba_sink* sink, const int32_t* origin, int H, int W, int paddle_width,
                               int brick_rows, int L, int pad_action, int t, const int32_t* ctx, void* out, int out_bf16,
                               int Cs, hipStream_t stream) {
  MZ_CHECK_ARG(sink && sink->start && origin && H > 0 && W > 0 && H <= 256 && W <= 256 && H * W == sink->HW, -1);
  MZ_CHECK_ARG(paddle_width > 0 && paddle_width <= W && brick_rows > 0 && brick_rows <= H, -1);
  return launch_sink_rep_input(*sink, FromOrigin{sink->start, origin, H, W, paddle_width, brick_rows}, L, pad_action, t,
                               ctx, out, out_bf16, Cs, stream);
}

int mzba_record_results_masked(const int64_t* counts, const float* values, const mzba_sink* rec, int t,
                               const int32_t* ctx, hipStream_t stream) {
  MZ_CHECK_ARG(counts && values && rec && rec->T > 0 && rec->B > 0 && rec->mask && rec->counts && rec->values, -1);
  MZ_CHECK_ARG(ctx || (t >= 0 && t < rec->T), -1);
  hipLaunchKernelGGL(record_masked_kernel, dim3((rec->B + 255) / 256), dim3(256), 0, stream, counts, values, rec->mask,
                     rec->counts, rec->values, rec->T, rec->B, t, ctx);
  MZ_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
