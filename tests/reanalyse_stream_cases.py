"""Shared cases of the streamed reanalyse tests (tests/test_cpu_reanalyse_stream.py shows them against the streaming
oracle loop without a GPU; tests/test_gpu_reanalyse_stream.py compares the device gather with them). Plain numpy on
top of stream_cases; nothing here calls the library.

* `stream_rep_input`: the representation input of row t of a streamed sink, as DESIGN.md §17 defines it.
* `gather_spec` / `lockstep_like_spec`: synthetic sinks (stream_cases.make_stream_sink) whose segment lengths sit on
  both sides of the history length.
"""
import numpy as np

import stream_cases as SC

LUT = SC.gray_lut()


def origin(start, t, b):
    """t0(t, b): the greatest row r <= t with a start word of env b."""
    rows = np.flatnonzero(start[:t + 1, b])
    assert len(rows), f"env {b} has no start word at or before row {t}"
    return int(rows[-1])


def stream_rep_input(rec, t, b, L, H, W, pad_action=0, pw=SC.PW, brick_rows=SC.BRICK_ROWS):
    """rec: host sink with "start" u32 (T, B), "frame" u8 codes (T, B, H*W), "action" (T, B) -> f32 [2L][H][W]:
    F = (L - 1) x g(s0), then the frames of rows t0 .. t - 1; A = L x pad_action, then their actions; channels
    0 .. L - 2 = the last L - 1 of F, channel L - 1 = row t - 1's frame (g(s0) at t = t0), channels L .. 2L - 1 = the
    last L of A as f32(a) / 3."""
    t0 = origin(rec["start"], t, b)
    g0 = LUT[SC.render_s0(*SC.unpack_start(rec["start"][t0, b]), H, W, pw, brick_rows)]
    F = [g0] * (L - 1) + [LUT[rec["frame"][r, b] & 7] for r in range(t0, t)]
    A = [pad_action] * L + [int(rec["action"][r, b]) for r in range(t0, t)]
    x = np.empty((2 * L, H * W), np.float32)
    x[:L - 1] = F[-(L - 1):]
    x[L - 1] = F[-1] if t > t0 else g0
    x[L:] = (np.array(A[-L:], np.int64).astype(np.float32) / np.float32(3))[:, None]
    return x.reshape(2 * L, H, W)


def ages(start):
    """t - t0(t, b) for every (t, b) of a sink whose row 0 carries a word for every env."""
    T, B = start.shape
    out = np.zeros((T, B), np.int64)
    for b in range(B):
        for t in range(T):
            out[t, b] = t - origin(start, t, b)
    return out


def gather_spec(B, T, L, seed):
    """Per env: segments of lengths drawn from {1, L - 1, L, L + 1, 2L + 3} (extent == length, so every tiled row is
    recorded) until T is full, the rest filled with length-1 segments: every row carries a start word or follows
    one. Env 0 opens with two length-1 segments (a start word at t and at t - 1) and then takes L + 1, L, L - 1 and
    2L + 3 as far as they fit into T; env 1 opens with 2L + 3."""
    g = np.random.default_rng(seed)
    pool = [1, L - 1, L, L + 1, 2 * L + 3]
    opening = {0: [1, 1, L + 1, L, L - 1, 2 * L + 3], 1: [2 * L + 3, 1, L - 1]}
    spec = []
    for b in range(B):
        lens, t = [], 0
        for n in opening.get(b, []):
            if t + n <= T:
                lens.append(n)
                t += n
        while t < T:
            n = int(g.choice(pool))
            n = n if t + n <= T else 1
            lens.append(n)
            t += n
        spec.append(([(n, n) for n in lens], True))
    return spec


def lockstep_like_spec(B, T):
    """One segment per env from row 0 over all T rows."""
    return [([(T, T)], True) for _ in range(B)]


def make_gather_sink(spec, T, H, W, seed):
    """stream_cases.make_stream_sink with its synthetic episode cap lifted for the call: the gather knows no cap, and
    its segments must outgrow the history (2L + 3 records at L = 32). -> the host sink alone."""
    cap = SC.CAP_SYN
    SC.CAP_SYN = T + 1
    try:
        return SC.make_stream_sink(spec, T, H, W, seed)[0]
    finally:
        SC.CAP_SYN = cap
