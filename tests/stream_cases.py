"""Shared cases of the streaming acting tests (tests/test_gpu_stream.py, tests/test_gpu_stream_ingest.py, and
tests/test_cpu_stream_cases.py, which shows without a GPU that the cases are not vacuous). Plain numpy plus the oracle
modules; nothing here calls the library.

* `render_s0`: g(s0) as u8 gray codes from (paddle, bx, by), and `start_word` / `unpack_start` (include/mzba.h).
* `stream_oracle`: the streaming acting loop composed from the oracle's env, trajectory, rep-input, nets and search: at
  the head of step t > 0 an env that is done, or holds `cap` records, is overwritten with `reset(reset_params(seed,
  ep_base + t))` and gets a fresh Trajectory; everything else is oracle.acting.run_episode's step.
* `make_stream_sink`: synthetic streamed sinks in the device layouts, poisoned outside the recorded rows.
"""
import numpy as np

from oracle import rng as R
from oracle.acting import Trajectory, prepare_mcts_input, sample_actions
from oracle.env import BreakoutEnvOracle, convert_to_grayscale
from mzba.config import default_config
from mzba.env import gray_lut

CFG = default_config()
K, HIST, DISCOUNT = CFG["num_unroll_steps"], CFG["model"]["state_history_length"], CFG["discount_factor"]
FLAG = 0x80000000
PW, BRICK_ROWS = 6, 3

# the acted stage of the GPU tests (small f32 nets, S = 20)
STAGE_B, STAGE_T, STAGE_SEED, STAGE_S, STAGE_SD_SEED = 8, 64, 2024, 20, 5
STAGE_CAP_SHORT = 12


def start_word(paddle, bx, by):
    return np.uint32(FLAG | int(paddle) | (int(bx) << 10) | (int(by) << 20))


def unpack_start(w):
    w = int(w)
    return w & 1023, (w >> 10) & 1023, (w >> 20) & 1023


def render_s0(paddle, bx, by, H=16, W=20, pw=PW, brick_rows=BRICK_ROWS):
    """u8 gray codes [H*W] (bit0 paddle, bit1 ball, bit2 brick) of the state reset() builds."""
    f = np.zeros((H, W), np.uint8)
    f[:brick_rows, :] |= 4
    f[H - 1, paddle:paddle + pw] |= 1
    f[by, bx] |= 2
    return f.reshape(-1)


def s0_of_params(params, b, H=16, W=20, pw=PW):
    """(paddle, bx, by) of env b's s0 under reset params (off, col, row, dx) (parallel_breakout.py:120-128)."""
    off, col, row, _ = params
    return int(W // 2 - pw // 2 + off[b]), int(col[b]), int(row[b] % H)


def codes_of_gray(g):
    """grayscale f32 frame -> the lowest u8 code with that value (frames of s0 and of steps hold codes 0, 1, 2, 4)."""
    lut = gray_lut()
    out = np.zeros(g.shape, np.uint8)
    for c in (4, 2, 1):
        out[g == lut[c]] = c
    assert np.array_equal(lut[out], g)
    return out


def make_env(B, H=16, W=20):
    env = BreakoutEnvOracle({**CFG["environment"], "n_parallel": B})
    env.height, env.width = H, W
    return env


def restart_envs(env, state, done, which, params):
    """Overwrite the envs `which` (bool [B]) with reset(params); the others keep state, ball_dx and ball_dy."""
    dx, dy = env.ball_dx.copy(), env.ball_dy.copy()
    fresh, _ = env.reset(params)
    state = state.copy()
    state[which] = fresh[which]
    env.ball_dx = np.where(which, env.ball_dx, dx)
    env.ball_dy = np.where(which, env.ball_dy, dy).astype(np.float32)
    done = done & ~which
    return state, done


def stream_oracle(cfg, seed, ep_base, T, B, act_fn, cap=261, H=16, W=20, params_fn=None):
    """T streamed rows. act_fn(t, x) -> (action i64 [B], counts [B][3], values f32 [B]) with x [B][2L][H][W] the
    rep inputs (built lazily: x() returns them). params_fn(key) replaces the keyed reset draws.
    -> dict of sink-layout arrays (action, reward, mask, counts, values, frame as grayscale f32, start u32),
    done / hlen at the end, and `episodes`: per env [(start_row, key)]."""
    L = cfg["model"]["state_history_length"]
    env = make_env(B, H, W)
    pf = params_fn or (lambda key: env.reset_params(seed, key))
    p0 = pf(ep_base)
    state, _ = env.reset(p0)
    g0 = convert_to_grayscale(state)
    trajs = [Trajectory(L, g0[b]) for b in range(B)]
    done = np.zeros(B, dtype=bool)
    warp = g0
    out = {"action": np.zeros((T, B), np.uint8), "reward": np.zeros((T, B), np.float32),
           "mask": np.zeros((T, B), np.uint8), "counts": np.zeros((T, B, 3), np.int64),
           "values": np.zeros((T, B), np.float32), "frame": np.zeros((T, B, H, W), np.float32),
           "start": np.zeros((T, B), np.uint32)}
    episodes = [[(0, ep_base)] for _ in range(B)]
    for b in range(B):
        out["start"][0, b] = start_word(*s0_of_params(p0, b, H, W))
    for t in range(T):
        if t > 0:
            which = done | (np.array([tr.length for tr in trajs]) >= cap)
            if which.any():
                p = pf(ep_base + t)
                state, done = restart_envs(env, state, done, which, p)
                warp = convert_to_grayscale(state)
                for b in np.flatnonzero(which):
                    trajs[b] = Trajectory(L, warp[b])
                    episodes[b].append((t, ep_base + t))
                    out["start"][t, b] = start_word(*s0_of_params(p, b, H, W))
        prev_done = done.copy()
        x = lambda: np.stack([prepare_mcts_input(warp[b], trajs[b], L) for b in range(B)])  # noqa: E731
        action, counts, values = act_fn(t, x)
        state, reward, done, _ = env.step(state, action, done)
        warp = convert_to_grayscale(state)
        rec = ~done if t == 0 else ~prev_done  # train_torch.py:179: at the first step prev_done aliases done
        for b in range(B):
            if rec[b]:
                trajs[b].add_observation(action[b], warp[b], reward[b], counts[b], values[b])
        out["action"][t], out["reward"][t], out["mask"][t] = action, reward, rec
        out["counts"][t], out["values"][t], out["frame"][t] = counts, values, warp[:, 0]
    hlen = np.array([tr.length for tr in trajs], np.int32)
    return out, done.copy(), hlen, episodes


def random_act_fn(seed, B):
    """Uniformly random actions, no nets (the issue's CPU measurement)."""
    g = np.random.default_rng(seed)

    def act(t, x):
        return g.integers(0, 3, B), np.zeros((B, 3), np.int64), np.zeros(B, np.float32)
    return act


def searched_act_fn(cfg, sd, seed, B, noise_fn, temperature=1.0, search_id0=0, step0=0):
    """oracle.acting.run_episode's representation -> search -> sampling for step t."""
    from oracle import nets as N
    from oracle.mcts import MCTSOracle, NetModel
    mcfg = cfg["model"]
    search = MCTSOracle(cfg, NetModel(sd, mcfg), seed)

    def act(t, x):
        h = N.create_hidden_state_root(x(), sd, mcfg)
        sid = search_id0 + t
        values, counts = search.search(h, noise_fn(sid, B), sid, 0)
        u = R.uniform(np.arange(B), R.STREAM_SAMPLE, step0 + t, 0, seed)
        return sample_actions(counts, temperature, u), counts, values
    return act


def dirichlet_noise_fn(seed):
    """A root-noise source of the tests' own (the CPU conditions; the GPU tests replay the device's draws)."""
    def fn(sid, B):
        return np.random.default_rng([seed, sid]).dirichlet([0.3] * 3, B).astype(np.float32)
    return fn


def segments_of(start, T, done, hlen, cap):
    """[(env, t0, t1, closed)] by env, then start row."""
    out = []
    for b in range(start.shape[1]):
        rows = np.flatnonzero(start[:T, b])
        for i, t0 in enumerate(rows):
            last = i + 1 == len(rows)
            out.append((b, int(t0), T if last else int(rows[i + 1]), bool(done[b] or hlen[b] >= cap) if last else True))
    return out


# ---------------------------------------------------------------------- synthetic streamed sinks
REWARDS = np.array([-1, 0, 0, 1, 5, 6, 0.3], np.float32)
SEG_POOL = np.array([1, 3, K, K + 1, K + 2, 8, 9, 10, 11, 12, 14, 15, 16, 17, 21, 24])
CAP_SYN = 24  # the synthetic stages' episode cap: a last segment shorter than this is closed only through `done`


def make_stream_sink(spec, T, H=16, W=20, seed=0):
    """spec[b] = ([(L, extent), ...], closed): env b's segments in row order, each `extent` >= L rows of which the
    first L are recorded (a streamed stage has extent == L; a lockstep sink one segment from row 0 with the rows
    after its L records unmasked), and whether the last one is closed. Rows outside the records are poison (NaN
    reward and value, action 255, counts -1, frame code 7); rows past the last extent carry no start word.
    -> (rec dict of host arrays incl. "start" u32, done u8 [B], hlen i32 [B])."""
    g = np.random.default_rng(seed)
    B, HW = len(spec), H * W
    live = np.zeros((T, B), bool)
    start = np.zeros((T, B), np.uint32)
    done, hlen = np.zeros(B, np.uint8), np.zeros(B, np.int32)
    for b, (segs, closed) in enumerate(spec):
        t = 0
        for L, ext in segs:
            assert ext >= L and t + ext <= T and L <= CAP_SYN
            start[t, b] = start_word(g.integers(1, W - PW + 1), g.integers(1, W - 1), g.integers(H - 3, H - 1))
            live[t:t + L, b] = True
            t += ext
        if segs:
            hlen[b] = segs[-1][0]
            done[b] = 1 if closed and hlen[b] < CAP_SYN else 0
            assert closed or hlen[b] < CAP_SYN
    rec = {
        "action": np.where(live, g.integers(0, 3, (T, B)), 255).astype(np.uint8),
        "reward": np.where(live, g.choice(REWARDS, (T, B)), np.float32(np.nan)).astype(np.float32),
        "mask": live.astype(np.uint8),
        "counts": np.where(live[..., None], g.multinomial(50, [0.3, 0.3, 0.4], (T, B)), -1).astype(np.int64),
        "values": np.where(live, (g.normal(size=(T, B)) * 2).astype(np.float32), np.float32(np.nan)).astype(np.float32),
        "frame": np.where(live[..., None], g.integers(0, 5, (T, B, HW)), 7).astype(np.uint8),
        "start": start,
    }
    return rec, done, hlen


def kept_segments(spec, tail, min_len=None):
    """[(env, t0, L)] of the segments ingest_stream keeps, in its order."""
    min_len = K + 1 if min_len is None else min_len
    out = []
    for b, (segs, closed) in enumerate(spec):
        t = 0
        for i, (L, ext) in enumerate(segs):
            last = i + 1 == len(segs)
            if (not last or closed or tail == "keep") and L > min_len and L >= K:
                out.append((b, t, L))
            t += ext
    return out


def oracle_save_stream(o, rec, spec, tail, H=16, W=20, min_len=None):
    """ReplayOracle.save once per kept segment in (env, start row) order -> windows (evicted ones included)."""
    lut = gray_lut()
    n = 0
    for b, t0, L in kept_segments(spec, tail, min_len):
        s = slice(t0, t0 + L)
        f0 = lut[render_s0(*unpack_start(rec["start"][t0, b]), H, W)].reshape(H, W)
        o.save(rec["action"][s, b].astype(np.int64), lut[rec["frame"][s, b]].reshape(L, H, W), f0, rec["reward"][s, b],
               rec["counts"][s, b], rec["values"][s, b])
        n += L - K + 1
    return n


def random_spec(B, T, seed, empty_runs=()):
    """Per env: segments drawn from SEG_POOL until T is full (extent == L), the last one open or closed at random;
    envs in `empty_runs` ranges get only segments of length <= K + 1 (no kept segment)."""
    g = np.random.default_rng(seed)
    short = SEG_POOL[SEG_POOL <= K + 1]
    none = np.zeros(B, bool)
    for lo, hi in empty_runs:
        none[lo:hi] = True
    spec = []
    for b in range(B):
        pool = short if none[b] else SEG_POOL
        segs, t = [], 0
        while True:
            L = int(g.choice(pool))
            if t + L > T:
                break
            segs.append((L, L))
            t += L
            if g.random() < 0.15:
                break
        full = bool(segs) and segs[-1][0] == CAP_SYN  # at the cap an episode is closed whatever `done` says
        spec.append((segs, bool(g.random() < 0.5) or full))
    return spec


def boot_offsets(spec, tail):
    """For each window position i < K: the set of (s + 10 + i) - L over the kept segments' windows."""
    seen = {i: set() for i in range(K)}
    for _, _, L in kept_segments(spec, tail):
        for s in range(L - K + 1):
            for i in range(K):
                seen[i].add(s + 10 + i - L)
    return seen
