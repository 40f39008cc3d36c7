"""Injected Breakout states for the env kernels, and the oracle step that goes with them.

`make_batch` builds, for a geometry and a seed, a batch of states that the compact representation (csrc/env.hip:
SoA scalars + a brick bitmask over the brick rows, a contiguous paddle) can hold, chosen to reach what trajectories
from reset under random actions never do: wins, lone brick bits, the ball wrapping to the bottom row after a brick hit
at the ceiling, done envs that still move, and every column of the paddle's hit window with its two neighbours. A
random mix supplies most of it; a constructed block walks the ball onto row H-1 at each column pnew-1 .. pnew+pw for
paddles at and next to both walls, because a random mix does not reach those columns at 84x84.

The batch comes in both forms (`planes` for the oracle and the planes kernel, `words` + the scalars for the compact
kernel), `oracle_step` runs `oracle.env.BreakoutEnvOracle` on it once per (geometry, seed) with four distinct dyadic
rewards (every sum exact in any order, every term visible), and `classify` labels each env from the oracle's inputs
and outputs. tests/test_cpu_env_cases.py holds the floor on every class; tests/test_gpu_env_cases.py compares the
kernels with these same oracle runs.
"""
import functools

import numpy as np

from oracle.env import BreakoutEnvOracle

PW = 6
# name -> (H, W, brick_rows); nw = ceil(brick_rows * W / 64) brick words
GEOMETRIES = {
    "16x20": (16, 20, 3),   # nw 1 (60 bits): the headline geometry, the one-word kernel
    "84x84": (84, 84, 3),   # nw 4 (252 bits): config 3
    "8x40": (8, 40, 3),     # nw 2 (120 bits): the four-word kernel with nw < 4
    "16x64": (16, 64, 3),   # nw 3 (192 bits, full words)
    "8x16": (8, 16, 4),     # nw 1, exactly 64 bits: bit 63
    "8x32": (8, 32, 4),     # nw 2, exactly 128 bits
}
SEEDS = (0, 1)
# distinct dyadic values: each of the 16 subsets has its own sum, so a reward names its terms
REWARDS = {"paddle_hit_reward": 0.25, "brick_hit_reward": 1.0, "game_lost_reward": -1.5, "game_won_reward": 5.0}
N_RANDOM = {"84x84": 200}  # random envs per batch (default 440); fewer where the numpy oracle's planes are large
CLASSES = ("missed", "won_live", "brick_up", "brick_down", "wrap_bottom", "ceiling", "ceiling_brick", "lone_bit_clear",
           "paddle_hit_left_edge", "paddle_hit_right_edge", "near_miss_left", "near_miss_right", "wall_left",
           "wall_right", "clamp_left", "clamp_right", "valid0_zero", "valid2_zero", "done_still", "done_velocity",
           "done_velocity_missed", "done_velocity_phantom_hit")
FLOOR = 4  # envs of every class in every batch the GPU tests use
# the envs-per-block runs: the first n envs of seed 0. The large n leave the last block partial at E = 3, 64 and 256
BLOCK_CASES = (("16x20", 668), ("16x20", 40), ("84x84", 428), ("84x84", 40))
# the lockstep runs (oracle_run): the first LOCKSTEP_N envs of seed LOCKSTEP_SEED, T = 3L steps, L in LOCKSTEP_L
LOCKSTEP_GEOMETRIES, LOCKSTEP_L, LOCKSTEP_SEED, LOCKSTEP_N = ("16x20", "8x40"), (2, 4), 1, 300


def nwords(geom):
    H, W, rows = GEOMETRIES[geom]
    return (rows * W + 63) // 64


def _random_block(g, n, H, W, rows):
    paddle = np.where(g.random(n) < 0.2, g.choice([0, 1, W - PW - 1, W - PW], n), g.integers(0, W - PW + 1, n))
    edge_rows = np.r_[0:rows + 2, H - 3:H]
    by = np.where(g.random(n) < 0.5, g.choice(edge_rows, n), g.integers(0, H, n))
    bx = np.where(g.random(n) < 0.25, g.choice([0, W - 1], n), g.integers(0, W, n))
    dx, dy = g.choice([-1, 1], n), g.choice([-1, 1], n)
    bricks = np.zeros((n, rows, W), bool)
    kind = g.choice(6, n, p=[0.3, 0.2, 0.1, 0.15, 0.15, 0.1])
    for b in range(n):
        k = kind[b]
        if k == 0:    # pair-aligned random
            bricks[b] = np.repeat(g.random((rows, W // 2)) < g.choice([0.1, 0.5, 0.9]), 2, axis=1)
        elif k == 1:  # random single bits
            bricks[b] = g.random((rows, W)) < g.choice([0.05, 0.5])
        elif k == 2:  # full
            bricks[b] = True
        elif k in (3, 4):  # one pair / one bit, anywhere in the mask; half of them with the ball aimed at it
            r, c = g.integers(0, rows), g.integers(0, W)
            if k == 3:
                bricks[b, r, c - c % 2: c - c % 2 + 2] = True
            else:
                bricks[b, r, c] = True
            y, x = r - dy[b], c - dx[b]
            if g.random() < 0.5 and 0 <= y < H and 0 <= x < W:
                by[b], bx[b] = y, x
        # k == 5: empty
    u = g.random(n)
    done = u < 0.16
    still = u < 0.08
    dx[still] = 0
    dy[still] = 0
    bricks[done] = False
    return paddle, bx, by, dx, dy, done, bricks, g.integers(0, 3, n)


def _constructed_block(g, H, W, rows):
    """Live envs, ball at row H-2 moving down onto row H-1 at every column pnew-1 .. pnew+pw, both dx, for paddles
    at and next to both walls and one interior column, every action (the clamps: paddle 0 with action 0, paddle
    W-pw with action 2). Then done envs that still move: onto the phantom paddle at column 0, and off the bottom."""
    out = []
    for p0 in (0, 1, W - PW - 1, W - PW, (W - PW) // 2):
        for a in (0, 1, 2):
            pnew = min(max(p0 + a - 1, 0), W - PW)
            for c in range(pnew - 1, pnew + PW + 1):
                for dx in (-1, 1):
                    if 0 <= c < W and 0 <= c - dx < W:
                        out.append((p0, c - dx, H - 2, dx, 1, False, a))
    for c in (0, 2, PW - 1, PW):
        for dx in (-1, 1):
            if 0 <= c - dx < W:
                out.append((g.integers(0, W - PW + 1), c - dx, H - 2, dx, 1, True, g.integers(0, 3)))
    for x in (0, 1, 3, W // 2, W - 4, W - 1):
        out.append((g.integers(0, W - PW + 1), x, H - 1, g.choice([-1, 1]), 1, True, g.integers(0, 3)))
    n_rand = len(out)
    # full bricks: a miss, the ceiling with a brick above it, a brick below row 0 (both wrap to row H-1)
    for x in (0, 1, 2, W // 2, W - 3, W - 1):
        for y, dy in ((H - 1, 1), (0, -1), (0, 1)):
            out.append((g.integers(0, W - PW + 1), x, y, g.choice([-1, 1]), dy, False, g.integers(0, 3)))
    n_full = len(out)
    # a lone odd brick bit with the ball moving onto its pair (cleared without a hit); a far pair keeps the env live
    lone = [(rows - 1, 3, 1), (rows - 1, W - 1, -1), (1, W // 2 + 1, 1), (1, W // 2 - 1, -1), (0, 5, -1), (0, W - 5, -1)]
    for r, c, dy in lone:
        out.append((g.integers(0, W - PW + 1), c - 2, r - dy, 1, dy, False, g.integers(0, 3)))
    paddle, bx, by, dx, dy, done, action = (np.array(v) for v in zip(*out))
    n = len(out)
    bricks = np.repeat(g.random((n, rows, W // 2)) < 0.5, 2, axis=2)
    bricks[:, 0, :2] = True  # never empty: no win hides the paddle
    bricks[n_rand:n_full] = True
    bricks[n_full:] = False
    for i, (r, c, _) in enumerate(lone):
        bricks[n_full + i, r, c] = True
        bricks[n_full + i, rows - 1 - r, (c + W // 2) % W // 2 * 2: (c + W // 2) % W // 2 * 2 + 2] = True
    bricks[done] = False
    return paddle, bx, by, dx, dy, done, bricks, action


@functools.lru_cache(maxsize=None)
def make_batch(geom, seed):
    """The batch as read-only arrays: paddle, bx, by, dx (int32), dy (float32), done (uint8), action (int64),
    bricks (bool (B, brick_rows, W)). A done env has no bricks and no paddle plane; its `paddle` entry is what the
    kernel last stored there, any legal column."""
    H, W, rows = GEOMETRIES[geom]
    g = np.random.default_rng([seed, H, W, rows])
    blocks = [_constructed_block(g, H, W, rows), _random_block(g, N_RANDOM.get(geom, 440), H, W, rows)]
    paddle, bx, by, dx, dy, done, bricks, action = (np.concatenate(v) for v in zip(*blocks))
    perm = g.permutation(len(paddle))  # classes spread over the blocks of a launch
    batch = {"paddle": paddle.astype(np.int32), "bx": bx.astype(np.int32), "by": by.astype(np.int32),
             "dx": dx.astype(np.int32), "dy": dy.astype(np.float32), "done": done.astype(np.uint8),
             "bricks": bricks, "action": action.astype(np.int64)}
    batch = {k: np.ascontiguousarray(v[perm]) for k, v in batch.items()}
    for v in batch.values():
        v.setflags(write=False)
    return batch


def take(batch, idx):
    """The sub-batch of envs `idx` (a slice or an index array)."""
    return {k: np.ascontiguousarray(v[idx]) for k, v in batch.items()}


def planes(batch, geom):
    """(B, 3, H, W) f32: the reference's state."""
    H, W, rows = GEOMETRIES[geom]
    B = len(batch["paddle"])
    s = np.zeros((B, 3, H, W), np.float32)
    cols = np.arange(W)[None, :]
    live = batch["done"][:, None] == 0
    s[:, 0, H - 1] = live & (cols >= batch["paddle"][:, None]) & (cols < batch["paddle"][:, None] + PW)
    s[np.arange(B), 1, batch["by"], batch["bx"]] = 1
    s[:, 2, :rows] = batch["bricks"]
    return s


def words(batch, geom):
    """(B, nw) uint64 brick masks, bit = row * W + col."""
    B = len(batch["paddle"])
    nw = nwords(geom)
    bits = np.zeros((B, nw * 64), np.uint8)
    flat = batch["bricks"].reshape(B, -1)
    bits[:, :flat.shape[1]] = flat
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u8").reshape(B, nw)


def compact_to_planes(paddle, bx, by, done, brick_words, geom):
    """numpy restatement of compact_to_planes_kernel (csrc/env.hip), pixel by pixel."""
    H, W, rows = GEOMETRIES[geom]
    B = len(paddle)
    s = np.zeros((B, 3, H, W), np.float32)
    for y in range(H):
        for x in range(W):
            s[:, 0, y, x] = (done == 0) & (y == H - 1) & (x >= paddle) & (x < paddle + PW)
            s[:, 1, y, x] = (y == by) & (x == bx)
            if y < rows:
                bit = y * W + x
                s[:, 2, y, x] = (brick_words[:, bit >> 6] >> np.uint64(bit & 63)) & np.uint64(1)
    return s


def reset_params(geom, B, seed=0):
    """Legal explicit reset draws (paddle offset, ball column, ball row offset, dx), int64 (B,) each. The keyed
    draws' offset range is the reference's for W = 20 and leaves the field at small W."""
    H, W, rows = GEOMETRIES[geom]
    g = np.random.default_rng([seed, W, 77])
    off = g.integers(0, W - PW + 1, B) - (W // 2 - PW // 2)
    return off, g.integers(0, W, B), g.integers(-3, -1, B), g.choice([-1, 1], B)


def make_oracle(geom, B):
    H, W, rows = GEOMETRIES[geom]
    o = BreakoutEnvOracle({**REWARDS, "n_parallel": B}, paddle_width=PW)
    o.height, o.width, o.brick_rows = H, W, rows
    return o


def oracle_from(batch, geom):
    """An oracle env holding the batch's ball directions, its planes and its done mask (fresh arrays)."""
    o = make_oracle(geom, len(batch["paddle"]))
    o.ball_dx = batch["dx"].astype(np.int64)
    o.ball_dy = batch["dy"].astype(np.float32)
    return o, planes(batch, geom), batch["done"].astype(bool)


@functools.lru_cache(maxsize=None)
def oracle_step(geom, seed):
    """One oracle step of make_batch(geom, seed), computed once: state, next_state, reward, done, valid, dx, dy."""
    batch = make_batch(geom, seed)
    o, s, done = oracle_from(batch, geom)
    ns, r, done, valid = o.step(s, batch["action"], done)
    out = {"state": s, "next_state": ns, "reward": r, "done": done, "valid": valid, "dx": o.ball_dx, "dy": o.ball_dy}
    for v in out.values():
        v.setflags(write=False)
    return out


def codes_of(state):
    """u8 gray codes of planes, (B, H*W): bit 0 paddle, bit 1 ball, bit 2 brick (csrc/env.hip)."""
    p = state.astype(np.uint8)
    return (p[:, 0] | (p[:, 1] << 1) | (p[:, 2] << 2)).reshape(len(p), -1)


@functools.lru_cache(maxsize=None)
def oracle_run(geom, seed, n, L, rec_flags, T):
    """T oracle steps of random actions from the first n envs of make_batch(geom, seed), recorded the way the acting
    loop records (train_torch.py:179, :204-209): rec = ~prev_done, and prev_done aliases done at the first step, so
    step 0 records the envs still live after it. rec_flags bit 0 records every env, bit 1 records env 0's action for
    all (run_test_simulation). The history starts as the ring does after a reset with reset_params(geom, n): L - 1
    copies of that reset state's frame and L pad actions 0, not the injected state.

    Returns, computed once: `actions` (T, n), `steps` (per step the dict check of next_state, reward, done, valid, dx,
    dy plus `rec` and `hist_len`), `sink` (the (T, n, ..) action / reward / mask / frame rows), `trajs` (an
    oracle.acting.Trajectory per env) and `gray` (the final frames)."""
    from oracle.acting import Trajectory
    from oracle.env import convert_to_grayscale
    H, W, rows = GEOMETRIES[geom]
    batch = take(make_batch(geom, seed), slice(0, n))
    g0 = convert_to_grayscale(make_oracle(geom, n).reset(reset_params(geom, n))[0])
    trajs = [Trajectory(L, g0[b]) for b in range(n)]
    o, s, done = oracle_from(batch, geom)
    g = np.random.default_rng([seed, n, L, T])
    actions = g.integers(0, 3, (T, n))
    sink = {"action": np.zeros((T, n), np.uint8), "reward": np.zeros((T, n), np.float32),
            "mask": np.zeros((T, n), np.uint8), "frame": np.zeros((T, n, H * W), np.uint8)}
    steps, prev = [], None
    for t in range(T):
        a = actions[t]
        s, r, done, valid = o.step(s, a, done)
        rec = ~(done if t == 0 else prev)
        if rec_flags & 1:
            rec = np.ones(n, bool)
        ra = np.full(n, a[0]) if rec_flags & 2 else a
        prev = done.copy()
        gray = convert_to_grayscale(s)
        for b in np.flatnonzero(rec):
            trajs[b].add_observation(ra[b], gray[b], r[b], np.zeros(3, np.int64), 0.0)
        sink["action"][t], sink["reward"][t], sink["mask"][t], sink["frame"][t] = ra, r, rec, codes_of(s)
        steps.append({"next_state": s, "reward": r, "done": done.copy(), "valid": valid, "dx": o.ball_dx.copy(),
                      "dy": o.ball_dy.copy(), "rec": rec, "hist_len": np.array([tr.length for tr in trajs], np.int32)})
    return {"actions": actions, "steps": steps, "sink": sink, "trajs": trajs, "gray": convert_to_grayscale(s)}


def classify(batch, out, geom):
    """name -> bool (B,) for every class of CLASSES, from the oracle's inputs (`batch`) and outputs (`out`)."""
    H, W, rows = GEOMETRIES[geom]
    B = len(batch["paddle"])
    s, ns = out["state"], out["next_state"]
    done_in = batch["done"] != 0
    dx, dy, x, y, a = batch["dx"], batch["dy"], batch["bx"], batch["by"], batch["action"]
    # the reward names its terms (REWARDS: 16 distinct subset sums)
    vals = np.array([REWARDS[k] for k in ("paddle_hit_reward", "brick_hit_reward", "game_lost_reward",
                                          "game_won_reward")], np.float32)
    sums = np.array([[(vals * [(m >> i) & 1 for i in range(4)]).sum() for m in range(16)]], np.float32)
    term = np.argmax(out["reward"][:, None] == sums, axis=1)
    assert (sums[0, term] == out["reward"]).all()
    paddle_hit, brick, lost, won = ((term >> i) & 1 == 1 for i in range(4))
    p_in = np.argmax(s[:, 0, H - 1], axis=1)
    pnew = np.clip(p_in + a - 1, 0, W - PW)
    _, fy, fx = np.nonzero(ns[:, 1] == 1)
    assert len(fy) == B
    live = ~done_in & ~lost  # neither done nor missing: the brick test and the clear see its bricks
    b = np.arange(B)
    landed = live & ~brick & (fy < rows)  # no hit: the ball sits on the tested cell
    c = {
        "missed": lost & ~done_in,
        "won_live": won & live,
        "brick_up": brick & (dy < 0) & (y > 0),
        "brick_down": brick & (dy > 0),
        "wrap_bottom": brick & (y == 0) & (fy == H - 1),
        "ceiling": ~done_in & (dy < 0) & (y == 0),
        "ceiling_brick": brick & (dy < 0) & (y == 0),
        "lone_bit_clear": landed & (s[b, 2, np.minimum(fy, rows - 1), fx | 1] == 1)
        & (s[b, 2, np.minimum(fy, rows - 1), fx & ~1] == 0),
        "paddle_hit_left_edge": paddle_hit & ~done_in & (fx == pnew),
        "paddle_hit_right_edge": paddle_hit & ~done_in & (fx == pnew + PW - 1),
        "near_miss_left": live & ~brick & ~paddle_hit & (fy == H - 1) & (fx == pnew - 1),
        "near_miss_right": live & ~brick & ~paddle_hit & (fy == H - 1) & (fx == pnew + PW),
        "wall_left": ~done_in & (dx < 0) & (x == 0),
        "wall_right": ~done_in & (dx > 0) & (x == W - 1),
        "clamp_left": ~done_in & (p_in == 0) & (a == 0),
        "clamp_right": ~done_in & (p_in == W - PW) & (a == 2),
        "valid0_zero": out["valid"][:, 0] == 0,
        "valid2_zero": out["valid"][:, 2] == 0,
        "done_still": done_in & (dx == 0) & (dy == 0),
        "done_velocity": done_in & (dx != 0),
        "done_velocity_missed": done_in & lost,
        "done_velocity_phantom_hit": done_in & paddle_hit,
    }
    assert tuple(c) == CLASSES
    return c


def labels(classes):
    """Per env, the names of its classes, for failure messages."""
    B = len(next(iter(classes.values())))
    return ["+".join(k for k, m in classes.items() if m[b]) or "plain" for b in range(B)]
