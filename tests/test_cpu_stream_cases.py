"""The streaming tests' cases are not vacuous (no GPU): the acted stage restarts envs, the synthetic sinks hold the
segment lengths, bootstrap positions and tails the ingest tests are meant to cover, and the helpers agree with the
oracle env."""
import numpy as np

import stream_cases as SC
from stream_cases import K
from oracle.env import convert_to_grayscale
from mzba.config import small_model_cfg
from mzba.weights import init_state_dict


def _small_cfg(S):
    cfg = SC.default_config()
    cfg["model"] = small_model_cfg(cfg)
    cfg["num_simulations"] = S
    return cfg


def test_render_s0_equals_the_oracle_reset():
    for H, W in ((16, 20), (84, 84)):
        env = SC.make_env(5, H, W)
        p = env.reset_params(7, 3)
        state, _ = env.reset(p)
        g = convert_to_grayscale(state)
        for b in range(5):
            paddle, bx, by = SC.s0_of_params(p, b, H, W)
            assert SC.unpack_start(SC.start_word(paddle, bx, by)) == (paddle, bx, by)
            np.testing.assert_array_equal(SC.gray_lut()[SC.render_s0(paddle, bx, by, H, W)].reshape(H, W), g[b, 0])
            np.testing.assert_array_equal(SC.codes_of_gray(g[b, 0]).reshape(-1), SC.render_s0(paddle, bx, by, H, W))


def test_stage_restarts_envs_under_the_searched_policy():
    """The GPU tests' stage (B = 8, T = 64, small f32 nets, S = 20) in the oracle alone, with the tests' own root
    noise: at least 4 of the 8 envs restart, at least one twice; every restart row carries the key ep_base + t."""
    cfg = _small_cfg(SC.STAGE_S)
    sd = init_state_dict(cfg["model"], SC.STAGE_SD_SEED)
    B, T, seed = SC.STAGE_B, SC.STAGE_T, SC.STAGE_SEED
    act = SC.searched_act_fn(cfg, sd, seed, B, SC.dirichlet_noise_fn(1))
    rec, done, hlen, episodes = SC.stream_oracle(cfg, seed, 0, T, B, act)
    n_restarts = np.array([len(e) - 1 for e in episodes])
    print("restarts per env:", n_restarts.tolist())
    assert (n_restarts >= 1).sum() >= 4 and n_restarts.max() >= 2
    assert all(key == t for e in episodes for t, key in e)
    assert ((rec["start"] != 0).sum(0) == n_restarts + 1).all() and (rec["start"][0] != 0).all()
    assert rec["mask"].all()  # a streamed env records every row
    # and under the short cap every episode ends by the cap
    rec, done, hlen, episodes = SC.stream_oracle(cfg, seed, 0, T, B, SC.random_act_fn(0, B), cap=SC.STAGE_CAP_SHORT)
    segs = SC.segments_of(rec["start"], T, done, hlen, SC.STAGE_CAP_SHORT)
    assert max(t1 - t0 for _, t0, t1, _ in segs) == SC.STAGE_CAP_SHORT
    assert len(segs) >= B * (T // SC.STAGE_CAP_SHORT)


def test_restart_keeps_the_other_envs():
    env = SC.make_env(6)
    state, _ = env.reset(env.reset_params(1, 0))
    done = np.zeros(6, bool)
    for t in range(3):
        state, _, done, _ = env.step(state, np.arange(6) % 3, done)
    dx, dy = env.ball_dx.copy(), env.ball_dy.copy()
    which = np.array([0, 1, 0, 0, 1, 0], bool)
    p = env.reset_params(1, 9)
    s2, d2 = SC.restart_envs(env, state, done | which, which, p)
    fresh = SC.make_env(6)
    f, _ = fresh.reset(p)
    np.testing.assert_array_equal(s2[which], f[which])
    np.testing.assert_array_equal(s2[~which], state[~which])
    np.testing.assert_array_equal(env.ball_dx, np.where(which, fresh.ball_dx, dx))
    np.testing.assert_array_equal(env.ball_dy, np.where(which, fresh.ball_dy, dy))
    assert not d2[which].any()


def test_synthetic_sinks_cover_the_segment_cases():
    T = 64
    spec = SC.random_spec(300, T, seed=3, empty_runs=((0, 3), (150, 191), (297, 300)))
    lens = [L for segs, _ in spec for L, _ in segs]
    assert {K, K + 1, K + 2} <= set(lens) and min(lens) < K
    assert any(len(segs) >= 3 for segs, _ in spec)
    tails = {closed for segs, closed in spec if segs}
    assert tails == {True, False}
    for tail in ("drop", "keep"):
        seen = SC.boot_offsets(spec, tail)
        assert all({-1, 0, 1} <= seen[i] for i in range(K)), seen  # both sides of the 10-step bootstrap boundary
    kept = {b for b, _, _ in SC.kept_segments(spec, "keep")}
    assert not kept & (set(range(3)) | set(range(150, 191)) | set(range(297, 300)))
    assert len(SC.kept_segments(spec, "keep")) > len(SC.kept_segments(spec, "drop")) > 0
    rec, done, hlen = SC.make_stream_sink(spec, T, seed=4)
    segs = SC.segments_of(rec["start"], T, done, hlen, SC.CAP_SYN)
    assert len(segs) == sum(len(s) for s, _ in spec)
    last_closed = {b: c for b, _, _, c in segs}
    assert all(last_closed[b] == closed for b, (s, closed) in enumerate(spec) if s)
    assert np.isnan(rec["reward"][rec["mask"] == 0]).all() and not np.isnan(rec["reward"][rec["mask"] == 1]).any()
