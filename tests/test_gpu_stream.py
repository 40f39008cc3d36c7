"""Streaming acting on the GPU: the restart kernel (csrc/env.hip) against the oracle env and a fresh reset, and a
streamed stage (mzba.stream.StreamingStage) against action replay in the oracle env, the lockstep ActingLoop, the
streaming oracle loop (tests/stream_cases.py) and its own graph replay."""
import numpy as np
import pytest
import torch

import stream_cases as SC
from oracle.acting import Trajectory, prepare_mcts_input
from oracle.env import convert_to_grayscale
from mzba.config import small_model_cfg
from mzba.env import gray_lut
from mzba.weights import init_state_dict

pytestmark = pytest.mark.gpu

STATE = ("paddle", "bx", "by", "dx", "dy", "done", "bricks", "hist_frames", "hist_actions", "hist_len", "cur_frame",
         "cur_src")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def _snapshot(env):
    return {k: getattr(env, k).clone() for k in STATE if getattr(env, k) is not None}


def _per_env(env, k, v):
    return v.view(env.B, -1).cpu().numpy()


def _i32(x):
    return torch.tensor(x, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("B,H,W,Lh,single_write,pad_action,inject", [
    (1, 16, 20, 32, True, 0, False), (5, 16, 20, 32, False, 1, True), (257, 16, 20, 32, True, 1, False),
    (257, 16, 20, 8, False, 0, True), (5, 84, 84, 4, True, 1, False), (5, 84, 84, 4, False, 0, True)])
def test_restart_kernel(B, H, W, Lh, single_write, pad_action, inject):
    """B = 1, 5 (one ragged block), 257 (five blocks of 64, the last with one env); both frame-storage modes; the
    keyed draws and injected params. t = 0 writes every env's start word and resets nothing; at t = 2 exactly the
    done envs and those at the record cap are reset, to what a fresh reset under the key ep_base + 2 gives."""
    from mzba.env import CompactBreakout
    seed, ep_base, cap, T = 11, 40, 5, 4
    cfg_env = SC.CFG["environment"]
    mk = lambda: CompactBreakout(cfg_env, B, Lh, H, W, seed=seed, pad_action=pad_action, single_write=single_write)  # noqa: E731
    env, o = mk(), SC.make_env(B, H, W)
    p0 = o.reset_params(seed, ep_base)
    env.reset(ep_base)
    start = torch.zeros(T, B, dtype=torch.int32, device="cuda")
    ctx, blk = _i32([0, 0, 0]), _i32([ep_base, cap])
    before = _snapshot(env)
    env.restart(start, ctx, blk, None)
    for k, v in before.items():
        assert torch.equal(getattr(env, k), v), f"t = 0 changed {k}"
    words = start.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(words[0], [SC.start_word(*SC.s0_of_params(p0, b, H, W)) for b in range(B)])
    assert not words[1:].any()
    # three steps, then flag envs: done, at the cap, both, neither
    g = np.random.default_rng(B + H)
    for t in range(3):
        env.step(torch.as_tensor(g.integers(0, 3, B), device="cuda"), t == 0)
    assert (env.hist_len == 3).all() and not env.done.any()
    flag_done, flag_cap = g.random(B) < 0.3, g.random(B) < 0.3
    flag_done[0] = flag_cap[B - 1] = True
    if B > 2:
        flag_done[1] = flag_cap[1] = False
    env.done.copy_(torch.as_tensor(flag_done.astype(np.uint8)))
    env.hist_len.copy_(torch.as_tensor(np.where(flag_cap, cap + (np.arange(B) % 2), 3).astype(np.int32)))
    which = flag_done | flag_cap
    if B > 1:
        which_not = ~which
        assert which_not.any()
    params = o.reset_params(seed + 1, 7) if inject else None  # injected: draws no key of this stage gives
    dparams = None if params is None else torch.as_tensor(np.asarray(params, np.int32), device="cuda").contiguous()
    before = _snapshot(env)
    ctx[2] = 2
    env.restart(start, ctx, blk, dparams)
    fresh = mk()
    fresh.reset(ep_base + 2, params)
    pe = params if inject else o.reset_params(seed, ep_base + 2)
    for k, v in before.items():
        got, old, new = (_per_env(env, k, x) for x in (getattr(env, k), v, getattr(fresh, k)))
        if k == "cur_frame" and single_write:
            new = old  # single-write mode: a reset leaves cur_frame alone (the current frame is the ring's newest)
        np.testing.assert_array_equal(got[~which], old[~which], err_msg=f"{k}: an env that does not restart changed")
        np.testing.assert_array_equal(got[which], new[which], err_msg=f"{k}: restarted envs differ from a fresh reset")
    words = start.cpu().numpy().view(np.uint32)
    exp = np.array([SC.start_word(*SC.s0_of_params(pe, b, H, W)) if which[b] else 0 for b in range(B)], np.uint32)
    np.testing.assert_array_equal(words[2], exp)
    assert not words[1].any() and not words[3].any() and words[0].all()
    # against the oracle: planes, ball direction, current frame, rep input of a fresh Trajectory
    so, _ = o.reset(pe)
    g0 = convert_to_grayscale(so)
    idx = np.flatnonzero(which)
    np.testing.assert_array_equal(env.to_planes().cpu().numpy()[idx], so[idx])
    np.testing.assert_array_equal(env.dx.cpu().numpy()[idx], o.ball_dx[idx])
    np.testing.assert_array_equal(env.dy.cpu().numpy()[idx], o.ball_dy[idx])
    cur = env.current_frame().view(B, H * W).cpu().numpy()
    cs = (2 * Lh + 63) // 64 * 64
    x = torch.zeros(B, H * W, cs, dtype=torch.float32, device="cuda")
    env.build_rep_input(x, cs, False)
    x = x.cpu().numpy()
    for b in idx:
        np.testing.assert_array_equal(cur[b], SC.render_s0(*SC.s0_of_params(pe, b, H, W), H, W))
        ref = prepare_mcts_input(g0[b], Trajectory(Lh, g0[b], pad_action), Lh)
        np.testing.assert_array_equal(x[b, :, :2 * Lh].T.reshape(2 * Lh, H, W), ref)


# ---------------------------------------------------------------------------- a streamed stage
def _small_cfg(S, B):
    cfg = SC.default_config()
    cfg["model"] = small_model_cfg(cfg)
    cfg["num_simulations"] = S
    cfg["n_parallel"] = B
    return cfg


def _agent(cfg):
    from mzba.agent import MuZeroAgent
    sd = init_state_dict(cfg["model"], SC.STAGE_SD_SEED)
    ag = MuZeroAgent(cfg["model"], dtype="f32")
    ag.load_state_dict(sd)
    return ag, sd


def _host(stage):
    rec = {k: v.cpu().numpy() for k, v in stage.loop.rec.items()}
    rec["start"] = rec["start"].view(np.uint32)
    return rec, stage.loop.env.done.cpu().numpy(), stage.loop.env.hist_len.cpu().numpy()


@pytest.fixture(scope="module")
def stage_run():
    """The stage every acted test reads: B = 8, T = 64, small f32 nets, S = 20, eager with the device's root noise
    logged. Computed once and left unchanged."""
    from mzba.stream import StreamingStage
    cfg = _small_cfg(SC.STAGE_S, SC.STAGE_B)
    ag, sd = _agent(cfg)
    st = StreamingStage(cfg, ag, steps=SC.STAGE_T, seed=SC.STAGE_SEED, use_graph=False)
    st.loop.noise_log = []
    trajs = st.run(trajectories=True)
    rec, done, hlen = _host(st)
    noises = [n.cpu().numpy() for n in st.loop.noise_log]
    return dict(cfg=cfg, ag=ag, sd=sd, rec=rec, done=done, hlen=hlen, noises=noises, trajs=trajs)


def _replay_actions(rec, done, hlen, seed, ep_base, T, B, cap):
    """Every segment again in the oracle env from its keyed reset, fed the recorded actions: frames, rewards and
    the row at which it ends."""
    lut = gray_lut()
    segs = SC.segments_of(rec["start"], T, done, hlen, cap)
    assert (rec["start"][0] != 0).all()
    for b, t0, t1, closed in segs:
        o = SC.make_env(B)
        p = o.reset_params(seed, ep_base + t0)
        assert rec["start"][t0, b] == SC.start_word(*SC.s0_of_params(p, b))
        state, _ = o.reset(p)
        d = np.zeros(B, bool)
        for t in range(t0, t1):
            assert not d[b] and rec["mask"][t, b] == 1, (b, t0, t)
            a = np.ones(B, np.int64)
            a[b] = rec["action"][t, b]
            state, r, d, _ = o.step(state, a, d)
            np.testing.assert_array_equal(lut[rec["frame"][t, b] & 7].reshape(16, 20), convert_to_grayscale(state)[b, 0])
            assert np.float32(r[b]).view(np.uint32) == rec["reward"][t, b].view(np.uint32)
        if t1 < T:  # a later segment follows: this one ended at row t1 - 1, by the game or by the cap
            assert d[b] or t1 - t0 == cap, (b, t0, t1)
        else:
            assert closed == bool(d[b] or t1 - t0 >= cap) and done[b] == d[b] and hlen[b] == t1 - t0
    return segs


def test_action_replay(stage_run):
    s = stage_run
    segs = _replay_actions(s["rec"], s["done"], s["hlen"], SC.STAGE_SEED, 0, SC.STAGE_T, SC.STAGE_B, 261)
    n = np.bincount([b for b, *_ in segs], minlength=SC.STAGE_B) - 1
    print("restarts per env:", n.tolist())
    assert (n >= 1).sum() >= 4 and n.max() >= 2
    # stream_trajectories lists the same segments
    assert [(b, t0, c) for b, t0, c, _ in s["trajs"]] == [(b, t0, c) for b, t0, _, c in segs]
    assert [tr.length for *_, tr in s["trajs"]] == [t1 - t0 for _, t0, t1, _ in segs]


def test_action_replay_short_cap_captured():
    """episode_cap = 12 on the captured step graph, two stages: every episode is cut at 12 records at the latest and
    the second stage's keys start at T."""
    from mzba.stream import StreamingStage
    cfg = _small_cfg(SC.STAGE_S, SC.STAGE_B)
    ag, _ = _agent(cfg)
    cap = SC.STAGE_CAP_SHORT
    st = StreamingStage(cfg, ag, steps=SC.STAGE_T, episode_cap=cap, seed=SC.STAGE_SEED)
    for i in range(2):
        st.run()
        assert st.loop.graph is not None and st.ep_base == (i + 1) * SC.STAGE_T
        rec, done, hlen = _host(st)
        segs = _replay_actions(rec, done, hlen, SC.STAGE_SEED, i * SC.STAGE_T, SC.STAGE_T, SC.STAGE_B, cap)
        lens = [t1 - t0 for _, t0, t1, _ in segs]
        assert max(lens) == cap and len(segs) >= SC.STAGE_B * (SC.STAGE_T // cap)


def test_first_segments_equal_the_lockstep_loop(stage_run):
    from mzba.acting import ActingLoop
    s = stage_run
    B, T = SC.STAGE_B, SC.STAGE_T
    loop = ActingLoop(s["cfg"], s["ag"], B, seed=SC.STAGE_SEED, max_steps=T)
    loop.reset(0)
    while not loop.all_done() and loop.t < T:
        loop.act(eager=True)
    lock = {k: v.cpu().numpy() for k, v in loop.rec.items()}
    rec = s["rec"]
    ends = []
    for b in range(B):
        n = int(lock["mask"][:, b].sum())
        rows = np.flatnonzero(rec["start"][:, b])
        first = (rows[1] if len(rows) > 1 else T)
        assert n == first, (b, n, first)
        ends.append(n)
        for k in ("action", "reward", "counts", "values", "frame", "mask"):
            np.testing.assert_array_equal(np.ascontiguousarray(rec[k][:n, b]).view(np.uint8),
                                          np.ascontiguousarray(lock[k][:n, b]).view(np.uint8), err_msg=f"{k} env {b}")
    assert min(ends) < T  # some env's first episode ended inside the stage


def test_stage_matches_the_streaming_oracle(stage_run):
    """Bounds of test_acting_loop_f32_matches_oracle_episode: integers equal, values rtol 1e-4 / atol 1e-5."""
    s = stage_run
    B, T, seed = SC.STAGE_B, SC.STAGE_T, SC.STAGE_SEED
    act = SC.searched_act_fn(s["cfg"], s["sd"], seed, B, lambda sid, n: s["noises"][sid])
    o, odone, ohlen, episodes = SC.stream_oracle(s["cfg"], seed, 0, T, B, act)
    rec = s["rec"]
    np.testing.assert_array_equal(rec["start"], o["start"])
    np.testing.assert_array_equal(rec["mask"], o["mask"])
    np.testing.assert_array_equal(rec["action"], o["action"])
    np.testing.assert_array_equal(rec["counts"], o["counts"])
    np.testing.assert_array_equal(rec["reward"].view(np.uint32), o["reward"].view(np.uint32))
    np.testing.assert_array_equal(gray_lut()[rec["frame"] & 7].reshape(T, B, 16, 20), o["frame"])
    np.testing.assert_allclose(rec["values"], o["values"], rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(s["done"].astype(bool), odone)
    np.testing.assert_array_equal(s["hlen"], ohlen)
    n = np.array([len(e) - 1 for e in episodes])
    assert (n >= 1).sum() >= 4 and n.max() >= 2


def test_graph_replay_equals_eager_over_two_stages():
    """Two consecutive stages, captured against eager (device noise in both): bit-equal sinks, so the one graph
    serves the second stage's ep_base."""
    from mzba.stream import StreamingStage
    cfg = _small_cfg(SC.STAGE_S, SC.STAGE_B)
    ag, _ = _agent(cfg)
    T = 32
    a = StreamingStage(cfg, ag, steps=T, episode_cap=SC.STAGE_CAP_SHORT, seed=SC.STAGE_SEED, use_graph=True)
    e = StreamingStage(cfg, ag, steps=T, episode_cap=SC.STAGE_CAP_SHORT, seed=SC.STAGE_SEED, use_graph=False)
    for i in range(2):
        a.run()
        e.run()
        assert a.loop.graph is not None and e.loop.graph is None and a.ep_base == e.ep_base == (i + 1) * T
        (ra, da, ha), (re, de, he) = _host(a), _host(e)
        for k in ra:
            np.testing.assert_array_equal(ra[k].view(np.uint8), re[k].view(np.uint8), err_msg=f"{k}, stage {i}")
        np.testing.assert_array_equal(da, de)
        np.testing.assert_array_equal(ha, he)
        assert (ra["start"][1:] != 0).sum() >= SC.STAGE_B  # restarts inside both stages


def test_multi_rank_streaming_is_refused():
    from mzba.stream import StreamingStage
    cfg = _small_cfg(SC.STAGE_S, SC.STAGE_B)
    ag, _ = _agent(cfg)
    with pytest.raises(NotImplementedError):
        StreamingStage(cfg, ag, steps=8, world_size=2)
