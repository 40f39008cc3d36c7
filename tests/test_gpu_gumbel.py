"""The Gumbel search on the device (csrc/gumbel.hip) against the f64 oracle of tests/gumbel_cases.py,
through the nets, the acting loop, the streamed ingest and one learner minibatch; and the PUCT path against a
fixture of its results from before the mode existed."""
import json
import os

import numpy as np
import pytest
import torch

import gumbel_cases as G
from conftest import GOLDEN, ROOT
from mzba.config import default_config, small_model_cfg
from mzba.weights import init_state_dict
from oracle import rng as R

pytestmark = pytest.mark.gpu

TOL = 1e-4  # pi' and value against f64: the f32 restatement sits at 1.6e-5, the rest covers the device's logf / expf
PARITY = os.path.join(ROOT, "profiles", "r11", "gumbel", "parity.json")
_seen = {}


def _cfg(m=3, S=8, B=8, small=False, **gumbel):
    cfg = default_config()
    if small:
        cfg["model"] = small_model_cfg(cfg)
    cfg["num_simulations"] = S
    cfg["n_parallel"] = B
    cfg["search"]["kind"] = "gumbel"
    cfg["search"]["gumbel"] = {"max_considered": m, **gumbel}
    return cfg


def _agent(cfg, seed=5):
    from mzba.agent import MuZeroAgent
    ag = MuZeroAgent(cfg["model"], dtype="f32")
    ag.load_state_dict(init_state_dict(cfg["model"], seed))
    return ag


def _replay(i, z="case", search_id=3, seed=77, **gumbel):
    from mzba.search import replay_search_gumbel
    B, S, m, off, _ = G.CASE_SETS[i]
    c, _ = G.oracle(i)
    return replay_search_gumbel(B, S, _cfg(m, S, **gumbel), c["v_root"], c["pi_root"], c["z"] if isinstance(z, str) else z,
                                c["r"], c["v"], c["pi"], seed, search_id, env_offset=off)


@pytest.fixture(scope="module", autouse=True)
def _parity_record():
    yield
    if not _seen:
        return
    out = {"tolerance": TOL, "ambiguous_margin": G.AMBIGUOUS, "sets": _seen,
           "max_pi_err": max(v["pi_err"] for v in _seen.values()),
           "max_value_err": max(v["value_err"] for v in _seen.values())}
    try:
        os.makedirs(os.path.dirname(PARITY), exist_ok=True)
        with open(PARITY, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass  # a read-only checkout: the figures were asserted above all the same


@pytest.mark.parametrize("i", range(len(G.CASE_SETS)), ids=[f"B{c[0]}_S{c[1]}_m{c[2]}_off{c[3]}" for c in G.CASE_SETS])
def test_replay_against_f64_oracle(i):
    """Unambiguous cases (f64 margin >= 1e-3): every simulation's leaf (parent, action), root N, the considered set
    and the chosen action are the oracle's. All cases: pi' and value within 1e-4 (value relative to max(1, |v|)),
    counts within 1e-4 * 2^24 of the oracle's packing. The ambiguous share stays under the committed caps."""
    B, S, m, off, _ = G.CASE_SETS[i]
    _, o = G.oracle(i)
    d = _replay(i)
    assert G.ambiguous_share(G.SMALL_S) <= 0.05 and G.ambiguous_share(G.LARGE_S) <= 0.10
    ok = o["margin"] >= G.AMBIGUOUS
    np.testing.assert_array_equal(d["leaf_parent"][:, ok], o["leaf_parent"][:, ok])
    np.testing.assert_array_equal(d["leaf_action"][:, ok], o["leaf_action"][:, ok])
    np.testing.assert_array_equal(d["root_n"][ok], o["root_n"][ok])
    np.testing.assert_array_equal(d["considered"][ok], o["considered"][ok])
    np.testing.assert_array_equal(d["actions"][ok], o["action"][ok])
    assert (d["root_n"].sum(1) == S).all()
    pi_err = float(np.abs(d["counts"] / G.Q24 - o["pi"]).max())
    v_err = float((np.abs(d["values"].astype(np.float64) - o["value"]) / np.maximum(1, np.abs(o["value"]))).max())
    cnt_err = int(np.abs(d["counts"] - o["counts"]).max())
    print(f"set {G.CASE_SETS[i]}: pi' err {pi_err:.3g}, value err {v_err:.3g}, counts err {cnt_err}, "
          f"ambiguous {int((~ok).sum())}/{B}")
    _seen[f"B{B}_S{S}_m{m}_off{off}"] = {"pi_err": pi_err, "value_err": v_err, "counts_err": cnt_err,
                                         "ambiguous": int((~ok).sum()), "cases": B}
    assert pi_err <= TOL and v_err <= TOL and cnt_err <= TOL * G.Q24
    assert (np.abs(d["counts"].sum(1) - (1 << 24)) <= 2).all()


def test_device_drawn_variates():
    """Without injected variates the root draws -log(-log u_a), u_a = ((x_a >> 8) + 0.5) / 2^24, from Philox (global env,
    stream 5, search id, a): the formula on oracle/rng.py's words within 1e-5 relative. Two searches with the same ids
    are bit-equal, another search id differs; g = gumbel_scale * variate."""
    i = 6  # B 257, S 8, env_offset 1000
    B, S, m, off, _ = G.CASE_SETS[i]
    a = _replay(i, z=None, search_id=9, seed=123)
    x = R.u32((np.arange(B) + off)[:, None], 5, 9, np.arange(3)[None, :], 123)
    u = ((x >> np.uint32(8)).astype(np.float64) + 0.5) / 2.0 ** 24
    want = -np.log(-np.log(u))
    np.testing.assert_allclose(a["variates"], want, rtol=1e-5, atol=1e-12)
    assert np.isfinite(a["variates"]).all()
    np.testing.assert_array_equal(a["g"].view(np.uint32), a["variates"].view(np.uint32))
    b = _replay(i, z=None, search_id=9, seed=123)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    c = _replay(i, z=None, search_id=10, seed=123)
    assert not np.array_equal(a["variates"], c["variates"])
    h = _replay(i, z=None, search_id=9, seed=123, scale=0.5)
    np.testing.assert_array_equal(h["g"], np.float32(0.5) * a["variates"])


def test_scale_zero_is_independent_of_the_variates():
    i = 6
    c, _ = G.oracle(i)
    a = _replay(i, scale=0.0)
    b = _replay(i, z=np.ascontiguousarray(c["z"][::-1]) * np.float32(3), scale=0.0)
    for k in ("values", "counts", "actions", "root_n", "leaf_parent", "leaf_action", "considered"):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert (a["g"] == 0).all()
    assert not np.array_equal(a["actions"], _replay(i)["actions"])  # the variates do matter at scale 1


def test_run_gumbel_equals_replay_of_its_recorded_network_outputs():
    """Small f32 agent, B = 8, S = 8: the search through the nets and the tree kernels replayed on the network
    outputs it recorded give the same integers and the same value bits; MCTSSearchVec.search returns them."""
    from mzba.search import MCTSSearchVec, replay_search_gumbel
    cfg = _cfg(3, 8, 8, small=True)
    ag = _agent(cfg)
    h = torch.rand(8, 64, 4, 5, generator=torch.Generator().manual_seed(3))
    s = MCTSSearchVec(cfg, ag, None, seed=21, env_offset=2)
    ws = s.workspace(8)
    ws.load_root(h)
    rec = {}
    values, counts, actions = ws.run_gumbel(4, record=rec)
    host = lambda t: t.cpu().numpy()  # noqa: E731
    d = replay_search_gumbel(8, 8, cfg, host(rec["v_root"]), host(rec["pi_root"]), host(ws.gumbel.variates),
                             host(torch.stack(rec["r"])), host(torch.stack(rec["v"])), host(torch.stack(rec["pi"])),
                             21, 4, env_offset=2)
    np.testing.assert_array_equal(host(counts), d["counts"])
    np.testing.assert_array_equal(host(actions), d["actions"])
    np.testing.assert_array_equal(host(ws.gumbel.root_n), d["root_n"])
    np.testing.assert_array_equal(host(values).view(np.uint32), d["values"].view(np.uint32))
    assert (d["root_n"].sum(1) == 8).all() and (np.abs(d["counts"].sum(1) - (1 << 24)) <= 2).all()
    s.search_id = 4
    v2, c2 = s.search(h)
    np.testing.assert_array_equal(c2.numpy(), d["counts"])
    np.testing.assert_array_equal(s.selected_actions.numpy(), d["actions"])
    np.testing.assert_array_equal(v2.numpy().view(np.uint32), d["values"].view(np.uint32))


def test_captured_acting_step_equals_eager_and_the_env_takes_the_chosen_action():
    """Two loops from the same seed: one eager, one replaying its captured step after a first eager step. Every sink
    row is bit-equal. The sink's action row is the search's chosen action, the sampling kernel's temperature has no
    effect, and the oracle env stepped with the recorded actions gives the recorded rewards."""
    from mzba.acting import ActingLoop
    from oracle.env import BreakoutEnvOracle
    cfg = _cfg(3, 8, 8, small=True)
    ag = _agent(cfg)
    B, T = 8, 4
    loops = [ActingLoop(cfg, ag, B, seed=41, temperature=t, max_steps=8) for t in (1.0, 0.25)]
    chosen = []
    for k, loop in enumerate(loops):
        loop.reset(0)
        for t in range(T):
            loop.act(eager=(k == 0))
            if k == 0:
                chosen.append(loop.ws.gumbel.actions.cpu().numpy().copy())
            elif loop.graph is None:
                loop.capture()
    torch.cuda.synchronize()
    assert loops[1].graph is not None
    ra, rb = ({k: v[:T].cpu().numpy() for k, v in lp.rec.items() if v is not None} for lp in loops)
    for k in ra:
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    np.testing.assert_array_equal(ra["action"], np.array(chosen))
    assert (np.abs(ra["counts"].sum(-1) - (1 << 24)) <= 2).all()
    o = BreakoutEnvOracle({**cfg["environment"], "n_parallel": B})
    o.height, o.width = loops[0].H, loops[0].W
    state, _ = o.reset(o.reset_params(41, 0))
    done = np.zeros(B, bool)
    for t in range(T):
        live = ~done
        assert np.array_equal(ra["mask"][t].astype(bool), live)
        state, r, done, _ = o.step(state, ra["action"][t].astype(np.int64), done)
        np.testing.assert_array_equal(ra["reward"][t][live], r[live].astype(np.float32))


def test_streamed_stage_ingest_and_one_minibatch():
    """A StreamingStage (T = 32, B = 8) in Gumbel mode ingested by ingest_stream: every ring `counts` row sums to
    2^24 +- 2 (the fixed-point improved policy survives the sink, the ingest and the ring's f32 row exactly), and one
    Learner.training_stage minibatch on it gives a finite loss."""
    from mzba.learner import Learner
    from mzba.replay import DeviceReplayBuffer
    from mzba.stream import StreamingStage
    cfg = _cfg(3, 8, 8, small=True)
    ag = _agent(cfg)
    st = StreamingStage(cfg, ag, steps=32, episode_cap=12, seed=17)
    K, hist = cfg["num_unroll_steps"], cfg["model"]["state_history_length"]
    buf = DeviceReplayBuffer(hist, K, 1024, cfg["discount_factor"], 8)
    st.run(buf, tail="keep")
    n = len(buf)
    assert n >= 16
    rows = buf._ring["counts"][:n].cpu().numpy().astype(np.float64)
    assert (np.abs(rows.sum(-1) - (1 << 24)) <= 2).all() and (rows >= 0).all()
    sink = st.loop.rec["counts"].cpu().numpy()
    assert set(np.unique(rows)) <= set(np.unique(sink).astype(np.float64))  # the ring's f32 rows hold the sink's integers
    lrn = Learner(cfg["model"], init_state_dict(cfg["model"], 6), K=K)
    losses = lrn.training_stage(buf, 1, 16, generator=torch.Generator().manual_seed(1))
    assert len(losses) == 1 and np.isfinite(losses[0])


def test_puct_path_is_untouched():
    """With no cfg["search"]["kind"], one seeded B = 8, S = 8 search of the small f32 agent gives the counts and the
    value bits stored in tests/golden/puct_b8_s8.npz, which were computed before the Gumbel mode existed."""
    from mzba.agent import MuZeroAgent
    from mzba.search import MCTSSearchVec
    d = np.load(os.path.join(GOLDEN, "puct_b8_s8.npz"))
    cfg = default_config()
    cfg["model"] = small_model_cfg(cfg)
    cfg["num_simulations"] = 8
    ag = MuZeroAgent(cfg["model"], dtype="f32")
    ag.load_state_dict(init_state_dict(cfg["model"], 31))
    h = torch.rand(8, 64, 4, 5, generator=torch.Generator().manual_seed(32))
    s = MCTSSearchVec(cfg, ag, None, seed=33, env_offset=5)
    assert s.kind == "puct" and s.gumbel is None
    values, counts = s.search(h)
    np.testing.assert_array_equal(counts.numpy(), d["counts"])
    np.testing.assert_array_equal(values.numpy().view(np.uint32), d["values"].view(np.uint32))
    assert (d["counts"].sum(1) == 8).all()
