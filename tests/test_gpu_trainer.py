"""The training loop on the GPU (mzba.train.Trainer): the loop closes (train, hand the weights to the
acting agent, count the episodes on the device), warm-up, a resume that continues bit for bit, and an evaluation that
leaves training alone. Small bf16 nets, 8 envs, 64 rows a stage, cap 12, S = 8, two slabs, two minibatches of 8."""
import numpy as np
import pytest
import torch

import episode_stats_cases as EC
import stream_cases as SC
from stream_cases import K

pytestmark = pytest.mark.gpu

B, STEPS, CAP, S, SLABS, NB, MB = 8, 64, 12, 8, 2, 2, 8
SD_SEED, SEED = 5, 3
KINDS = {"uniform": {}, "prioritized": {"prioritized": True}, "reanalyse": {"reanalyse_every": 2}}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib
    _lib.lib()


def _cfg():
    from mzba.config import small_model_cfg
    cfg = SC.default_config()
    cfg["model"] = small_model_cfg(cfg)
    cfg["num_simulations"], cfg["n_parallel"] = S, B
    return cfg


def _agent(cfg, seed=SD_SEED):
    from mzba.agent import MuZeroAgent
    from mzba.weights import init_state_dict
    ag = MuZeroAgent(cfg["model"], dtype="bf16")
    ag.load_state_dict(init_state_dict(cfg["model"], seed))
    return ag


def _trainer(warmup=1, **kw):
    from mzba.learner import Learner
    from mzba.train import Trainer
    from mzba.weights import init_state_dict
    cfg = _cfg()
    ln = Learner(cfg["model"], init_state_dict(cfg["model"], SD_SEED), K=K, dtype="bf16")
    return Trainer(cfg, _agent(cfg), ln, steps=STEPS, slabs=SLABS, episode_cap=CAP, seed=SEED, num_batches=NB,
                   minibatch_size=MB, warmup_windows=warmup, **kw)


def _ints(t):
    return t.contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16, 1: torch.uint8}[t.element_size()])


def _packs(agent):
    from mzba.refresh import named_tensors
    return {k: _ints(v).cpu().clone() for k, v in named_tensors(agent.packed).items()}


def _download(stage):
    env = stage.loop.env
    rec = {k: v[:stage.steps].cpu().numpy() for k, v in stage.loop.rec.items() if v is not None}
    rec["start"] = rec["start"].view(np.uint32)
    return rec, env.done.cpu().numpy(), env.hist_len.cpu().numpy()


def _snapshot(tr):
    """Everything a resumed run must reproduce, as integer host tensors and plain values."""
    ln, arc = tr.learner, tr.archive
    out = {"P": ln.P, "M1": ln.M1, "M2": ln.M2, "stats": tr.stats.block}
    for k in ln.bn_keys:
        out["mean." + k], out["var." + k] = ln.run[k]
    for k, v in arc.rec.items():
        out["sink." + k] = v
    if arc.prioritized:
        out["q"] = arc._q
    out = {k: _ints(v).cpu().clone() for k, v in out.items()}
    out["plain"] = dict(nbt=dict(ln.nbt), step_count=ln.step_count, per_step=ln.per_step, draw_step=arc.draw_step,
                        search_id0=list(arc.search_id0), appended=arc.appended, windows=arc.windows,
                        ep_base=tr.stage.ep_base, search_id=tr.stage.loop.search_id, it=tr.it)
    return out


def _same(a, b):
    assert a["plain"] == b["plain"], (a["plain"], b["plain"])
    assert sorted(a) == sorted(b)
    for k in a:
        if k != "plain":
            assert torch.equal(a[k], b[k]), k


_FOUR = {}


def _four(kind):
    """Four uninterrupted iterations of one kind, once: the snapshot at the end and the per-iteration results."""
    if kind not in _FOUR:
        tr = _trainer(**KINDS[kind])
        outs = [tr.iteration() for _ in range(4)]
        _FOUR[kind] = (_snapshot(tr), outs)
    return _FOUR[kind]


def test_the_loop_closes():
    from mzba.agent import PackedNets
    tr = _trainer()
    before = _packs(tr.agent)
    o = None
    for i in range(3):
        out = tr.iteration()
        assert out["trained"] and out["iteration"] == i + 1 and len(out["losses"]) == NB, out
        assert all(np.isfinite(out["losses"])), out
        rec, done, hlen = _download(tr.stage)
        oi = EC.stats_oracle(rec, STEPS, done, hlen, CAP, gamma=SC.DISCOUNT)
        o = oi if o is None else EC.combine(o, oi)
    assert tr.learner.step_count == 3 * NB == 6
    # the acting agent runs the learner's weights: its packs are the host pack of the learner's state, bit for bit
    ref = PackedNets(tr.learner.state_dict(), tr.cfg["model"], "bf16", "cuda", None)
    from mzba.refresh import named_tensors
    got, want = _packs(tr.agent), {k: _ints(v).cpu() for k, v in named_tensors(ref).items()}
    assert list(got) == list(want)
    for k in got:
        assert torch.equal(got[k], want[k]), k
    assert any(not torch.equal(got[k], before[k]) for k in got)
    d = tr.stats.read()
    assert o["episodes"] > 3 * B
    EC.check_block(d, o, "three stages")


def test_warm_up():
    probe = _trainer(warmup=10 ** 9)
    before = _packs(probe.agent)
    out = probe.iteration()
    w1 = out["windows"]
    assert w1 > 0 and not out["trained"] and out["losses"] == [] and probe.learner.step_count == 0
    after = _packs(probe.agent)
    assert all(torch.equal(before[k], after[k]) for k in before)
    # a threshold one stage does not reach: training starts in the iteration whose append crosses it
    tr = _trainer(warmup=w1 + 1)
    out = tr.iteration()
    assert out["windows"] == w1 and not out["trained"] and tr.learner.step_count == 0
    out = tr.iteration()
    assert out["windows"] >= w1 + 1 and out["trained"] and tr.learner.step_count == NB


@pytest.mark.parametrize("kind", list(KINDS))
def test_resume_is_bit_equal(kind, tmp_path):
    from mzba.checkpoint import load_checkpoint
    want, outs = _four(kind)
    if kind == "reanalyse":
        assert [o["reanalysed"] for o in outs] == [None, 0, None, 0]  # the slab that was not just written
    a = _trainer(**KINDS[kind])
    for _ in range(2):
        a.iteration()
    path = str(tmp_path / "run.pth")
    a.save(path)
    mid = _snapshot(a)
    del a
    b = _trainer(**KINDS[kind])
    ck = b.load(path)
    _same(_snapshot(b), mid)
    assert ck["iteration"] == 2 and ck["training_iteration"] == 2 * NB and ck["replay_buffer"]["length"] == 0
    for _ in range(2):
        b.iteration()
    _same(_snapshot(b), want)
    # the file is still a checkpoint of the existing layout
    cfg = _cfg()
    ag = _agent(cfg, seed=9)
    ck = load_checkpoint(path, agent=ag)
    assert sorted(k for k in ck if k != "trainer") == ["acting_step", "iteration", "model_state_dict",
                                                       "optimizer_state_dict", "replay_buffer", "training_iteration"]
    assert ck["acting_step"] == 2 * STEPS and len(ck["optimizer_state_dict"]["state"]) > 0


def test_save_without_the_archive_resumes_empty(tmp_path):
    a = _trainer()
    a.iteration()
    path = str(tmp_path / "light.pth")
    a.save(path, archive=False)
    b = _trainer()
    b.load(path)
    assert b.archive.windows == 0 and b.archive.appended == 0 and b.archive.draw_step == a.archive.draw_step
    assert torch.equal(b.learner.P, a.learner.P) and b.stage.ep_base == a.stage.ep_base
    out = b.iteration()
    assert out["iteration"] == 2 and out["windows"] > 0 and out["trained"]


def test_evaluation_counts_and_leaves_training_alone():
    want, _ = _four("uniform")
    tr = _trainer()
    for _ in range(2):
        tr.iteration()
    d = tr.evaluate(episodes=2)
    assert d["episodes"] == 2 * B == 16
    assert d["ep_len"].shape == (B, 2) and (d["ep_len"] >= 1).all() and (d["ep_len"] <= CAP).all()
    assert d["len_max"] <= CAP and d["rows"] == int(d["ep_len"].sum())
    stage, _ = tr.eval_stage(2)
    assert stage.steps == 2 * CAP and stage.loop.env_offset == B and stage.loop.seed != tr.stage.loop.seed
    rec, done, hlen = _download(stage)
    o = EC.stats_oracle(rec, stage.steps, done, hlen, CAP, first_n=2, ep_n=2, gamma=SC.DISCOUNT)
    EC.check_block(d, o, "evaluation")
    EC.check_lists(d, o, "evaluation")
    for _ in range(2):
        tr.iteration()
    _same(_snapshot(tr), want)
