"""Reanalyse on streamed sinks, host side (no GPU): the numpy statement of the streamed representation
input (tests/reanalyse_stream_cases.py) against what the streaming oracle loop offered its search at every row, the
sinks refresh_stream refuses, and the handle bookkeeping of reingest_stream."""
import numpy as np
import pytest
import torch

import reanalyse_stream_cases as RC
import stream_cases as SC
from mzba.reanalyse import Reanalyser
from mzba.replay import DeviceReplayBuffer, StreamHandle


def test_the_definition_equals_the_streaming_oracle_loop():
    """B = 6, T = 40, cap = 7, L = 4, 16x20, random actions: the helper's input from the finished sink equals the x()
    the oracle loop offered to act_fn at that row, for every env. cap = 7 > L, so every env passes through t = t0,
    0 < t - t0 < L - 1 and t - t0 >= L."""
    B, T, cap, L, H, W = 6, 40, 7, 4, 16, 20
    cfg = SC.default_config()
    cfg["model"]["state_history_length"] = L
    inner, offered = SC.random_act_fn(3, B), []

    def act(t, x):
        offered.append(x())
        return inner(t, x)

    o, done, hlen, episodes = SC.stream_oracle(cfg, 11, 0, T, B, act, cap=cap, H=H, W=W)
    assert len(offered) == T and offered[0].shape == (B, 2 * L, H, W)
    rec = {"start": o["start"], "action": o["action"], "frame": SC.codes_of_gray(o["frame"]).reshape(T, B, H * W)}
    age = RC.ages(rec["start"])
    assert (age == 0).any(0).all() and ((age > 0) & (age < L - 1)).any(0).all() and (age >= L).any(0).all()
    assert (rec["start"][1:] != 0).any(), "no restart inside the stage"
    assert age.max() <= cap - 1
    for t in range(T):
        for b in range(B):
            np.testing.assert_array_equal(RC.stream_rep_input(rec, t, b, L, H, W), offered[t][b], err_msg=f"row {t} env {b}")


def test_the_gather_cases_hold_the_segment_lengths():
    """The GPU test's synthetic sinks: all rows recorded, consecutive start words, segments on both sides of L."""
    for H, W, L, T in ((16, 20, 32, 80), (84, 84, 4, 16), (16, 20, 6, 24)):
        for B in (1, 5):
            spec = RC.gather_spec(B, T, L, seed=L + B)
            assert all(sum(n for n, _ in segs) == T for segs, _ in spec)
            rec = RC.make_gather_sink(spec, T, H, W, seed=1)
            assert rec["mask"].all() and rec["start"][0].all()
            assert rec["start"][1, 0] and rec["start"][2, 0], "env 0: a start word at t and at t - 1"
            age = RC.ages(rec["start"])
            assert {0, 1, L - 2, L - 1, L}.issubset(set(age[:, 0].tolist()))
            assert rec["action"].max() <= 2 and rec["frame"].max() <= 4


# ---------------------------------------------------------------------------- the sinks refresh_stream refuses
def _refresher(B=3, H=16, W=20):
    """A Reanalyser's host state without its device buffers: the checks run before the first launch."""
    r = object.__new__(Reanalyser)
    r.B, r.H, r.W = B, H, W
    return r


def _sink(T=4, B=3, HW=320):
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt)  # noqa: E731
    return {"action": z(T, B), "reward": z(T, B, dt=torch.float32), "mask": z(T, B), "frame": z(T, B, HW),
            "counts": z(T, B, 3, dt=torch.int64), "values": z(T, B, dt=torch.float32),
            "start": z(T, B, dt=torch.int32)}


@pytest.mark.parametrize("entry", ["refresh_stream", "begin_stream"])
def test_refresh_stream_refuses_what_it_cannot_reanalyse(entry):
    rec = _sink()
    call = lambda r, *a, **k: getattr(r, entry)(*a, **k)  # noqa: E731
    with pytest.raises(ValueError, match="start"):
        call(_refresher(), {**rec, "start": None}, 4, 0)
    with pytest.raises(ValueError, match="start"):
        call(_refresher(), {k: v for k, v in rec.items() if k != "start"}, 4, 0)
    with pytest.raises(ValueError, match="frames"):
        call(_refresher(), {**rec, "frame": None}, 4, 0)
    with pytest.raises(ValueError, match="envs"):
        call(_refresher(B=4), rec, 4, 0)
    with pytest.raises(ValueError, match="rows"):
        call(_refresher(), rec, 5, 0)
    with pytest.raises(ValueError, match="rows"):
        call(_refresher(), rec, 0, 0)
    with pytest.raises(ValueError, match="start"):
        call(_refresher(), {**rec, "start": torch.zeros(3, 3, dtype=torch.int32)}, 4, 0)
    with pytest.raises(ValueError, match="rows"):
        call(_refresher(), rec, 4, 0, rows=[0, 4])
    with pytest.raises(ValueError, match="rows"):
        call(_refresher(), rec, 4, 0, rows=[-1])


def test_refresh_still_refuses_a_streamed_sink():
    rec = _sink()
    with pytest.raises(ValueError, match="streamed"):
        _refresher().refresh(rec, torch.zeros(3, 320, dtype=torch.uint8), 4, 0)
    with pytest.raises(ValueError, match="streamed"):
        _refresher().begin(rec, torch.zeros(3, 320, dtype=torch.uint8), 4, 0)


def test_snapshot_stream_clones_the_first_rows():
    rec = _sink(T=6)
    rec["start"][2, 1] = 5
    done, hlen = torch.tensor([1, 0, 1], dtype=torch.uint8), torch.tensor([3, 4, 5], dtype=torch.int32)
    snap, d, h = Reanalyser.snapshot_stream({**rec, "extra": None}, 4, done, hlen)
    assert set(snap) == set(rec) | {"extra"} and snap["extra"] is None
    assert all(snap[k].shape[0] == 4 and torch.equal(snap[k], rec[k][:4]) for k in rec)
    rec["start"][2, 1] = 0
    done.zero_(); hlen.zero_()
    assert snap["start"][2, 1] == 5 and d.tolist() == [1, 0, 1] and h.tolist() == [3, 4, 5]


# ---------------------------------------------------------------------------- handles
def test_reingest_stream_without_a_live_handle_touches_no_device():
    """handle=None, a handle of an earlier epoch and a fully evicted one: 0, before any launch (the sink here is a
    dict of nothing and the buffer has no device state)."""
    buf = object.__new__(DeviceReplayBuffer)
    buf._epoch, buf._written, buf.length, buf.max_length = 2, 100, 10, 10
    assert buf.reingest_stream(None, {}, 8, None, None) == 0
    stale = StreamHandle(head=0, n=5, segments=1, serial=0, epoch=1, tail="drop", min_len=6, episode_cap=261)
    assert buf.reingest_stream(stale, {}, 8, None, None) == 0
    evicted = stale._replace(epoch=2, serial=50)  # serials 50 .. 54; the ring holds 90 .. 99
    assert buf.reingest_stream(evicted, {}, 8, None, None) == 0
    assert StreamHandle._fields == ("head", "n", "segments", "serial", "epoch", "tail", "min_len", "episode_cap")
