"""GPU: the compact env's two ways of addressing the trajectory sink (include/mzba.h mzba_env_step_compact)."""
import pytest
import torch

from mzba.config import default_config

pytestmark = pytest.mark.gpu


def test_env_step_row_sink_equals_ctx_sink():
    """CompactBreakout.step(action, first_step, rec, t) without a device step context hands the kernel row t of the
    sink; with a context it hands the (T, B, ..) bases and the kernel takes the row from ctx[2]. The same four steps
    of two equally seeded envs through either path must leave the same bytes in rows 0..3 of action, reward, mask and
    frame, and must leave every later row of a poisoned sink (and counts / values, which the step never writes) as
    it was."""
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from mzba import _lib as L
    from mzba.env import CompactBreakout
    B, T, rows, H, W = 3, 4, 6, 16, 20
    actions = torch.randint(0, 3, (T, B), generator=torch.Generator().manual_seed(11)).cuda()
    poison = 0xAB

    def sink():
        shapes = {"action": ((rows, B), torch.uint8), "reward": ((rows, B), torch.float32),
                  "mask": ((rows, B), torch.uint8), "frame": ((rows, B, H * W), torch.uint8),
                  "counts": ((rows, B, 3), torch.int64), "values": ((rows, B), torch.float32)}
        rec = {k: torch.empty(s, dtype=dt, device="cuda") for k, (s, dt) in shapes.items()}
        for v in rec.values():
            v.view(torch.uint8).fill_(poison)
        return rec

    envs = [CompactBreakout(default_config()["environment"], B, 4, H, W, seed=5) for _ in range(2)]
    recs = [sink(), sink()]
    ctx = torch.zeros(3, dtype=torch.int32, device="cuda")
    for env in envs:
        env.reset(0)
    for t in range(T):
        envs[0].step(actions[t], t == 0, recs[0], t)
        envs[1].step(actions[t], False, recs[1], 0, ctx=ctx)  # row and first_step from ctx[2]
        L.call("mzba_ctx_advance", L.ptr(ctx), L.stream())
    assert ctx.tolist() == [T, T, T]
    raw = [{k: v.view(torch.uint8).reshape(rows, -1).cpu() for k, v in rec.items()} for rec in recs]
    for k in ("action", "reward", "mask", "frame"):
        assert torch.equal(raw[0][k][:T], raw[1][k][:T]), k
        assert not (raw[0][k][:T] == poison).all(), k  # the rows were written
    assert raw[0]["mask"][:T].any() and (raw[0]["frame"][:T] < 8).all()
    for r in raw:
        for k, v in r.items():
            assert (v[T if k in ("action", "reward", "mask", "frame") else 0:] == poison).all(), k
    for k in ("paddle", "bx", "by", "done", "hist_len"):
        assert torch.equal(getattr(envs[0], k), getattr(envs[1], k)), k
