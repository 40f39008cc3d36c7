"""bench.py end to end on the GPU at a small size: a plain run's line and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_plain_bench_run_times_the_steps_and_dumps_the_last_record(tmp_path):
    """`bench.py --gpus 1 --steps 3 --warmup 1` (256 envs x 4 sims): one JSON line with the headline fields, nothing
    of --full in it, and the last timed step's record row as float32 .npy files: every visit-count row sums to the
    simulation count, actions in 0..2, the mask and rewards of a Breakout step."""
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--envs", "256", "--sims", "4", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = lines[0]
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["ms_per_step"] > 0
    assert abs(d["value"] - 256 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    for k in ("cpu_baseline", "visit_count_match", "visit_count_match_f32_path", "visit_count_match_full", "parity_path"):
        assert d[k] is None, k
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == {"action", "reward", "mask", "frame", "counts", "values"}
    assert all(a.dtype == np.float32 and a.shape[0] == 256 for a in got.values())
    assert got["counts"].shape == (256, 3) and (got["counts"].sum(1) == 4).all()
    assert got["frame"].shape == (256, 320) and np.isin(got["action"], (0, 1, 2)).all()
    assert np.isin(got["mask"], (0, 1)).all() and got["mask"].any() and np.isfinite(got["values"]).all()
