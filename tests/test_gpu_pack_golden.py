"""The host packer's bits (mzba/agent.py PackedNets) against recorded hashes: tests/golden/pack_sha256.json.

For each configuration, PackedNets(_state(mcfg, 3), mcfg, dtype, "cuda", dyn_dtype) is built (test_gpu_refresh's drawn
BatchNorm state: negative, zero and tiny-variance channels) and every tensor of refresh.named_tensors(pack) is compared
by path, dtype, numel and the SHA-256 of its raw bytes. Configurations: N, W and W16 in bf16 as test_gpu_refresh uses
them (plain, wf, wt, act_bias, wb, tower, fused, fp16, rep_tail and rep_blocks packs), and W in f32 (the split packs
wx, wx3, wsc). Zero differing hashes is the only pass.

The fixture was written by this module (`python tests/test_gpu_pack_golden.py --write`) on the tree of commit 3f03f17
("Weight hand-off on device"), before the host fold and the tower pack became shared helpers. It is never regenerated
from the tree under test: a packer change that moves a bit has to say so and rewrite it from the commit before.
"""
import hashlib
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "pack_sha256.json")

CASES = [("N", "bf16"), ("W", "bf16"), ("W16", "bf16"), ("W", "f32")]

pytestmark = pytest.mark.gpu


def _hashes(name, dtype):
    """[[path, dtype, numel, sha256 of the raw bytes], ...] of the host pack, in named_tensors() order."""
    import torch
    from mzba.agent import PackedNets
    from mzba.refresh import named_tensors
    from test_gpu_refresh import _cfg, _state
    mcfg, dd = _cfg(name)
    pack = PackedNets(_state(mcfg, 3), mcfg, dtype, "cuda", dd)
    out = []
    for path, t in named_tensors(pack).items():
        raw = t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()
        out.append([path, str(t.dtype), t.numel(), hashlib.sha256(raw).hexdigest()])
    return out


@pytest.mark.parametrize("name,dtype", CASES)
def test_host_pack_matches_recorded_hashes(name, dtype):
    want = json.load(open(FIXTURE))[f"{name}/{dtype}"]
    got = _hashes(name, dtype)
    assert [g[:3] for g in got] == [w[:3] for w in want]  # paths in order, dtypes, sizes
    bad = [g[0] for g, w in zip(got, want) if g[3] != w[3]]
    print(f"{name}/{dtype}: {len(got)} tensors, {len(bad)} hashes differ {bad}")
    assert len(got) > 20 and not bad


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_gpu_pack_golden.py --write   (on the commit before a packer change)")
    root = os.path.dirname(HERE)
    sys.path[:0] = [root, os.path.join(root, "muzero-breakout_amd")]
    rec = {f"{n}/{d}": _hashes(n, d) for n, d in CASES}
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print({k: len(v) for k, v in rec.items()})
