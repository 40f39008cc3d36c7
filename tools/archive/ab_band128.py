"""Band kernel A/B at the representation's Cout 128 shapes (64->128 stem, 128->128) and the Cout 256
shapes, isolated launches timed with HIP events (MZBA_LIB selects the build). usage: python tools/ab_band128.py
The A/B build (the Cout 128 convs on the per-shift loops, -DBAND_ONEPASS128=0) needs
profiles/r02/b128/band_per_shift_loops_retired.patch put back on a copy of the tree (patch -R -p1)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "muzero-breakout_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_conv import run  # noqa: E402

for cin, cout in ((64, 128), (128, 128), (128, 256), (256, 256)):
    print(json.dumps({"lib": os.path.basename(os.environ.get("MZBA_LIB", "libmzba.so")), **run(4096, 16, 20, cin, cout, 3, "band", iters=30)}))
