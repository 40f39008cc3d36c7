"""Golden fixtures stored in parts: a large .npz under tests/golden/ is kept as STEM.00.npz, STEM.01.npz, ...
(every committed file below 1 MiB), the keys of all parts together being the fixture."""
import glob
import os

import numpy as np

PART_BYTES = 900 * 1024  # target size of one part on disk


class NpzParts:
    """Read-only view over the parts of one fixture with np.load's interface as the tests use it: `z[key]`,
    `z.files`, `key in z`."""

    def __init__(self, golden_dir, stem):
        paths = sorted(glob.glob(os.path.join(golden_dir, stem + ".[0-9][0-9].npz")))
        if not paths:
            raise FileNotFoundError(f"no parts {stem}.NN.npz under {golden_dir}")
        self._where, self.files = {}, []
        for p in paths:
            z = np.load(p)
            for k in z.files:
                if k in self._where:
                    raise ValueError(f"{k} is in two parts of {stem}")
                self._where[k] = z
                self.files.append(k)

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where

    def keys(self):
        return list(self.files)


def load_npz_parts(golden_dir, stem):
    return NpzParts(golden_dir, stem)


def save_npz_parts(golden_dir, stem, arrays, part_bytes=PART_BYTES):
    """Write `arrays` (name -> ndarray, order kept) as compressed parts of at most about part_bytes each; returns
    the paths. A part is closed when the next array would take it past the target (sizes are measured on a
    compressed copy of the array alone, plus the archive's per-entry overhead)."""
    import io
    groups, cur, size = [], {}, 0
    for k, a in arrays.items():
        buf = io.BytesIO()
        np.savez_compressed(buf, **{k: a})
        n = buf.getbuffer().nbytes
        if cur and size + n > part_bytes:
            groups.append(cur)
            cur, size = {}, 0
        cur[k] = a
        size += n
    if cur:
        groups.append(cur)
    paths = []
    for i, g in enumerate(groups):
        paths.append(os.path.join(golden_dir, f"{stem}.{i:02d}.npz"))
        np.savez_compressed(paths[-1], **g)
    return paths
