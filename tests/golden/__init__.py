"""Golden fixtures: arrays recorded from the reference (make_golden*.py).  A fixture is one ``NAME.npz``, or, when its
arrays would make a file larger than 1 MiB, ``NAME.part0.npz``, ``NAME.part1.npz``, ... with the arrays split between
them; ``load(NAME)`` reads either form the same way."""
import glob
import io
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PART_LIMIT = 1000 << 10                 # bytes per written file, below the 1 MiB limit of a committed file


class Fixture(dict):
    """The arrays of a multi-part fixture, in the order they were saved; ``.files`` as on ``np.load``'s result."""

    @property
    def files(self):
        return list(self)


def load(name):
    path = os.path.join(HERE, name + ".npz")
    if os.path.exists(path):
        return np.load(path)
    parts = glob.glob(os.path.join(HERE, glob.escape(name) + ".part*.npz"))
    if not parts:
        raise FileNotFoundError(path)
    out = Fixture()
    for p in sorted(parts, key=lambda p: int(p.rsplit(".part", 1)[1][:-len(".npz")])):
        with np.load(p) as z:
            out.update((k, z[k]) for k in z.files)
    return out


def _compressed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def save(name, arrays, limit=PART_LIMIT):
    """np.savez_compressed to NAME.npz, or, above `limit` bytes, to NAME.partK.npz files that keep the arrays' order."""
    for old in glob.glob(os.path.join(HERE, glob.escape(name) + ".part*.npz")) + glob.glob(os.path.join(HERE, name + ".npz")):
        os.remove(old)
    if _compressed_size(arrays) <= limit:
        np.savez_compressed(os.path.join(HERE, name + ".npz"), **arrays)
        return
    parts, cur = [], {}
    for k, v in arrays.items():
        if cur and _compressed_size({**cur, k: v}) > limit:
            parts.append(cur)
            cur = {}
        cur[k] = v
    parts.append(cur)
    for i, part in enumerate(parts):
        if _compressed_size(part) > limit:
            raise ValueError(f"{name}: array {next(iter(part))} alone exceeds {limit} bytes compressed")
        np.savez_compressed(os.path.join(HERE, f"{name}.part{i}.npz"), **part)
