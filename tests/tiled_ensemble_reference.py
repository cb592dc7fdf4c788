"""numpy restatement of the reduction of an ensemble of tiled runs (include/midd.h: mi_tile_blend_reduce): the blend of
tests/tiled_reference.py per member, then the reduce of tests/ensemble_reference.py over the blended members.  Float64
throughout, every operation rounded on its own: the yardstick, not an emulation of the device."""
import numpy as np

from tests import ensemble_reference, tiled_reference


def blend_reduce(tiles, H, W, overlap):
    """tiles float32 [members, B, ny * nx, C, th, tw] -> (mean [B, C, H, W], std [B, C, H, W] or None for one member,
    samples [B, members, C, H, W]), all float32.  ``overlap`` is (oy, ox)."""
    t = np.asarray(tiles)
    assert t.dtype == np.float32 and t.ndim == 6
    samples = np.stack([tiled_reference.blend(t[m], H, W, overlap) for m in range(t.shape[0])], axis=1)
    mean, std = ensemble_reference.reduce(samples)
    return mean, std, samples
