"""Pure-numpy restatement of the geometric self-ensemble (include/midd.h: THE GEOMETRY, mi_dihedral_views, mi_dihedral_reduce,
mi_dihedral_quantiles): the eight flip / rotate views of an image as array operations, the aligned members as unview of every
view, and over them the fixed arithmetic of tests/ensemble_reference.py and tests/quantile_reference.py.  The device kernels are
held to this bit for bit (tests/test_gpu_self_ensemble.py)."""
import numpy as np

from tests import ensemble_reference as eref
from tests import quantile_reference as qref

FLIPS, D4 = (0, 1, 2, 3), (0, 1, 2, 3, 4, 5, 6, 7)


def view(x, g):
    """View g = 4 t + 2 fy + fx of x [..., H, W]: swap the last two axes if t, then reverse the rows if fy, the columns if fx."""
    assert 0 <= g <= 7
    u = np.swapaxes(x, -1, -2) if g & 4 else x
    if g & 2:
        u = u[..., ::-1, :]
    if g & 1:
        u = u[..., :, ::-1]
    return np.ascontiguousarray(u)


def unview(y, g):
    """The inverse: reverse the columns if fx, the rows if fy, then swap the axes if t."""
    assert 0 <= g <= 7
    u = y
    if g & 1:
        u = u[..., :, ::-1]
    if g & 2:
        u = u[..., ::-1, :]
    if g & 4:
        u = np.swapaxes(u, -1, -2)
    return np.ascontiguousarray(u)


def views(images, codes):
    """images [B, C, H, W] -> [B, G, C, Hv, Wv] (codes that transpose need H == W, so every view has one shape)."""
    return np.stack([np.stack([view(img, g) for g in codes]) for img in images])


def members(view_outputs, codes):
    """view_outputs [B, G, C, Hv, Wv], view k in its own frame -> the aligned members [B, G, C, H, W]."""
    return np.stack([np.stack([unview(v[k], g) for k, g in enumerate(codes)]) for v in view_outputs])


def reduce(view_outputs, codes):
    """-> (mean, std or None, samples): tests/ensemble_reference.reduce over the aligned members, in list order."""
    m = members(np.asarray(view_outputs, np.float32), codes)
    mean, std = eref.reduce(m)
    return mean, std, m


def quantiles(view_outputs, codes, q):
    return qref.quantiles(members(np.asarray(view_outputs, np.float32), codes), q)
