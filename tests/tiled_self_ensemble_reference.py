"""Pure-numpy restatement of the tiled self-ensemble (include/midd.h: TILED SELF-ENSEMBLE, mi_tile_blend_unview_reduce,
mi_tile_blend_unview_quantiles): the flip / rotate views for H != W, "a view's tiles are the tiles of the viewed image", and the
composition of the existing restatements -- tests/tiled_reference.py (blend, in the view's frame), the un-view, then
tests/ensemble_reference.py / tests/quantile_reference.py.  The device kernels are held to this bit for bit
(tests/test_gpu_tiled_self_ensemble.py)."""
import numpy as np

from tests import ensemble_reference as eref
from tests import quantile_reference as qref
from tests import self_ensemble_reference as sref
from tests import tiled_reference as tref

FLIPS, D4 = sref.FLIPS, sref.D4


def view(x, g):
    """View g = 4 t + 2 fy + fx of x [..., H, W], any H and W.  The array form of tests/self_ensemble_reference.py (swap the axes
    if t, reverse the rows if fy, the columns if fx) IS the general form of the header:
    t = 1: view(x)[p][q] = x[fx ? H-1-q : q][fy ? W-1-p : p], a W x H plane (view_entry restates that entry by entry)."""
    return sref.view(x, g)


def unview(v, g):
    """The inverse: unview(v)[y][x] = v[p][q] with p = fy ? W-1-x : x, q = fx ? H-1-y : y for t = 1."""
    return sref.unview(v, g)


def view_entry(x, g):
    """view(x, g) of a 2-D array written out entry by entry from the header's formulas (slow; the CPU test holds view() to it)."""
    H, W = x.shape
    t, fy, fx = g & 4, g & 2, g & 1
    if not t:
        return np.array([[x[H - 1 - p if fy else p][W - 1 - q if fx else q] for q in range(W)] for p in range(H)], x.dtype)
    return np.array([[x[H - 1 - q if fx else q][W - 1 - p if fy else p] for q in range(H)] for p in range(W)], x.dtype)


def unview_entry(v, g, H, W):
    t, fy, fx = g & 4, g & 2, g & 1
    if not t:
        return np.array([[v[H - 1 - y if fy else y][W - 1 - x if fx else x] for x in range(W)] for y in range(H)], v.dtype)
    return np.array([[v[W - 1 - x if fy else x][H - 1 - y if fx else y] for x in range(W)] for y in range(H)], v.dtype)


def frame(H, W, tile, overlap, g):
    """(Hv, Wv, (th, tw), (oy, ox)) of view g's frame: a transposing code swaps the axes of the image AND of the tiling."""
    (th, tw), (oy, ox) = tile, overlap
    if g & 4:
        assert th == tw and oy == ox, "codes 4 .. 7 need a square tile and overlap"
        return W, H, (tw, th), (ox, oy)
    return H, W, (th, tw), (oy, ox)


def view_tiles(images, tile, overlap, codes):
    """images [B, C, H, W] -> tiles [G, B, K, C, th, tw]: slice k holds the tiles of view(images, codes[k]), cut in THAT frame."""
    return np.stack([tref.extract(view(images, g), *frame(images.shape[2], images.shape[3], tile, overlap, g)[2:]) for g in codes])


def members(tiles, H, W, overlap, codes):
    """tiles [G, B, K, C, th, tw] -> the aligned blended members [B, G, C, H, W]: tiled_reference.blend in every view's frame, un-viewed."""
    th, tw = tiles.shape[4], tiles.shape[5]
    out = []
    for k, g in enumerate(codes):
        Hv, Wv, _, ov = frame(H, W, (th, tw), overlap, g)
        out.append(unview(tref.blend(tiles[k], Hv, Wv, ov), g))
    return np.ascontiguousarray(np.stack(out, axis=1))


def reduce(tiles, H, W, overlap, codes):
    """-> (mean, std or None, samples): tests/ensemble_reference.reduce over the aligned blended members, in list order."""
    m = members(np.asarray(tiles, np.float32), H, W, overlap, codes)
    mean, std = eref.reduce(m)
    return mean, std, m


def quantiles(tiles, H, W, overlap, codes, q):
    return qref.quantiles(members(np.asarray(tiles, np.float32), H, W, overlap, codes), q)
