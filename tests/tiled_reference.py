"""numpy restatement of tiled denoising (include/midd.h: mi_tile_geometry, mi_tile_extract, mi_tile_blend, mi_denoise_tiled):
the per-axis geometry, the integer ramp window and the blend in float64.  Nothing here imports the package."""
import numpy as np


def tile_count(L, T, O):
    """n = 1 if L == T, else max(2, ceil((L - O) / (T - O)))."""
    if L == T:
        return 1
    return max(2, -((L - O) // -(T - O)))


def origins(L, T, O):
    """o_i = (i * (L - T)) // (n - 1); a single tile starts at 0."""
    n = tile_count(L, T, O)
    if n == 1:
        return [0]
    return [(i * (L - T)) // (n - 1) for i in range(n)]


def window(T, O):
    """w(r) = min(r + 1, T - r, O + 1) for r in [0, T), as int64."""
    r = np.arange(T, dtype=np.int64)
    return np.minimum(np.minimum(r + 1, T - r), O + 1)


def extract(x, tile, overlap):
    """x [B, C, H, W] -> tiles [B, ny * nx, C, th, tw], k = ky * nx + kx (plain slicing)."""
    (th, tw), (oy, ox) = tile, overlap
    B, C, H, W = x.shape
    ys, xs = origins(H, th, oy), origins(W, tw, ox)
    out = np.empty((B, len(ys) * len(xs), C, th, tw), x.dtype)
    for ky, y0 in enumerate(ys):
        for kx, x0 in enumerate(xs):
            out[:, ky * len(xs) + kx] = x[:, :, y0:y0 + th, x0:x0 + tw]
    return out


def blend(tiles, H, W, overlap):
    """tiles [B, ny * nx, C, th, tw] -> float32 [B, C, H, W].  Per pixel, over the covering tiles in ascending (ky, kx), in
    float64 with every operation rounded on its own (numpy never fuses):  num += (wy * wx) * v;  den += wy * wx;  num / den."""
    oy, ox = overlap
    B, K, C, th, tw = tiles.shape
    ys, xs = origins(H, th, oy), origins(W, tw, ox)
    assert K == len(ys) * len(xs)
    wy, wx = window(th, oy), window(tw, ox)
    num = np.zeros((B, C, H, W), np.float64)
    den = np.zeros((H, W), np.float64)
    for ky, y0 in enumerate(ys):                      # ascending (ky, kx): every pixel meets its tiles in that order
        for kx, x0 in enumerate(xs):
            w = (wy[:, None] * wx[None, :]).astype(np.float64)
            num[:, :, y0:y0 + th, x0:x0 + tw] += w * tiles[:, ky * len(xs) + kx].astype(np.float64)
            den[y0:y0 + th, x0:x0 + tw] += w
    return (num / den).astype(np.float32)


def cover_counts(L, T, O):
    """How many tiles lie over every position of the axis."""
    c = np.zeros(L, np.int64)
    for o in origins(L, T, O):
        c[o:o + T] += 1
    return c
