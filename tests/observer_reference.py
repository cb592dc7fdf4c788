"""The numpy restatement of THE CHANNEL RESPONSES (include/midd.h; mi_channel_responses) and of the input rule of the detectability
study (DiffusionDenoiser.detectability), for the observer tests.  Every double operation below is one numpy operation, rounded on
its own; nothing here comes from the package."""
import numpy as np

LANES = 64
QNAN64 = np.uint64(0x7FF8000000000000)


def rois(x, centres, R):
    """x [N, H, W], centres [L, 2] as (cy, cx) -> the ROIs [N, L, R * R] in x's dtype: rows cy - R // 2 .. + R - 1, likewise columns,
    flattened as p = y R + x.  An ROI that leaves the image is an error here as it is in the call."""
    N, H, W = x.shape
    out = np.empty((N, len(centres), R * R), x.dtype)
    for l, (cy, cx) in enumerate(np.asarray(centres).tolist()):
        y0, x0 = cy - R // 2, cx - R // 2
        assert 0 <= y0 and y0 + R <= H and 0 <= x0 and x0 + R <= W, (cy, cx, R, H, W)
        out[:, l] = x[:, y0:y0 + R, x0:x0 + R].reshape(N, R * R)
    return out


def ordered_dot(u, g):
    """u [C, P], g [..., P], float64 -> [..., C]: lane j = 0 .. 63 starts from 0 and adds u[p] * g[p] (the product rounded, then
    added) for p = j, j + 64, .. < P in increasing order; then the tree  for off = 32 .. 1: v[j] += v[j + off], j < off;  the root."""
    P = u.shape[-1]
    v = np.zeros(g.shape[:-1] + (u.shape[0], LANES), np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, P, LANES):
            m = min(LANES, P - lo)
            prod = u[..., :, lo:lo + m] * g[..., None, lo:lo + m]
            v[..., :m] = v[..., :m] + prod
        off = LANES // 2
        while off:
            v[..., :off] = v[..., :off] + v[..., off:2 * off]
            off //= 2
    return np.ascontiguousarray(v[..., 0])


def responses(x, centres, channels):
    """x float32 [N, H, W], centres [L, 2], channels float64 [C, R, R] -> (values float64 [N, L, C], invalid bool [N, L]): an ROI with a
    pixel that is not finite is invalid and the canonical quiet NaN in every channel."""
    C, R = channels.shape[:2]
    g32 = rois(np.asarray(x, np.float32), centres, R)
    invalid = ~np.isfinite(g32).all(axis=-1)
    values = ordered_dot(np.ascontiguousarray(channels, np.float64).reshape(C, R * R), g32.astype(np.float64))
    values.view(np.uint64)[invalid] = QNAN64
    return values, invalid


def study_noisy(clean, eps, sigma):
    """The study's input rule in float32: clamp(clean + float32(sigma) * eps, 0, 1), one multiplication, one addition, the clamp."""
    clean, eps = np.asarray(clean, np.float32), np.asarray(eps, np.float32)
    return np.clip(clean + np.float32(sigma) * eps, np.float32(0.0), np.float32(1.0)).astype(np.float32)


def planes(N, H, W, seed):
    """Test planes in [0, 1) with a smooth part and noise, float32."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    base = 0.5 + 0.3 * np.sin(0.37 * yy + 0.11 * xx)
    return (base[None] * 0.8 + 0.2 * rng.random((N, H, W))).astype(np.float32)


def templates(C, R, seed):
    """Test channels: signed float64 values of mixed magnitude, so that the order of the sum shows in the low bits."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((C, R, R)) * np.exp(rng.uniform(-3.0, 3.0, (C, R, R)))
