"""Pure-numpy restatement of the three specifications behind the denoising-loss calls (include/midd.h: THE FORWARD NOISE, THE
NOISING, THE DENOISING LOSS).

fp32 arithmetic is numpy float32, one operation per line, so that every operation is rounded on its own as the header demands; the
sums are float64 in the header's order.  The forward noise z is float64, as tests/step_noise_reference.py keeps the step noise: it is
the yardstick the device's fp32 values are compared with, not an emulation of them -- the bit-for-bit checks of x_t and of the loss
therefore start from an eps tensor (the device's export, or any other)."""
import numpy as np

from tests import step_noise_reference as sn

PATCH = 32
F = np.float32


def forward_noise(seed, shape, sample_offset=0, draw=0, sample_index=None, draws=None):
    """float64 [B, C, H, W]: z of (seed, sample_offset + b, draw, element) -- the step-noise generator with the counter words
    (element, sample, 0x80000000 | draw, 0) and no 0.5 factor."""
    B, C, H, W = shape
    e = np.arange(C * H * W, dtype=np.uint64)
    out = np.empty((B, C * H * W), np.float64)
    for b in range(B):
        d = draw if draws is None else draws[b]
        assert 0 <= d < 2 ** 31
        out[b] = sn.normal(seed, (sample_offset + b) if sample_index is None else sample_index[b], 0x80000000 | d, e)
    return out.reshape(B, C, H, W)


def coefficients(t, alpha_hat):
    """(a, s) float32 [B]: sqrtf(alpha_hat[t]), sqrtf(1 - alpha_hat[t]), host fp32 in the reference's order."""
    ah = np.asarray(alpha_hat, F)[np.asarray(t, np.int64)]
    return np.sqrt(ah), np.sqrt(F(1.0) - ah)


def noise_images(clean, eps, t, alpha_hat):
    """x_t = a*x + s*eps: two products and one sum, each rounded once."""
    a, s = coefficients(t, alpha_hat)
    a, s = a[:, None, None, None], s[:, None, None, None]
    pa = a * np.asarray(clean, F)
    ps = s * np.asarray(eps, F)
    return pa + ps


def _clamp(v, lo, hi):
    """torch.clamp: a NaN stays a NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(v < F(lo), F(lo), np.where(v > F(hi), F(hi), v)).astype(F)


def _sobel_magnitude(u):
    """u float32 [..., H, W] -> m(u), zero padding, the six non-zero taps of each kernel in row-major order, left to right."""
    pad = np.zeros(u.shape[:-2] + (u.shape[-2] + 2, u.shape[-1] + 2), F)
    pad[..., 1:-1, 1:-1] = u
    H, W = u.shape[-2:]
    n = lambda i, j: pad[..., i:i + H, j:j + W]
    two = F(2.0)
    ex = -n(0, 0)
    ex = ex + n(0, 2)
    ex = ex - two * n(1, 0)
    ex = ex + two * n(1, 2)
    ex = ex - n(2, 0)
    ex = ex + n(2, 2)
    ey = -n(0, 0)
    ey = ey - two * n(0, 1)
    ey = ey - n(0, 2)
    ey = ey + n(2, 0)
    ey = ey + two * n(2, 1)
    ey = ey + n(2, 2)
    xx = ex * ex
    yy = ey * ey
    ss = xx + yy
    ss = ss + F(1e-8)
    return np.sqrt(ss)


def pixel_maps(clean, x_t, eps, eps_pred, t, alpha_hat, clamp_eps):
    """(q, g, p) float32 [B, C, H, W] of THE DENOISING LOSS."""
    clean, x_t, eps, eps_pred = (np.asarray(v, F) for v in (clean, x_t, eps, eps_pred))
    a, s = coefficients(t, alpha_hat)
    a, s = a[:, None, None, None], s[:, None, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        e = _clamp(eps_pred, -5.0, 5.0) if clamp_eps else eps_pred
        d = e - eps
        q = d * d
        se = s * e
        num = x_t - se
        p = _clamp(num / a, 0.0, 1.0)
        mp = _sobel_magnitude(p)
        mc = _sobel_magnitude(clean)
        g = np.abs(mp - mc)
    return q.astype(F), g.astype(F), p


def ordered_sum(v):
    """float64 [B]: the sum of v float32 [B, C, H, W] in the header's one order -- 32 x 32 patches; inside a patch lane j owns column
    j % 32 of rows j / 32 + 8 k, k = 0 .. 3 in that order, then the tree v[j] += v[j + off], off = 128 .. 1; the patch sums of a sample
    one by one in (channel, patch row, patch column) order."""
    B, C, H, W = v.shape
    ty, tx = -(-H // PATCH), -(-W // PATCH)
    pad = np.zeros((B, C, ty * PATCH, tx * PATCH), np.float64)
    pad[:, :, :H, :W] = v
    # [B, C, ty, k, ly0, tx, lx] -> lanes [B, C, ty, tx, ly0 * 32 + lx], summed over k in order
    r = pad.reshape(B, C, ty, 4, 8, tx, PATCH).transpose(0, 1, 2, 5, 3, 4, 6)
    with np.errstate(invalid="ignore"):
        lane = np.zeros(r.shape[:4] + (8, PATCH), np.float64)
        for k in range(4):
            lane = lane + r[:, :, :, :, k]
        lane = lane.reshape(B, C, ty, tx, 256)
        n = 256
        while n > 1:
            n //= 2
            lane = lane[..., :n] + lane[..., n:2 * n]
        patch = lane[..., 0].reshape(B, C * ty * tx)
        total = np.zeros(B, np.float64)
        for i in range(patch.shape[1]):
            total = total + patch[:, i]
    return total


def loss_terms(clean, x_t, eps, eps_pred, t, alpha_hat, clamp_eps, edge_weight):
    """-> (out float64 [B, 3] = (mse, edge, loss), (q, g, p))."""
    q, g, p = pixel_maps(clean, x_t, eps, eps_pred, t, alpha_hat, clamp_eps)
    count = np.float64(q[0].size)
    with np.errstate(invalid="ignore"):
        mse = ordered_sum(q) / count
        edge = ordered_sum(g) / count
        loss = mse + np.float64(edge_weight) * edge
    return np.stack([mse, edge, loss], axis=1), (q, g, p)
