"""The noise power spectrum of include/midd.h (THE NOISE POWER SPECTRUM) restated in numpy, operation for operation: the device is
held to these bits (tests/test_gpu_nps.py), and this file is held to float64 numpy.fft and to known answers (tests/test_nps_cpu.py).
Every float32 / float64 numpy operation below is one IEEE operation rounded to nearest; sums that have an order are explicit loops."""
import math
from typing import NamedTuple

import numpy as np

CHUNK = 16                                   # ROIs per chunk of the summation order
QNAN = 0x7FF8000000000000
DETREND = {"none": 0, "mean": 1, "plane": 2}


def twiddles(R):
    """T[t] = exp(-2 pi i t / R), t < R/2: double precision, angle 2.0 * pi * t / R left to right, rounded to fp32."""
    tc = np.array([math.cos(2.0 * math.pi * t / R) for t in range(R // 2)], np.float64).astype(np.float32)
    ts = np.array([-math.sin(2.0 * math.pi * t / R) for t in range(R // 2)], np.float64).astype(np.float32)
    return tc, ts


def hann(R):
    """The periodic Hann window 0.5 - 0.5 cos(2 pi n / R), computed in double and rounded to fp32."""
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * n / R) for n in range(R)], np.float64).astype(np.float32)


def bitrev(R):
    bits = R.bit_length() - 1
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(R)])


def fft_pass(re, im, R):
    """Radix-2 decimation in time along the last axis of (re, im), whose input is already in bit-reversed order."""
    tc, ts = twiddles(R)
    lead = re.shape[:-1]
    for s in range(1, R.bit_length()):
        half = 1 << (s - 1)
        wr, wi = tc[::R >> s][:half], ts[::R >> s][:half]
        r4, i4 = re.reshape(lead + (R >> s, 2, half)), im.reshape(lead + (R >> s, 2, half))
        ar, ai, xr, xi = r4[..., 0, :], i4[..., 0, :], r4[..., 1, :], i4[..., 1, :]
        tr = wr * xr - wi * xi
        ti = wr * xi + wi * xr
        re = np.stack([ar + tr, ar - tr], axis=-2).reshape(lead + (R,))
        im = np.stack([ai + ti, ai - ti], axis=-2).reshape(lead + (R,))
    return re, im


def cut_rois(f, R, S):
    """f [K, H, W] -> [K * ny * nx, R, R] in (member, iy, ix) order."""
    K, H, W = f.shape
    ny, nx = (H - R) // S + 1, (W - R) // S + 1
    out = np.empty((K, ny, nx, R, R), f.dtype)
    for iy in range(ny):
        for ix in range(nx):
            out[:, iy, ix] = f[:, iy * S:iy * S + R, ix * S:ix * S + R]
    return out.reshape(K * ny * nx, R, R)


def detrend_window(rois, detrend, window):
    """Stages 1 and 2 on finite ROIs [n, R, R] float32 -> float32."""
    n, R, _ = rois.shape
    d = rois
    if detrend != "none":
        f64 = rois.astype(np.float64)
        c = np.arange(R, dtype=np.float64) - 0.5 * (R - 1)
        s0, s1 = np.zeros((n, R)), np.zeros((n, R))
        for x in range(R):
            s0 = s0 + f64[:, :, x]
            s1 = s1 + c[x] * f64[:, :, x]
        t0, tx, ty = np.zeros(n), np.zeros(n), np.zeros(n)
        for y in range(R):
            t0 = t0 + s0[:, y]
            tx = tx + s1[:, y]
            ty = ty + c[y] * s0[:, y]
        m = t0 / np.float64(R * R)
        den = np.float64(R) * (np.float64(R) * (np.float64(R) * R - 1.0) / 12.0)
        ax = tx / den if detrend == "plane" else np.zeros(n)
        ay = ty / den if detrend == "plane" else np.zeros(n)
        t = (m[:, None, None] + ax[:, None, None] * c[None, None, :]) + ay[:, None, None] * c[None, :, None]
        d = (f64 - t).astype(np.float32)
    if window is not None:
        w = np.asarray(window, np.float32)
        d = (d * w[None, :, None]) * w[None, None, :]
    return d


def periodograms(d):
    """Stage 3 on [n, R, R] float32: the half plane P [n, R, R/2+1] in double."""
    n, R, _ = d.shape
    br = bitrev(R)
    re = np.ascontiguousarray(d[:, br][:, :, br])                    # stored at [bitrev(y)][bitrev(x)]: reading there is the same permutation
    im = np.zeros_like(re)
    re, im = fft_pass(re, im, R)                                     # rows
    NC = R // 2 + 1
    cr, ci = np.ascontiguousarray(re[:, :, :NC].transpose(0, 2, 1)), np.ascontiguousarray(im[:, :, :NC].transpose(0, 2, 1))
    cr, ci = fft_pass(cr, ci, R)                                     # columns 0 .. R/2: [n, u, v]
    cr, ci = cr.astype(np.float64), ci.astype(np.float64)
    return (cr * cr + ci * ci).transpose(0, 2, 1)


def full_plane(half):
    """[..., R, R/2+1] -> [..., R, R] by P[v][u] = P[(R - v) % R][R - u]."""
    R = half.shape[-2]
    out = np.empty(half.shape[:-1] + (R,), half.dtype)
    out[..., :R // 2 + 1] = half
    v = (R - np.arange(R)) % R
    for u in range(R // 2 + 1, R):
        out[..., u] = half[..., v, R - u]
    return out


def radial_bins(R):
    """[R, R] int: the bin of every entry by the integer rule (bins beyond R/2 included)."""
    fr = np.where(np.arange(R) < R // 2, np.arange(R), np.arange(R) - R)
    d4 = 4 * (fr[None, :] ** 2 + fr[:, None] ** 2)
    bins = np.full((R, R), -1)
    for r in range(R):
        lo = (2 * r - 1) ** 2 if r else 0
        bins[(d4 >= lo) & (d4 < (2 * r + 1) ** 2)] = r
    return bins, fr


def radial_profile(nps, exclude_axes):
    R = nps.shape[-1]
    bins, fr = radial_bins(R)
    keep = np.ones((R, R), bool)
    if exclude_axes:
        keep &= (fr[None, :] != 0) & (fr[:, None] != 0)
    radial = np.empty(R // 2 + 1, np.float64)
    count = np.zeros(R // 2 + 1, np.int64)
    for r in range(R // 2 + 1):
        s = np.float64(0.0)
        for v, u in zip(*np.nonzero((bins == r) & keep)):           # row-major
            s = s + nps[v, u]
            count[r] += 1
        radial[r] = s / np.float64(count[r]) if count[r] else np.nan
    return radial, count


class Nps(NamedTuple):
    nps: np.ndarray                # float64 [B, C, R, R]
    radial: np.ndarray             # float64 [B, C, R/2+1]
    radial_count: np.ndarray       # int64 [R/2+1]
    rois_used: np.ndarray          # int64 [B, C]
    rois_skipped: np.ndarray       # int64 [B, C]


def canonical_nan(x):
    x = x.copy()
    x.view(np.uint64)[np.isnan(x)] = QNAN
    return x


def noise_power_spectrum(a, b=None, roi=64, step=None, detrend="plane", window=None, scale=1.0, exclude_axes=False):
    """a [B, K, C, H, W] float32, b [B, C, H, W] float32 or None, window a float32 [roi] table or None."""
    a = np.asarray(a, np.float32)
    B, K, C, H, W = a.shape
    R, S = roi, roi // 2 if step is None else step
    with np.errstate(invalid="ignore"):
        f = a if b is None else a - np.asarray(b, np.float32)[:, None]
    if window is None:
        sw = np.float64(R) * np.float64(R)
    else:
        q = np.float64(0.0)
        for wi in np.asarray(window, np.float32):
            q = q + np.float64(wi) * np.float64(wi)
        sw = q * q
    NC = R // 2 + 1
    nps = np.empty((B, C, R, R), np.float64)
    radial = np.empty((B, C, NC), np.float64)
    used, skipped = np.zeros((B, C), np.int64), np.zeros((B, C), np.int64)
    count = np.zeros(NC, np.int64)
    for bi in range(B):
        for c in range(C):
            rois = cut_rois(f[bi, :, c], R, S)
            ok = np.isfinite(rois).all(axis=(1, 2))
            P = np.zeros((len(rois), R, NC), np.float64)
            if ok.any():
                P[ok] = periodograms(detrend_window(rois[ok], detrend, window))
            total = np.zeros((R, NC), np.float64)
            for c0 in range(0, len(rois), CHUNK):
                part = np.zeros((R, NC), np.float64)
                for n in range(c0, min(c0 + CHUNK, len(rois))):
                    if ok[n]:
                        part = part + P[n]
                total = total + part
            used[bi, c], skipped[bi, c] = ok.sum(), (~ok).sum()
            if used[bi, c]:
                nps[bi, c] = full_plane((np.float64(scale) * total) / (np.float64(used[bi, c]) * sw))
                radial[bi, c], count = radial_profile(nps[bi, c], exclude_axes)
                radial[bi, c] = canonical_nan(radial[bi, c])
            else:
                nps[bi, c], radial[bi, c] = np.nan, np.nan
                _, count = radial_profile(np.zeros((R, R)), exclude_axes)
    return Nps(canonical_nan(nps), canonical_nan(radial), count, used, skipped)


def error_bound(R):
    """2 rho + rho^2 with rho = t eta / (1 - t eta) + 3u: Higham, Accuracy and Stability of Numerical Algorithms, Theorem 24.2, for the
    two radix-2 passes (t = 2 log2 R) with correctly rounded twiddles (mu = u), plus 3u for the subtraction, the detrend rounding and
    the window products."""
    u = 2.0 ** -24
    g4 = 4 * u / (1 - 4 * u)
    eta = u + g4 * (math.sqrt(2.0) + u)
    t = 2 * (R.bit_length() - 1)
    rho = t * eta / (1 - t * eta) + 3 * u
    return 2 * rho + rho * rho


def philox_field(shape, seed, ramp=0.0):
    """Seeded Philox normal noise (sigma 0.05 around 0.5) as float32, optionally on a ramp along both axes."""
    rng = np.random.Generator(np.random.Philox(seed))
    x = 0.5 + 0.05 * rng.standard_normal(shape)
    if ramp:
        H, W = shape[-2:]
        x = x + ramp * (np.arange(W)[None, :] / W + 0.5 * np.arange(H)[:, None] / H)
    return x.astype(np.float32)
