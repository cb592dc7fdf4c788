"""The cross-spectrum of include/midd.h (THE CROSS SPECTRUM) restated in numpy, operation for operation: the device is held to
these bits (tests/test_gpu_cross_spectrum.py), and this file is held to float64 numpy.fft and to known answers
(tests/test_cross_spectrum_cpu.py).  What the section shares with THE NOISE POWER SPECTRUM is imported from tests/nps_reference.py.
Every float32 / float64 numpy operation below is one IEEE operation rounded to nearest; sums that have an order are explicit loops."""
from typing import NamedTuple

import numpy as np

from .nps_reference import CHUNK, bitrev, canonical_nan, cut_rois, detrend_window, fft_pass, radial_profile

QUANTITIES = ("sxx", "syy", "sxy_re", "sxy_im")


def packed_transform(dx, dy):
    """[n, R, R] float32 twice -> (re, im) of Z = DFT2(dx + i dy), [n, v, u] float32: every row, then every column."""
    n, R, _ = dx.shape
    br = bitrev(R)
    re = np.ascontiguousarray(dx[:, br][:, :, br])                   # stored at [bitrev(y)][bitrev(x)]
    im = np.ascontiguousarray(dy[:, br][:, :, br])
    re, im = fft_pass(re, im, R)                                     # rows
    cr, ci = np.ascontiguousarray(re.transpose(0, 2, 1)), np.ascontiguousarray(im.transpose(0, 2, 1))
    cr, ci = fft_pass(cr, ci, R)                                     # all R columns: [n, u, v]
    return cr.transpose(0, 2, 1), ci.transpose(0, 2, 1)


def separate(re, im):
    """The separation on the half plane: Z [n, R, R] float32 -> four double arrays [n, R, R/2+1]."""
    R = re.shape[-1]
    NC = R // 2 + 1
    mv, mu = (R - np.arange(R)) % R, (R - np.arange(NC)) % R
    x1, y1 = re[:, :, :NC].astype(np.float64), im[:, :, :NC].astype(np.float64)
    x2, y2 = re[:, mv][:, :, mu].astype(np.float64), im[:, mv][:, :, mu].astype(np.float64)
    n1 = x1 * x1 + y1 * y1
    n2 = x2 * x2 + y2 * y2
    c = x1 * x2 - y1 * y2
    s = x1 * y2 + y1 * x2
    nn, c2 = n1 + n2, 2.0 * c
    return (nn + c2) / 4.0, (nn - c2) / 4.0, s / 2.0, (n1 - n2) / 4.0


def full_plane_signed(half, sign):
    """[R, R/2+1] -> [R, R]: entry ((R - v) % R, R - u) = sign * entry (v, u) for 0 < u < R/2."""
    R = half.shape[-2]
    out = np.empty((R, R), half.dtype)
    out[:, :R // 2 + 1] = half
    v = (R - np.arange(R)) % R
    for u in range(R // 2 + 1, R):
        out[:, u] = half[v, R - u] if sign > 0 else -half[v, R - u]
    return out


class Xs(NamedTuple):
    planes: np.ndarray             # float64 [4, B, C, R, R]: sxx, syy, sxy_re, sxy_im
    radial: np.ndarray             # float64 [4, B, C, R/2+1]
    radial_count: np.ndarray       # int64 [R/2+1]
    rois_used: np.ndarray          # int64 [B, C]
    rois_skipped: np.ndarray       # int64 [B, C]


def cross_spectrum(x, y, roi=64, step=None, detrend="plane", window=None, exclude_axes=False):
    """x [B, Kx, C, H, W], y [B, Ky, C, H, W] float32 with Kx, Ky in {K, 1}; window a float32 [roi] table or None."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    B, Kx, C, H, W = x.shape
    Ky = y.shape[1]
    K = max(Kx, Ky)
    assert Kx in (K, 1) and Ky in (K, 1) and x.shape[:1] + x.shape[2:] == y.shape[:1] + y.shape[2:]
    R, S = roi, roi // 2 if step is None else step
    if window is None:
        sw = np.float64(R) * np.float64(R)
    else:
        q = np.float64(0.0)
        for wi in np.asarray(window, np.float32):
            q = q + np.float64(wi) * np.float64(wi)
        sw = q * q
    NC = R // 2 + 1
    planes = np.empty((4, B, C, R, R), np.float64)
    radial = np.empty((4, B, C, NC), np.float64)
    used, skipped = np.zeros((B, C), np.int64), np.zeros((B, C), np.int64)
    _, count = radial_profile(np.zeros((R, R)), exclude_axes)
    for bi in range(B):
        for c in range(C):
            fx = np.broadcast_to(x[bi, :, c], (K, H, W))             # one realisation is broadcast over the members
            fy = np.broadcast_to(y[bi, :, c], (K, H, W))
            rx, ry = cut_rois(fx, R, S), cut_rois(fy, R, S)
            ok = np.isfinite(rx).all(axis=(1, 2)) & np.isfinite(ry).all(axis=(1, 2))
            Q = np.zeros((4, len(rx), R, NC), np.float64)
            if ok.any():
                re, im = packed_transform(detrend_window(rx[ok], detrend, window), detrend_window(ry[ok], detrend, window))
                Q[:, ok] = separate(re, im)
            total = np.zeros((4, R, NC), np.float64)
            for c0 in range(0, len(rx), CHUNK):
                part = np.zeros((4, R, NC), np.float64)
                for n in range(c0, min(c0 + CHUNK, len(rx))):
                    if ok[n]:
                        part = part + Q[:, n]
                total = total + part
            used[bi, c], skipped[bi, c] = ok.sum(), (~ok).sum()
            for q in range(4):
                if used[bi, c]:
                    planes[q, bi, c] = full_plane_signed(total[q] / (np.float64(used[bi, c]) * sw), -1 if q == 3 else 1)
                    radial[q, bi, c], _ = radial_profile(planes[q, bi, c], exclude_axes)
                else:
                    planes[q, bi, c], radial[q, bi, c] = np.nan, np.nan
    return Xs(canonical_nan(planes), canonical_nan(radial), count, used, skipped)


def float64_spectra(x, y, roi, step, detrend, window):
    """The four planes [4, B, C, R, R] from float64 numpy.fft.fft2 of the same detrended, windowed fp32 ROIs (all finite)."""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    B, Kx, C, H, W = x.shape
    K = max(Kx, y.shape[1])
    R = roi
    sw = np.float64(R * R) if window is None else np.sum(np.asarray(window, np.float64) ** 2) ** 2
    out = np.empty((4, B, C, R, R), np.float64)
    for bi in range(B):
        for c in range(C):
            dx = detrend_window(cut_rois(np.broadcast_to(x[bi, :, c], (K, H, W)), R, step), detrend, window).astype(np.float64)
            dy = detrend_window(cut_rois(np.broadcast_to(y[bi, :, c], (K, H, W)), R, step), detrend, window).astype(np.float64)
            X, Y = np.fft.fft2(dx), np.fft.fft2(dy)
            sxy = (X * np.conj(Y)).mean(axis=0) / sw
            out[0, bi, c], out[1, bi, c] = (np.abs(X) ** 2).mean(axis=0) / sw, (np.abs(Y) ** 2).mean(axis=0) / sw
            out[2, bi, c], out[3, bi, c] = sxy.real, sxy.imag
    return out


def gate_errors(planes, exact):
    """sum |S - S*| / sum (sxx* + syy*) per quantity: the float64 gate's left-hand side (include/midd.h: Accuracy)."""
    norm = (exact[0] + exact[1]).sum()
    return [float(np.abs(planes[q] - exact[q]).sum() / norm) for q in range(4)]
