"""The Welch cross-spectrum of two fields and what follows from it: the signal transfer and the Fourier ring correlation
(include/midd.h: THE CROSS SPECTRUM)."""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from . import native
from .nps import _as5, _check_fields, _packed, _window_arg, _workspace, nps_window
from .rules import NPS_DETREND, check_nps_args


class CrossSpectrum(NamedTuple):
    """What ``cross_spectrum`` returns (include/midd.h: THE CROSS SPECTRUM), on the host.  A group is a (b, c) pair; inputs [H, W] drop
    the two leading axes.  Sxy = X conj(Y); the planes are in DFT order (index 0 is DC), frequencies in cycles per pixel."""
    sxx: Optional[torch.Tensor]           # float64 [B, C, R, R], or None unless return_planes
    syy: Optional[torch.Tensor]
    sxy_re: Optional[torch.Tensor]
    sxy_im: Optional[torch.Tensor]
    radial_xx: torch.Tensor               # float64 [B, C, R/2+1]: the mean of the entries of radial bin r; NaN where the bin is empty
    radial_yy: torch.Tensor
    radial_xy_re: torch.Tensor
    radial_xy_im: torch.Tensor
    radial_count: torch.Tensor            # int64 [R/2+1]: entries per bin
    freqs: torch.Tensor                   # float64 [R/2+1]: r / R, cycles per pixel (0 .. 0.5)
    rois_used: torch.Tensor               # int64 [B, C]: ROIs averaged
    rois_skipped: torch.Tensor            # int64 [B, C]: ROIs left out because x or y holds a NaN or an Inf there
    roi: int
    step: int

    def transfer(self) -> torch.Tensor:
        """float64 [B, C, R/2+1]: ``radial_xy_re / radial_xx``, the share of x's amplitude at a frequency that is in y (1: kept, 0:
        removed; y = 0.5 x gives 0.5 everywhere).  On the host, in float64."""
        return self.radial_xy_re / self.radial_xx

    def frc(self) -> torch.Tensor:
        """float64 [B, C, R/2+1]: the Fourier ring correlation ``radial_xy_re / sqrt(radial_xx * radial_yy)``, in [-1, 1]."""
        return self.radial_xy_re / torch.sqrt(self.radial_xx * self.radial_yy)

    def resolution(self, threshold: float = 1.0 / 7.0) -> torch.Tensor:
        """float64 [B, C]: the frequency, in cycles per pixel, at which the FRC first falls below ``threshold``, looking from bin 1
        upward and interpolating linearly between that bin and the one before it (bin 1 itself below: its own frequency); 0.5 if it
        never falls below; NaN for a group without a used ROI."""
        frc = self.frc()
        flat = frc.reshape(-1, frc.shape[-1])
        used = self.rois_used.reshape(-1)
        out = torch.empty(flat.shape[0], dtype=torch.float64)
        for g in range(flat.shape[0]):
            out[g] = _first_crossing(flat[g].tolist(), self.freqs.tolist(), float(threshold)) if int(used[g]) > 0 else math.nan
        return out.reshape(frc.shape[:-1])


def _first_crossing(frc, freqs, threshold):
    for r in range(1, len(frc)):
        if frc[r] < threshold:                                  # (a NaN bin -- empty under exclude_axes -- is not below)
            prev = frc[r - 1]
            if r == 1 or not prev >= threshold:
                return freqs[r]
            return freqs[r - 1] + (prev - threshold) / (prev - frc[r]) * (freqs[r] - freqs[r - 1])
    return 0.5


@torch.no_grad()
def cross_spectrum(x: torch.Tensor, y: torch.Tensor, roi: int = 64, step: Optional[int] = None, detrend: str = "plane", window="hann",
                   exclude_axes: bool = False, return_planes: bool = False) -> CrossSpectrum:
    """The Welch cross-spectrum of the fields ``x`` and ``y`` (mi_cross_spectrum; include/midd.h: THE CROSS SPECTRUM): overlapping
    ``roi`` x ``roi`` regions at ``step`` (default roi / 2) of both fields are detrended and windowed as ``noise_power_spectrum`` does,
    transformed on the device as ONE complex field, separated into Sxx, Syy and Sxy = X conj(Y), averaged per (b, c) group over the
    K members and every position, and binned by radial frequency.  ``x`` and ``y`` are [B, K, C, H, W], [B, C, H, W] or [H, W]; a
    4-D argument beside a 5-D one is broadcast over K, otherwise the shapes are equal.  ROIs in which either field holds a NaN or an
    Inf are left out and counted once.  The fp32 transform's rounding error is relative to the two fields' COMBINED energy: a field
    much weaker than its partner inherits about 1e-7 of the stronger amplitude.  The results are copied to the host once (that waits
    for the stream); the planes only with ``return_planes``."""
    roi, step = check_nps_args(roi, step, detrend)
    w = nps_window(window, roi)
    x5, y5 = _as5(x, "x"), _as5(y, "y")
    flat = x.dim() == 2
    mixed = {x.dim(), y.dim()} == {4, 5}
    if mixed:
        if tuple(x5.shape[:1] + x5.shape[2:]) != tuple(y5.shape[:1] + y5.shape[2:]):
            raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)}: a [B, C, H, W] field beside a [B, K, C, H, W] one is broadcast over "
                             "K; B, C, H and W must agree")
    elif tuple(x.shape) != tuple(y.shape):
        raise ValueError(f"x {tuple(x.shape)} and y {tuple(y.shape)} must have the same shape (or one [B, C, H, W] beside one [B, K, C, H, W])")
    (B, Kx, CH, H, W), Ky = x5.shape, y5.shape[1]
    if min(B, Kx, Ky, CH) < 1:
        raise ValueError("x and y must have B >= 1, K >= 1 and C >= 1")
    _check_fields("cross_spectrum", "x and y", [x, y], H, W, roi)
    xs, ys = x5.contiguous(), y5.contiguous()
    lib, dev = native.lib(), xs.device
    G, bins = B * CH, roi // 2 + 1
    with torch.cuda.device(dev):
        # the planes last: they are copied to the host only if they are asked for
        ptr, host = _packed([("radial", 4 * G * bins, torch.float64, (4, B, CH, bins)), ("radial_count", bins, torch.int64, (bins,)),
                             ("rois_used", G, torch.int64, (B, CH)), ("rois_skipped", G, torch.int64, (B, CH)),
                             ("planes", 4 * G * roi * roi, torch.float64, (4, B, CH, roi, roi))], dev)
        ws, nbytes = _workspace(lib.mi_cross_spectrum_workspace_bytes, B, Kx, Ky, CH, H, W, roi, step, device=dev)
        native.check(lib.mi_cross_spectrum(xs.data_ptr(), ys.data_ptr(), B, Kx, Ky, CH, H, W, roi, step, NPS_DETREND[detrend], _window_arg(w),
                                           1 if exclude_axes else 0, ptr["planes"], ptr["radial"], ptr["radial_count"], ptr["rois_used"],
                                           ptr["rois_skipped"], ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream))
        got = host(None if return_planes else "planes")
    radial, used, skipped, planes = got["radial"], got["rois_used"], got["rois_skipped"], got.get("planes")
    if flat:
        radial, used, skipped = radial[:, 0, 0], used[0, 0], skipped[0, 0]
        planes = None if planes is None else planes[:, 0, 0]
    freqs = torch.arange(bins, dtype=torch.float64) / float(roi)
    pl = (None,) * 4 if planes is None else tuple(planes)
    return CrossSpectrum(*pl, *tuple(radial), got["radial_count"], freqs, used, skipped, roi, step)
