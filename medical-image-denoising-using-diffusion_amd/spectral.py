"""The Welch cross-spectrum of two fields and what follows from it: the signal transfer and the Fourier ring correlation
(include/midd.h: THE CROSS SPECTRUM)."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import native
from .nps import nps_window
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


def _as5(t: torch.Tensor, name: str):
    if not isinstance(t, torch.Tensor) or t.dim() not in (2, 4, 5):
        raise ValueError(f"{name} must be a [B, K, C, H, W], [B, C, H, W] or [H, W] tensor")
    return t[None, None, None] if t.dim() == 2 else (t[:, None] if t.dim() == 4 else t)


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
    B, Kx, CH, H, W = x5.shape
    Ky = y5.shape[1]
    if min(B, Kx, Ky, CH) < 1:
        raise ValueError("x and y must have B >= 1, K >= 1 and C >= 1")
    if H < roi or W < roi:
        raise ValueError(f"the image ({H} x {W}) is smaller than the ROI ({roi} x {roi}): there are no partial ROIs")
    if x.device != y.device:
        raise ValueError(f"x and y must be on one device (got {x.device} and {y.device})")
    if x.device.type != "cuda":
        raise RuntimeError(f"cross_spectrum runs only on a ROCm GPU (got {x.device}): there is no CPU fallback")
    if x.dtype != torch.float32 or y.dtype != torch.float32:
        raise TypeError(f"x and y must be float32 (got {x.dtype} and {y.dtype})")
    xs, ys = x5.contiguous(), y5.contiguous()
    lib = native.lib()
    dev = xs.device
    G, bins = B * CH, roi // 2 + 1
    with torch.cuda.device(dev):
        # one 8-byte-word buffer for the outputs [radial 4*G*bins | radial_count bins | used G | skipped G | planes 4*G*R*R]: one
        # copy to the host, without the planes unless they are asked for
        o_cnt = 4 * G * bins
        o_used, o_skip, o_pl = o_cnt + bins, o_cnt + bins + G, o_cnt + bins + 2 * G
        raw = torch.empty(o_pl + 4 * G * roi * roi, dtype=torch.int64, device=dev)
        nbytes = lib.mi_cross_spectrum_workspace_bytes(B, Kx, Ky, CH, H, W, roi, step)
        if nbytes == 0:
            native.check(-1)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        base = raw.data_ptr()
        warg = None if w is None else (C.c_float * roi)(*w.tolist())
        native.check(lib.mi_cross_spectrum(xs.data_ptr(), ys.data_ptr(), B, Kx, Ky, CH, H, W, roi, step, NPS_DETREND[detrend], warg,
                                           1 if exclude_axes else 0, base + 8 * o_pl, base, base + 8 * o_cnt, base + 8 * o_used,
                                           base + 8 * o_skip, ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream))
        host = (raw if return_planes else raw[:o_pl]).cpu()
    radial = host[:o_cnt].view(torch.float64).reshape(4, B, CH, bins).clone()
    count = host[o_cnt:o_used].clone()
    used, skipped = host[o_used:o_skip].reshape(B, CH).clone(), host[o_skip:o_pl].reshape(B, CH).clone()
    planes = host[o_pl:].view(torch.float64).reshape(4, B, CH, roi, roi).clone() if return_planes else None
    if flat:
        radial, used, skipped = radial[:, 0, 0], used[0, 0], skipped[0, 0]
        planes = None if planes is None else planes[:, 0, 0]
    freqs = torch.arange(bins, dtype=torch.float64) / float(roi)
    pl = (None,) * 4 if planes is None else tuple(planes)
    return CrossSpectrum(*pl, *tuple(radial), count, freqs, used, skipped, roi, step)
