"""The noise power spectrum of a residual field or of an ensemble's spread by Welch's method (include/midd.h: THE NOISE POWER
SPECTRUM)."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import native
from .rules import NPS_DETREND, check_nps_args
from .tensors import _ptr


class NoisePowerSpectrum(NamedTuple):
    """What ``noise_power_spectrum`` returns (include/midd.h: THE NOISE POWER SPECTRUM), on the host.  A group is a (b, c) pair; an input
    [H, W] drops the two leading axes."""
    nps: torch.Tensor                     # float64 [B, C, R, R]: DFT order (index 0 is DC), frequencies in cycles per pixel
    radial: torch.Tensor                  # float64 [B, C, R/2+1]: the mean of the entries of radial bin r; NaN where the bin is empty
    radial_count: torch.Tensor            # int64 [R/2+1]: entries per bin
    freqs: torch.Tensor                   # float64 [R/2+1]: r / R, cycles per pixel (0 .. 0.5)
    rois_used: torch.Tensor               # int64 [B, C]: ROIs averaged
    rois_skipped: torch.Tensor            # int64 [B, C]: ROIs left out because they hold a NaN or an Inf
    roi: int
    step: int

    def variance(self) -> torch.Tensor:
        """float64 [B, C]: the Parseval integral sum(nps) / R^2 -- ``scale`` times the mean windowed variance of the detrended ROIs."""
        return self.nps.sum(dim=(-2, -1)) / float(self.roi * self.roi)


def nps_window(window, roi: int) -> Optional[torch.Tensor]:
    """The window table of ``noise_power_spectrum`` as a float32 CPU tensor [roi], or None: "hann" is the periodic
    0.5 - 0.5 cos(2 pi n / roi), computed in double and rounded to fp32; a sequence or tensor of ``roi`` finite numbers is taken as is."""
    if window is None:
        return None
    if isinstance(window, str):
        if window != "hann":
            raise ValueError(f"window must be 'hann', None or a table of {roi} numbers (got {window!r})")
        return torch.tensor([0.5 - 0.5 * math.cos(2.0 * math.pi * n / roi) for n in range(roi)], dtype=torch.float64).to(torch.float32)
    w = torch.as_tensor(window).detach().to("cpu", torch.float32).contiguous()
    if w.dim() != 1 or w.numel() != roi or not bool(torch.isfinite(w).all()):
        raise ValueError(f"window must be 'hann', None or a table of {roi} finite numbers")
    return w


@torch.no_grad()
def noise_power_spectrum(a: torch.Tensor, b: Optional[torch.Tensor] = None, roi: int = 64, step: Optional[int] = None, detrend: str = "plane",
                         window="hann", scale: float = 1.0, exclude_axes: bool = False) -> NoisePowerSpectrum:
    """The noise power spectrum of the field ``a - b`` by Welch's method (mi_noise_power_spectrum; include/midd.h: THE NOISE POWER
    SPECTRUM): overlapping ``roi`` x ``roi`` regions at ``step`` (default roi / 2) are detrended ("none", "mean", "plane"), windowed
    ("hann", None or a table), transformed on the device, their periodograms averaged per (b, c) group over the K members and every
    position, and the average binned by radial frequency.  ``a`` is [B, K, C, H, W], [B, C, H, W] (K = 1) or [H, W]; ``b`` is
    [B, C, H, W] ([H, W] for an [H, W] field), broadcast over K, subtracted inside the kernel.  White noise of variance s^2 gives a
    flat spectrum of ``scale`` * s^2.  ROIs holding a NaN or an Inf are left out and counted.  The results are copied to the host
    once (that waits for the stream)."""
    roi, step = check_nps_args(roi, step, detrend)
    w = nps_window(window, roi)
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"scale must be finite (got {scale!r})")
    if not isinstance(a, torch.Tensor) or a.dim() not in (2, 4, 5):
        raise ValueError("a must be a [B, K, C, H, W], [B, C, H, W] or [H, W] tensor")
    flat = a.dim() == 2
    a5 = a[None, None, None] if flat else (a[:, None] if a.dim() == 4 else a)
    B, K, CH, H, W = a5.shape
    if min(B, K, CH) < 1:
        raise ValueError("a must have B >= 1, K >= 1 and C >= 1")
    b4 = None
    if b is not None:
        want = (H, W) if flat else (B, CH, H, W)
        if not isinstance(b, torch.Tensor) or tuple(b.shape) != want or b.device != a.device:
            raise ValueError(f"b must be a tensor of shape {want} on {a.device}: one image per (b, c) group, without the member axis")
        b4 = b[None, None] if flat else b
    if H < roi or W < roi:
        raise ValueError(f"the image ({H} x {W}) is smaller than the ROI ({roi} x {roi}): there are no partial ROIs")
    if a.device.type != "cuda":
        raise RuntimeError(f"noise_power_spectrum runs only on a ROCm GPU (got {a.device}): there is no CPU fallback")
    if a.dtype != torch.float32 or (b is not None and b.dtype != torch.float32):
        raise TypeError(f"a and b must be float32 (got {a.dtype}" + (f" and {b.dtype})" if b is not None else ")"))
    src = a5.contiguous()
    sub = None if b4 is None else b4.contiguous()
    lib = native.lib()
    dev = src.device
    G, bins = B * CH, roi // 2 + 1
    with torch.cuda.device(dev):
        # one 8-byte-word buffer for the outputs [nps G*R*R | radial G*bins | radial_count bins | used G | skipped G]: one copy to the host
        o_rad = G * roi * roi
        o_cnt, o_used, o_skip = o_rad + G * bins, o_rad + G * bins + bins, o_rad + G * bins + bins + G
        raw = torch.empty(o_skip + G, dtype=torch.int64, device=dev)
        nbytes = lib.mi_noise_power_spectrum_workspace_bytes(B, K, CH, H, W, roi, step)
        if nbytes == 0:
            native.check(-1)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        base = raw.data_ptr()
        warg = None if w is None else (C.c_float * roi)(*w.tolist())
        native.check(lib.mi_noise_power_spectrum(src.data_ptr(), _ptr(sub), B, K, CH, H, W, roi, step,
                                                 NPS_DETREND[detrend], warg, scale, 1 if exclude_axes else 0,
                                                 base, base + 8 * o_rad, base + 8 * o_cnt, base + 8 * o_used, base + 8 * o_skip,
                                                 ws.data_ptr(), nbytes, torch.cuda.current_stream(dev).cuda_stream))
        host = raw.cpu()
    nps = host[:o_rad].view(torch.float64).reshape(B, CH, roi, roi).clone()
    radial = host[o_rad:o_cnt].view(torch.float64).reshape(B, CH, bins).clone()
    count = host[o_cnt:o_used].clone()
    used, skipped = host[o_used:o_skip].reshape(B, CH).clone(), host[o_skip:].reshape(B, CH).clone()
    if flat:
        nps, radial, used, skipped = nps[0, 0], radial[0, 0], used[0, 0], skipped[0, 0]
    freqs = torch.arange(bins, dtype=torch.float64) / float(roi)
    return NoisePowerSpectrum(nps, radial, count, freqs, used, skipped, roi, step)
