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


# ------------------------------------------------------------------------------ the preamble of a Welch call (spectral.py shares it)
def _as5(t: torch.Tensor, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or t.dim() not in (2, 4, 5):
        raise ValueError(f"{name} must be a [B, K, C, H, W], [B, C, H, W] or [H, W] tensor")
    return t[None, None, None] if t.dim() == 2 else (t[:, None] if t.dim() == 4 else t)


def _check_fields(call: str, names: str, fields, H: int, W: int, roi: int) -> None:      # the ROI fits; one CUDA device; float32
    if H < roi or W < roi:
        raise ValueError(f"the image ({H} x {W}) is smaller than the ROI ({roi} x {roi}): there are no partial ROIs")
    if len({f.device for f in fields}) > 1:
        raise ValueError(f"{names} must be on one device (got {' and '.join(str(f.device) for f in fields)})")
    if fields[0].device.type != "cuda":
        raise RuntimeError(f"{call} runs only on a ROCm GPU (got {fields[0].device}): there is no CPU fallback")
    if any(f.dtype != torch.float32 for f in fields):
        raise TypeError(f"{names} must be float32 (got {' and '.join(str(f.dtype) for f in fields)})")


def _packed(segments, device):
    """The outputs of a call in ONE device buffer of 8-byte words; ``segments``: the ordered (name, words, dtype, shape).  Returns
    ({name: device address}, host): ``host(until)`` copies the segments before the one named ``until`` (default: all) to the host
    once -- that waits for the stream -- and returns {name: cloned host tensor of its shape}."""
    offset, words = {}, 0
    for name, n, _, _ in segments:
        offset[name], words = words, words + n
    raw = torch.empty(words, dtype=torch.int64, device=device)

    def host(until=None):
        end = words if until is None else offset[until]
        h = raw[:end].cpu()
        return {name: h[offset[name]:offset[name] + n].view(dtype).reshape(shape).clone() for name, n, dtype, shape in segments if offset[name] < end}
    return {name: raw.data_ptr() + 8 * o for name, o in offset.items()}, host


def _workspace(query, *shape, device):      # (the workspace, its bytes); a query that answers 0 raises the library's message
    nbytes = query(*shape)
    if nbytes == 0:
        native.check(-1)
    return torch.empty(nbytes // 8, dtype=torch.float64, device=device), nbytes


def _window_arg(w: Optional[torch.Tensor]):
    return None if w is None else (C.c_float * w.numel())(*w.tolist())


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
    a5 = _as5(a, "a")
    flat = a.dim() == 2
    B, K, CH, H, W = a5.shape
    if min(B, K, CH) < 1:
        raise ValueError("a must have B >= 1, K >= 1 and C >= 1")
    b4 = None
    if b is not None:
        want = (H, W) if flat else (B, CH, H, W)
        if not isinstance(b, torch.Tensor) or tuple(b.shape) != want or b.device != a.device:
            raise ValueError(f"b must be a tensor of shape {want} on {a.device}: one image per (b, c) group, without the member axis")
        b4 = b[None, None] if flat else b
    _check_fields("noise_power_spectrum", "a and b", [a] if b is None else [a, b], H, W, roi)
    src, sub = a5.contiguous(), None if b4 is None else b4.contiguous()
    lib, dev = native.lib(), src.device
    G, bins = B * CH, roi // 2 + 1
    with torch.cuda.device(dev):
        ptr, host = _packed([("nps", G * roi * roi, torch.float64, (B, CH, roi, roi)), ("radial", G * bins, torch.float64, (B, CH, bins)),
                             ("radial_count", bins, torch.int64, (bins,)), ("rois_used", G, torch.int64, (B, CH)),
                             ("rois_skipped", G, torch.int64, (B, CH))], dev)
        ws, nbytes = _workspace(lib.mi_noise_power_spectrum_workspace_bytes, B, K, CH, H, W, roi, step, device=dev)
        native.check(lib.mi_noise_power_spectrum(src.data_ptr(), _ptr(sub), B, K, CH, H, W, roi, step, NPS_DETREND[detrend], _window_arg(w), scale,
                                                 1 if exclude_axes else 0, ptr["nps"], ptr["radial"], ptr["radial_count"], ptr["rois_used"],
                                                 ptr["rois_skipped"], ws.data_ptr(), nbytes,
                                                 torch.cuda.current_stream(dev).cuda_stream))
        got = host()
    nps, radial, used, skipped = (got[k][0, 0] if flat else got[k] for k in ("nps", "radial", "rois_used", "rois_skipped"))
    return NoisePowerSpectrum(nps, radial, got["radial_count"], torch.arange(bins, dtype=torch.float64) / float(roi), used, skipped, roi, step)
