"""Pre/post-processing either side of the sampler, on the GPU.

Host-side mirror of what the reference does around `denoise` with PIL / torchvision / numpy on the host
(Backend/run.py:143-149,193-201; Backend/cddpm/cddpmModels.py:485-503) and of `compute_metrics`
(Backend/DDIM/DDIMModel.py:290-300), backed by libmidd.so (csrc/prepost.hip).  GPU tensors only: like the sampler
there is no CPU fallback here -- the reference's own host recipe (`server.preprocess` / `tensor_to_base64`)
remains the path for CPU tensors.

`resize_bicubic_f32`, `u16_to_unit_float` and `to_u16` are the high-bit-depth twin (not in the reference; include/midd.h: THE FLOAT
RESIZE AND THE 16-BIT ELEMENT RULES): Pillow's mode "F" resample bit for bit with typed loads and stores; image16.py is the host recipe.

`histogram_u16`, `window_levels`, `window_u16_to_float`, `window_to_u16` and `resize_bicubic_f32(..., levels=...)` are the window of
that path (include/midd.h: THE WINDOW): the grey range between two percentiles of an image goes to [0, 1] and back, exactly; the
levels are an int32 tensor that stays on the GPU.
"""
from typing import Optional, Tuple

import torch

from . import native


def _stream(t: torch.Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _need_cuda(t: torch.Tensor, dtype: torch.dtype, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{what}: expected a tensor on the GPU (the HIP kernels are the only implementation)")
    if t.dtype != dtype:
        raise TypeError(f"{what}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


def _workspace(nbytes: int, device) -> Tuple[torch.Tensor, int]:
    buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    return buf, (buf.data_ptr() + 255) & ~255


def resize_bicubic_u8(images: torch.Tensor, size: Tuple[int, int]) -> torch.Tensor:
    """uint8 [N,H,W] (or [H,W]) -> uint8 [N,size[0],size[1]]; bit-identical to
    `Image.fromarray(img, 'L').resize((size[1], size[0]), Image.BICUBIC)` per image
    (= `transforms.Resize(size, BICUBIC)` on a PIL 'L' image, run.py:198)."""
    squeeze = images.dim() == 2
    x = _need_cuda(images[None] if squeeze else images, torch.uint8, "resize_bicubic_u8")
    if x.dim() != 3:
        raise ValueError("resize_bicubic_u8: expected [N,H,W] or [H,W]")
    n, sh, sw = x.shape
    dh, dw = int(size[0]), int(size[1])
    lib = native.lib()
    nbytes = lib.mi_resize_workspace_bytes(n, sw, sh, dw, dh)
    if nbytes == 0:
        raise ValueError(f"resize_bicubic_u8: bad sizes {tuple(x.shape)} -> {(dh, dw)}")
    out = torch.empty((n, dh, dw), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        ws, wptr = _workspace(nbytes, x.device)
        native.check(lib.mi_resize_bicubic_u8(x.data_ptr(), n, sw, sh, out.data_ptr(), dw, dh, wptr, nbytes, _stream(x)))
        ws.record_stream(torch.cuda.current_stream(x.device))
    return out[0] if squeeze else out


def to_unit_float(images_u8: torch.Tensor) -> torch.Tensor:
    """`transforms.ToTensor()` scaling: uint8 -> float32 / 255 (same shape)."""
    x = _need_cuda(images_u8, torch.uint8, "to_unit_float")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().mi_u8_to_unit_f32(x.data_ptr(), out.data_ptr(), x.numel(), _stream(x)))
    return out


def to_u8(images: torch.Tensor) -> torch.Tensor:
    """`(clamp(x, 0, 1) * 255).astype('uint8')` (run.py:107,145): fp32 multiply, truncation."""
    x = _need_cuda(images, torch.float32, "to_u8")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().mi_unit_f32_to_u8(x.data_ptr(), out.data_ptr(), x.numel(), _stream(x)))
    return out


_PIX = {torch.uint8: native.MI_PIX_U8, torch.uint16: native.MI_PIX_U16, torch.float32: native.MI_PIX_F32}


def _need_levels(levels: torch.Tensor, n: int, device, what: str) -> torch.Tensor:
    """int32 [n,2] (or [2] when n == 1) on `device`: the (lo, hi) of include/midd.h: THE WINDOW, one pair per image."""
    if not isinstance(levels, torch.Tensor):
        raise TypeError(f"{what}: levels is an int32 tensor [N,2] on the GPU (window_levels returns one)")
    lv = _need_cuda(levels, torch.int32, f"{what}: levels")
    if lv.dim() == 1 and n == 1:
        lv = lv[None]
    if lv.dim() != 2 or tuple(lv.shape) != (n, 2):
        raise ValueError(f"{what}: levels must have shape [{n},2] (one (lo, hi) per image), got {tuple(levels.shape)}")
    if lv.device != device:
        raise RuntimeError(f"{what}: levels is on {lv.device}, the images on {device}")
    return lv.contiguous()


def resize_bicubic_f32(images: torch.Tensor, size: Tuple[int, int], clamp: bool = False,
                       out_dtype: torch.dtype = torch.float32, levels: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8, uint16 or float32 [N,H,W] (or [H,W]) -> float32 (or uint16) [N,size[0],size[1]]: the integer types are scaled to
    unit float on load (/ 255, / 65535), the resample is bit-identical to
    `Image.fromarray(img, mode "F").resize((size[1], size[0]), Image.BICUBIC)` per image, `clamp` clips the final value to [0, 1],
    and out_dtype=torch.uint16 stores clamp(v) * 65535 rounded to nearest (include/midd.h: THE FLOAT RESIZE).  Equal sizes: the pure
    conversion.  Channels fold into N.
    levels (int32 [N,2] on the GPU, from `window_levels`): a uint16 source and / or destination is taken under the window of its
    image instead (include/midd.h: THE WINDOW); None, the default, is the call as it always was."""
    squeeze = images.dim() == 2
    if images.dtype not in _PIX:
        raise TypeError(f"resize_bicubic_f32: expected uint8, uint16 or float32, got {images.dtype}")
    if out_dtype not in (torch.float32, torch.uint16):
        raise ValueError(f"resize_bicubic_f32: out_dtype is float32 or uint16, got {out_dtype} (8-bit output: resize_bicubic_u8)")
    x = _need_cuda(images[None] if squeeze else images, images.dtype, "resize_bicubic_f32")
    if x.dim() != 3:
        raise ValueError("resize_bicubic_f32: expected [N,H,W] or [H,W]")
    n, sh, sw = x.shape
    dh, dw = int(size[0]), int(size[1])
    lib = native.lib()
    nbytes = lib.mi_resize_f32_workspace_bytes(n, sw, sh, dw, dh)
    if nbytes == 0:
        raise ValueError(f"resize_bicubic_f32: bad sizes {tuple(x.shape)} -> {(dh, dw)}")
    lv = None
    if levels is not None:
        if x.dtype != torch.uint16 and out_dtype != torch.uint16:
            raise ValueError("resize_bicubic_f32: levels needs a uint16 source or out_dtype=torch.uint16 (the window acts on 16-bit elements)")
        lv = _need_levels(levels, n, x.device, "resize_bicubic_f32")
    out = torch.empty((n, dh, dw), dtype=out_dtype, device=x.device)
    with torch.cuda.device(x.device):
        ws, wptr = _workspace(nbytes, x.device)
        if lv is None:
            native.check(lib.mi_resize_bicubic_f32(x.data_ptr(), _PIX[x.dtype], n, sw, sh, out.data_ptr(), _PIX[out_dtype], dw, dh,
                                                   int(bool(clamp)), wptr, nbytes, _stream(x)))
        else:
            native.check(lib.mi_resize_bicubic_f32_window(x.data_ptr(), _PIX[x.dtype], n, sw, sh, out.data_ptr(), _PIX[out_dtype], dw, dh,
                                                          int(bool(clamp)), lv.data_ptr(), wptr, nbytes, _stream(x)))
        ws.record_stream(torch.cuda.current_stream(x.device))
    return out[0] if squeeze else out


def u16_to_unit_float(images_u16: torch.Tensor) -> torch.Tensor:
    """uint16 -> float32 / 65535 (same shape): one correctly rounded fp32 division."""
    x = _need_cuda(images_u16, torch.uint16, "u16_to_unit_float")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().mi_u16_to_unit_f32(x.data_ptr(), out.data_ptr(), x.numel(), _stream(x)))
    return out


def to_u16(images: torch.Tensor) -> torch.Tensor:
    """`(uint16)(clamp(x, 0, 1) * 65535 + 0.5)`, multiply and add in fp32: round to nearest (to_u8 truncates, as the reference)."""
    x = _need_cuda(images, torch.float32, "to_u16")
    out = torch.empty(x.shape, dtype=torch.uint16, device=x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().mi_unit_f32_to_u16(x.data_ptr(), out.data_ptr(), x.numel(), _stream(x)))
    return out


HIST_BINS = 65536


def _images_u16(images: torch.Tensor, what: str) -> Tuple[torch.Tensor, int, int]:
    """uint16 [N,...] (or [H,W]: one image) -> (contiguous tensor, N, pixels per image)."""
    x = _need_cuda(images, torch.uint16, what)
    if x.dim() < 2:
        raise ValueError(f"{what}: expected [N,H,W] or [H,W], got {tuple(x.shape)}")
    n = 1 if x.dim() == 2 else x.shape[0]
    if n < 1 or x.numel() == 0:
        raise ValueError(f"{what}: no pixels in {tuple(x.shape)}")
    return x, n, x.numel() // n


def histogram_u16(images: torch.Tensor) -> torch.Tensor:
    """uint16 [N,H,W] (or [H,W]) -> uint32 [N,65536]: per image, the number of pixels of every value (include/midd.h: THE WINDOW).
    Integer counts, deterministic; zeroed and filled on the current stream."""
    x, n, count = _images_u16(images, "histogram_u16")
    hist = torch.empty((n, HIST_BINS), dtype=torch.uint32, device=x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().mi_histogram_u16(x.data_ptr(), n, count, hist.data_ptr(), _stream(x)))
    return hist


def window_levels(images_or_hist: torch.Tensor, percentiles: Tuple[float, float] = (0.5, 99.5)) -> torch.Tensor:
    """uint16 images [N,H,W] (or [H,W]), or their uint32 histogram [N,65536] -> int32 [N,2] on the GPU: (lo, hi) per image, the
    grey levels at the two percentiles (0-based order statistic at floor(p * (pixels - 1) / 100)), hi > lo always (a flat image:
    hi = lo + 1).  (0, 100) is the min-max window.  The levels stay on the device: no synchronisation."""
    p_lo, p_hi = (float(p) for p in percentiles)
    if images_or_hist.dtype == torch.uint32:
        hist = _need_cuda(images_or_hist, torch.uint32, "window_levels")
        if hist.dim() == 1:
            hist = hist[None]
        if hist.dim() != 2 or hist.shape[1] != HIST_BINS:
            raise ValueError(f"window_levels: a histogram is uint32 [N,{HIST_BINS}], got {tuple(images_or_hist.shape)}")
    else:
        hist = histogram_u16(images_or_hist)
    n = hist.shape[0]
    levels = torch.empty((n, 2), dtype=torch.int32, device=hist.device)
    with torch.cuda.device(hist.device):
        native.check(native.lib().mi_window_levels(hist.data_ptr(), n, p_lo, p_hi, levels.data_ptr(), _stream(hist)))
    return levels


def window_u16_to_float(images: torch.Tensor, levels: torch.Tensor) -> torch.Tensor:
    """uint16 -> float32 (same shape): clip((v - lo) / (hi - lo), 0, 1) under the (lo, hi) of each image, one fp32 division."""
    x, n, count = _images_u16(images, "window_u16_to_float")
    lv = _need_levels(levels, n, x.device, "window_u16_to_float")
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().mi_window_u16_to_f32(x.data_ptr(), lv.data_ptr(), n, count, out.data_ptr(), _stream(x)))
    return out


def window_to_u16(x: torch.Tensor, levels: torch.Tensor) -> torch.Tensor:
    """float32 [N,H,W] (or [H,W]) -> uint16: lo + (uint32)(clip(x, 0, 1) * (hi - lo) + 0.5) under the (lo, hi) of each image (the
    multiply and the add in fp32; a NaN stores lo).  The inverse of window_u16_to_float on every level inside the window."""
    x = _need_cuda(x, torch.float32, "window_to_u16")
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"window_to_u16: expected [N,H,W] or [H,W], got {tuple(x.shape)}")
    n = 1 if x.dim() == 2 else x.shape[0]
    lv = _need_levels(levels, n, x.device, "window_to_u16")
    out = torch.empty(x.shape, dtype=torch.uint16, device=x.device)
    with torch.cuda.device(x.device):
        native.check(native.lib().mi_window_f32_to_u16(x.data_ptr(), lv.data_ptr(), n, x.numel() // n, out.data_ptr(), _stream(x)))
    return out


def image_metrics(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Per-image (PSNR, SSIM) of `compute_metrics`: float64 [N,2] on the GPU; inputs [N,1,H,W] or [N,H,W] fp32."""
    p = _need_cuda(pred, torch.float32, "image_metrics")
    t = _need_cuda(target, torch.float32, "image_metrics")
    if p.shape != t.shape:
        raise ValueError("image_metrics: shapes differ")
    if p.dim() == 4:
        if p.shape[1] != 1:
            raise ValueError("image_metrics: single-channel images expected")
        p, t = p[:, 0].contiguous(), t[:, 0].contiguous()
    n, h, w = p.shape
    lib = native.lib()
    nbytes = lib.mi_metrics_workspace_bytes(n, h)
    out = torch.empty((n, 2), dtype=torch.float64, device=p.device)
    with torch.cuda.device(p.device):
        ws, wptr = _workspace(nbytes, p.device)
        native.check(lib.mi_image_metrics(t.data_ptr(), p.data_ptr(), n, h, w, out.data_ptr(), wptr, nbytes, _stream(p)))
        ws.record_stream(torch.cuda.current_stream(p.device))
    return out


def compute_metrics(pred: torch.Tensor, target: torch.Tensor) -> Tuple[float, float]:
    """Drop-in for the reference's `compute_metrics(pred, target)` (DDIMModel.py:290-300): batch means of PSNR, SSIM."""
    m = image_metrics(pred, target).mean(dim=0).cpu()
    return float(m[0]), float(m[1])
