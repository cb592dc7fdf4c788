"""The training objective as an evaluation: the forward noising and the loss terms as stand-alone calls, their argument rules and
what ``DiffusionDenoiser.denoising_loss`` / ``loss_profile`` return (include/midd.h: THE FORWARD NOISE, THE NOISING, THE DENOISING
LOSS)."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from . import native
from .rules import _integer, check_seed
from .tensors import _ptr


class LossMaps(NamedTuple):
    """The per-pixel maps of ``denoising_loss(..., return_maps=True)``, each [B, C, H, W] (include/midd.h: THE DENOISING LOSS)."""
    q: torch.Tensor          # squared error of the predicted noise
    g: torch.Tensor          # |Sobel magnitude of the predicted clean image - that of the clean image|
    p: torch.Tensor          # the predicted clean image, clamped to [0, 1]


class DenoisingLoss(NamedTuple):
    """``DiffusionDenoiser.denoising_loss``: per-sample float64 [B] scalars, the timesteps [B] they were taken at, the seed of the
    forward noise (None with a caller's ``noise``) and, on request, the per-pixel maps."""
    loss: torch.Tensor
    mse: torch.Tensor
    edge: torch.Tensor
    t: torch.Tensor
    seed: Optional[int]
    maps: Optional[LossMaps]


class LossProfile(NamedTuple):
    """``DiffusionDenoiser.loss_profile``: the timesteps (a tuple of T ints) and float64 CPU tensors [T, B]."""
    t: Tuple[int, ...]
    loss: torch.Tensor
    mse: torch.Tensor
    edge: torch.Tensor


def check_loss_source(seed, noise, sample_offset, draw, like: torch.Tensor) -> Tuple[Optional[int], int, int]:
    """Argument rules of the forward noise (include/midd.h: THE FORWARD NOISE) -> (seed or None, sample_offset, draw); raises
    ValueError before any GPU work.  Exactly one of ``seed`` (drawn on the device) and ``noise`` (a tensor like ``like``)."""
    if seed is not None and noise is not None:
        raise ValueError("pass either seed (noise drawn on the device) or noise (a tensor), not both")
    if seed is None and noise is None:
        raise ValueError("pass a seed (noise drawn on the device) or a noise tensor")
    _, sample_offset = check_seed(0, sample_offset)
    draw = _integer(draw, "draw", 1 << 31)
    if seed is not None:
        return _integer(seed, "seed", 1 << 64), sample_offset, draw
    if not isinstance(noise, torch.Tensor) or noise.shape != like.shape or noise.dtype != like.dtype or noise.device != like.device:
        raise ValueError(f"noise must be a {like.dtype} tensor of shape {tuple(like.shape)} on {like.device}")
    return None, sample_offset, draw


def loss_table_args(t, alpha_hat, B: int):
    """-> (host arrays to keep alive over the call, (t, alpha_hat, noise_steps) as the loss calls take them); ValueError for a ``t``
    that has not B entries or leaves [0, noise_steps).  ``alpha_hat``: the schedule tensor (copied to the host here: from a device
    that waits for its stream) or a float32 host array its owner keeps (``DiffusionDenoiser`` does, per instance)."""
    import numpy as np
    if isinstance(alpha_hat, np.ndarray):
        tab = np.ascontiguousarray(alpha_hat, dtype=np.float32)
    else:
        tab = np.ascontiguousarray(alpha_hat.detach().to("cpu", torch.float32).numpy())
    tt = torch.as_tensor(t).reshape(-1).to("cpu", torch.int64)
    if tt.numel() != B:
        raise ValueError(f"t must have {B} entries (got {tt.numel()})")
    if B and (int(tt.min()) < 0 or int(tt.max()) >= tab.shape[0]):
        raise ValueError(f"t must be in [0, {tab.shape[0]}) (got {tt.tolist()})")
    t_host = np.ascontiguousarray(tt.numpy().astype(np.int32))
    return [tab, t_host], (t_host.ctypes.data_as(C.POINTER(C.c_int32)), tab.ctypes.data_as(C.POINTER(C.c_float)), int(tab.shape[0]))


def loss_counter_args(seed, sample_index, draws, B: int):
    """-> (host arrays to keep alive, (sample_index, draws) as the loss calls take them: int64 [B] or NULL each)."""
    import numpy as np
    if seed is None and (sample_index is not None or draws is not None):
        raise ValueError("sample_index and draws are counter words of the seeded noise: pass seed as well")
    keep, out = [], []
    for v, what, bound in ((sample_index, "sample_index", 1 << 63), (draws, "draws", 1 << 31)):
        if v is None:
            out.append(None)
            continue
        vals = [_integer(i, what, bound) for i in v]
        if len(vals) != B:
            raise ValueError(f"{what} must have {B} entries (got {len(vals)})")
        keep.append(np.ascontiguousarray(np.asarray(vals, dtype=np.int64)))
        out.append(keep[-1].ctypes.data_as(C.POINTER(C.c_int64)))
    return keep, tuple(out)


def _loss_tensor(x, what: str, like: Optional[torch.Tensor] = None) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"{what} must be a [B, C, H, W] tensor")
    if like is not None and (x.shape != like.shape or x.device != like.device):
        raise ValueError(f"{what} must match the clean images in shape and device (got {tuple(x.shape)} on {x.device})")
    if x.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (got {x.dtype})")
    return x


@torch.no_grad()
def noise_images(x: torch.Tensor, t, alpha_hat: torch.Tensor, seed: Optional[int] = None, sample_offset: int = 0, draw: int = 0,
                 noise: Optional[torch.Tensor] = None, sample_index=None, draws=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x_t, eps) with x_t = sqrt(alpha_hat[t]) * x + sqrt(1 - alpha_hat[t]) * eps per sample (mi_noise_images; include/midd.h: THE
    NOISING): the bits of the reference's expression in torch eager.  eps is ``noise`` or the seeded forward noise of
    (seed, sample_offset + b, draw), drawn on the device (THE FORWARD NOISE).  ``alpha_hat``: the schedule tensor, or a float32 host
    array of it (a device tensor is copied to the host per call, which waits for the stream)."""
    x = _loss_tensor(x, "x")
    seed, sample_offset, draw = check_loss_source(seed, noise, sample_offset, draw, x)
    B, Cc, H, W = x.shape
    keep, tables = loss_table_args(t, alpha_hat, B)
    keep2, counters = loss_counter_args(seed, sample_index, draws, B)
    if x.device.type != "cuda":
        raise RuntimeError(f"noise_images runs only on a ROCm GPU (got {x.device}): there is no CPU fallback")
    with torch.cuda.device(x.device):
        src = x.contiguous()
        eps = noise.contiguous() if seed is None else torch.empty_like(src)
        x_t = torch.empty_like(src)
        native.check(native.lib().mi_noise_images(src.data_ptr(), *tables, eps.data_ptr() if seed is None else None, 0 if seed is None else 1,
                                                  C.c_uint64(seed or 0), C.c_int64(sample_offset), C.c_int64(draw), *counters,
                                                  x_t.data_ptr(), None if seed is None else eps.data_ptr(), B, Cc, H, W,
                                                  torch.cuda.current_stream(x.device).cuda_stream))
    return x_t, eps


@torch.no_grad()
def loss_terms(clean: torch.Tensor, eps_pred: torch.Tensor, t, alpha_hat: torch.Tensor, x_t: Optional[torch.Tensor] = None,
               noise: Optional[torch.Tensor] = None, seed: Optional[int] = None, sample_offset: int = 0, draw: int = 0,
               clamp_eps: bool = True, edge_weight: float = 0.2, return_maps: bool = False, sample_index=None, draws=None):
    """THE DENOISING LOSS (include/midd.h) of a given predicted noise, no network (mi_loss_terms) -> (out float64 [B, 3] =
    (mse, edge, loss), maps float32 [3, B, C, H, W] = (q, g, p) or None).  Explicit form: ``x_t`` and ``noise``; seeded form: ``seed``
    (x_t and the noise are formed again on the device, the bits of the explicit form on what ``noise_images(seed=...)`` returns)."""
    clean = _loss_tensor(clean, "clean")
    eps_pred = _loss_tensor(eps_pred, "eps_pred", clean)
    seed, sample_offset, draw = check_loss_source(seed, noise, sample_offset, draw, clean)
    if (seed is None) != (x_t is not None):
        raise ValueError("x_t goes with noise (the explicit form); the seeded form takes neither")
    if x_t is not None:
        x_t = _loss_tensor(x_t, "x_t", clean)
    B, Cc, H, W = clean.shape
    keep, tables = loss_table_args(t, alpha_hat, B)
    keep2, counters = loss_counter_args(seed, sample_index, draws, B)
    if clean.device.type != "cuda":
        raise RuntimeError(f"loss_terms runs only on a ROCm GPU (got {clean.device}): there is no CPU fallback")
    dev = clean.device
    lib = native.lib()
    with torch.cuda.device(dev):
        cl, pred = clean.contiguous(), eps_pred.contiguous()
        xt = None if x_t is None else x_t.contiguous()
        eps = None if noise is None else noise.contiguous()
        out = torch.empty((B, 3), dtype=torch.float64, device=dev)
        maps = torch.empty((3,) + tuple(cl.shape), dtype=torch.float32, device=dev) if return_maps else None
        nbytes = lib.mi_loss_workspace_bytes(B, Cc, H, W)
        if nbytes == 0:
            native.check(-1)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        native.check(lib.mi_loss_terms(cl.data_ptr(), _ptr(xt), _ptr(eps),
                                       pred.data_ptr(), *tables, 0 if seed is None else 1, C.c_uint64(seed or 0), C.c_int64(sample_offset),
                                       C.c_int64(draw), *counters, native.MI_CLAMP_EPS if clamp_eps else 0, C.c_double(float(edge_weight)),
                                       out.data_ptr(), _ptr(maps), B, Cc, H, W, ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream(dev).cuda_stream))
    return out, maps
