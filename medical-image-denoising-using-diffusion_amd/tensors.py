"""What the native wrappers ask of a tensor argument, once: the pointer of an optional tensor and the shape / device / dtype rule
of the stand-alone operators."""
from __future__ import annotations

from typing import Callable, Optional

import torch


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def gpu_tensor(x, shape_ok: Callable[[torch.Tensor], bool], shape_msg: str, device_msg: str, what: str,
               then: Optional[Callable[[torch.Tensor], None]] = None) -> torch.Tensor:
    """The tensor rule of a stand-alone operator -> ``x``, contiguous.  In this order: a tensor for which ``shape_ok`` holds, or
    ValueError(shape_msg); ``then(x)``, a further rule of the caller's; a ROCm device, or RuntimeError(device_msg, whose ``{}`` is
    the device); float32, or TypeError.  The wording is the caller's."""
    if not isinstance(x, torch.Tensor) or not shape_ok(x):
        raise ValueError(shape_msg)
    if then is not None:
        then(x)
    if x.device.type != "cuda":
        raise RuntimeError(device_msg.format(x.device))
    if x.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (got {x.dtype})")
    return x.contiguous()


def dims_tensor(x, what: str, dims: int, kernels: str) -> torch.Tensor:
    """``gpu_tensor`` for a non-empty tensor of ``dims`` dimensions; ``kernels`` names who refuses a CPU tensor ("tiling runs")."""
    return gpu_tensor(x, lambda t: t.dim() == dims and min(t.shape) >= 1, f"{what} must be a {dims}-dimensional non-empty tensor",
                      f"{what} is on {{}}: {kernels} only on a ROCm GPU, there is no CPU fallback", what)


def members_tensor(samples, caller: str, then: Optional[Callable[[torch.Tensor], None]] = None) -> torch.Tensor:
    """``gpu_tensor`` for the ``samples`` [B, members, ...] of the ensemble operators."""
    return gpu_tensor(samples, lambda t: t.dim() >= 3 and t.shape[0] >= 1 and t.shape[1] >= 1,
                      "samples must be a [B, members, ...] tensor with B >= 1 and members >= 1",
                      f"{caller} runs only on a ROCm GPU (got {{}}): there is no CPU fallback", "samples", then)
