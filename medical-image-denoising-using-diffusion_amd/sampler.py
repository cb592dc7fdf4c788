"""``DiffusionDenoiser``: schedule + reverse loop, same surface as the reference class
(/root/reference/Backend/DDIM/DDIMModel.py:250-289; stochastic cddpm variant
/root/reference/Backend/cddpm/cddpmModels.py:263-308).

The schedule tables are built with the same torch calls as the reference so they are bit
identical; the loop itself (UNet forward + fused x_{t-1} update per timestep) is a single
call into libmidd.so.
"""
from __future__ import annotations

import ctypes as C
import operator
from typing import Optional, Sequence, Tuple

import torch

from . import native
from .config import timestep_list

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")    # DDIMModel.py:10


def check_seed(seed, sample_offset) -> Tuple[int, int]:
    """Argument rules of the seeded step noise (include/midd.h: mi_denoise_seeded) -> (seed, sample_offset) as Python ints;
    raises ValueError before any GPU work."""
    def integer(v, what, bound):
        try:
            if isinstance(v, bool):
                raise TypeError
            i = operator.index(v)
        except TypeError:
            raise ValueError(f"{what} must be an integer (got {v!r})") from None
        if not (0 <= i < bound):
            raise ValueError(f"{what} must be in [0, 2**{bound.bit_length() - 1}) (got {v!r})")
        return i
    return integer(seed, "seed", 1 << 64), integer(sample_offset, "sample_offset", 1 << 63)


@torch.no_grad()
def step_noise(seed: int, n_iters: int, shape: Sequence[int], sample_offset: int = 0, device=None) -> torch.Tensor:
    """The 0.5-scaled step noise a seeded cddpm run draws, as a tensor [n_iters, B, C, H, W] (mi_step_noise_fill).

    ``denoise(x, k, step_noise=step_noise(s, n, x.shape))`` equals ``denoise(x, k, seed=s)`` bit for bit: the replay and
    export path of a seeded run.  Entry ``[i, b]`` is a pure function of (seed, sample_offset + b, i, element index):
    Philox4x32-10 + Box-Muller, specified in include/midd.h.  ``shape`` is the image batch's (B, C, H, W)."""
    seed, sample_offset = check_seed(seed, sample_offset)
    if len(shape) != 4 or n_iters < 0 or min(shape) < 0:
        raise ValueError("shape must be (B, C, H, W) and n_iters >= 0")
    B, Cc, H, W = (int(v) for v in shape)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError(f"step_noise runs only on a ROCm GPU (got {dev}): there is no CPU fallback")
    lib = native.lib()
    with torch.cuda.device(dev):
        out = torch.empty((int(n_iters), B, Cc, H, W), dtype=torch.float32, device=dev)
        native.check(lib.mi_step_noise_fill(out.data_ptr(), int(n_iters), B, Cc, H, W, C.c_uint64(seed), C.c_int64(sample_offset),
                                            torch.cuda.current_stream(out.device).cuda_stream))
    return out


class DiffusionDenoiser:
    def __init__(self, model, noise_steps=50, beta_start=1e-4, beta_end=0.02):
        self.model = model
        self.noise_steps = noise_steps
        dev = device
        try:
            dev = next(model.parameters()).device
        except (AttributeError, StopIteration):
            pass
        # DDIMModel.py:255-257 (linspace is evaluated on the CPU there too, then moved)
        self.beta = torch.linspace(beta_start, beta_end, noise_steps).to(dev)
        self.alpha = 1.0 - self.beta
        self.alpha_hat = torch.cumprod(self.alpha, dim=0)

    @torch.no_grad()
    def denoise(self, noisy_img: torch.Tensor, inference_steps: int = 25,
                step_noise: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                sample_offset: int = 0) -> torch.Tensor:
        """x = denoiser.denoise(noisy_img, inference_steps) — DDIMModel.py:268-289.

        Starts from the noisy image itself, conditions every step on it, never mutates it and
        returns a new tensor on the same device.  For ``model.variant == 'cddpm'`` the update
        adds ``sqrt(beta_t) * 0.5 * randn`` for t > 0 and does not clamp eps
        (cddpmModels.py:290-303); ``step_noise`` ([n_iters,B,C,H,W], already scaled by 0.5)
        overrides the on-device draw so a run can be replayed exactly.

        ``seed`` (cddpm; not a reference argument): the noise is drawn inside the fused update from a counter-based
        generator instead (``step_noise()`` above gives the same values as a tensor): no noise tensor is allocated, the
        same seed gives the same bits again, and a sample's noise depends on its GLOBAL index ``sample_offset + b`` only --
        with ``batch_invariant=True``, ``denoise(x, seed=s)[lo:hi] == denoise(x[lo:hi], seed=s, sample_offset=lo)``.
        ``seed`` together with ``step_noise`` raises ValueError; the DDIM variant ignores both.  ``seed=None``: torch.randn
        up front, as before.
        """
        if seed is not None:
            if step_noise is not None:
                raise ValueError("pass either seed (noise drawn on the device) or step_noise (a noise tensor), not both")
            seed, sample_offset = check_seed(seed, sample_offset)
        self.model.eval()
        steps = timestep_list(self.noise_steps, inference_steps)
        stochastic = getattr(self.model, "variant", "ddim") == "cddpm"
        if stochastic and step_noise is None and seed is None:
            step_noise = 0.5 * torch.randn((len(steps),) + tuple(noisy_img.shape), device=noisy_img.device)
        if not stochastic:
            step_noise = seed = None
        seeded = {} if seed is None else {"seed": seed, "sample_offset": sample_offset}
        return self.model.run_sampler(noisy_img, steps, self.beta, self.alpha, self.alpha_hat,
                                      clamp_eps=not stochastic, step_noise=step_noise, **seeded)

    # north_star's wording for the same call
    ddim_sample = denoise
