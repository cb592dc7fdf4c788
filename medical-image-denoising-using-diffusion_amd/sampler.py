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
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import native
from .config import timestep_list

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")    # DDIMModel.py:10


def _integer(v, what, bound, low=0) -> int:
    try:
        if isinstance(v, bool):
            raise TypeError
        i = operator.index(v)
    except TypeError:
        raise ValueError(f"{what} must be an integer (got {v!r})") from None
    if not (low <= i < bound):
        raise ValueError(f"{what} must be in [{low}, 2**{bound.bit_length() - 1}) (got {v!r})")
    return i


def check_seed(seed, sample_offset) -> Tuple[int, int]:
    """Argument rules of the seeded step noise (include/midd.h: mi_denoise_seeded) -> (seed, sample_offset) as Python ints;
    raises ValueError before any GPU work."""
    return _integer(seed, "seed", 1 << 64), _integer(sample_offset, "sample_offset", 1 << 63)


def check_member(member, what: str = "member", low: int = 0) -> int:
    """A member index (or, with low=1, a member count) of the seeded step noise: one 32-bit counter word (include/midd.h)."""
    return _integer(member, what, 1 << 32 if low == 0 else 1 << 31, low)


class EnsembleResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_ensemble`` returns."""
    mean: torch.Tensor                    # [B, C, H, W]: per-pixel mean of the members
    std: Optional[torch.Tensor]           # [B, C, H, W]: unbiased per-pixel standard deviation; None for one member
    samples: Optional[torch.Tensor]       # [B, members, C, H, W] with return_samples=True
    seed: int                             # the seed of the run (drawn when the call had seed=None): pass it to repeat the run


@torch.no_grad()
def step_noise(seed: int, n_iters: int, shape: Sequence[int], sample_offset: int = 0, device=None, member: int = 0) -> torch.Tensor:
    """The 0.5-scaled step noise a seeded cddpm run draws, as a tensor [n_iters, B, C, H, W] (mi_step_noise_fill_member).

    ``denoise(x, k, step_noise=step_noise(s, n, x.shape))`` equals ``denoise(x, k, seed=s)`` bit for bit: the replay and
    export path of a seeded run.  Entry ``[i, b]`` is a pure function of (seed, sample_offset + b, i, element index):
    Philox4x32-10 + Box-Muller, specified in include/midd.h.  ``shape`` is the image batch's (B, C, H, W).  ``member`` m: the
    noise of ensemble member m of every image (``denoise_ensemble``, ``denoise(..., member=m)``); 0 is the plain seeded run."""
    seed, sample_offset = check_seed(seed, sample_offset)
    member = check_member(member)
    if len(shape) != 4 or n_iters < 0 or min(shape) < 0:
        raise ValueError("shape must be (B, C, H, W) and n_iters >= 0")
    B, Cc, H, W = (int(v) for v in shape)
    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError(f"step_noise runs only on a ROCm GPU (got {dev}): there is no CPU fallback")
    lib = native.lib()
    with torch.cuda.device(dev):
        out = torch.empty((int(n_iters), B, Cc, H, W), dtype=torch.float32, device=dev)
        native.check(lib.mi_step_noise_fill_member(out.data_ptr(), int(n_iters), B, Cc, H, W, C.c_uint64(seed), C.c_int64(sample_offset),
                                                   C.c_int64(member), torch.cuda.current_stream(out.device).cuda_stream))
    return out


@torch.no_grad()
def ensemble_reduce(samples: torch.Tensor) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(mean, std) over dim 1 of ``samples`` [B, members, ...] with the arithmetic of ``denoise_ensemble`` (mi_ensemble_reduce:
    double precision, members in index order, unbiased std) -- for members gathered from several calls or GPUs.  std is None
    for one member."""
    if not isinstance(samples, torch.Tensor) or samples.dim() < 3 or samples.shape[0] < 1 or samples.shape[1] < 1:
        raise ValueError("samples must be a [B, members, ...] tensor with B >= 1 and members >= 1")
    if samples.device.type != "cuda":
        raise RuntimeError(f"ensemble_reduce runs only on a ROCm GPU (got {samples.device}): there is no CPU fallback")
    if samples.dtype != torch.float32:
        raise TypeError(f"samples must be float32 (got {samples.dtype})")
    src = samples.contiguous()
    B, K = src.shape[:2]
    chw = src[0, 0].numel()
    with torch.cuda.device(src.device):
        mean = torch.empty((B,) + tuple(src.shape[2:]), dtype=torch.float32, device=src.device)
        std = torch.empty_like(mean) if K >= 2 else None
        native.check(native.lib().mi_ensemble_reduce(src.data_ptr(), B, K, chw, mean.data_ptr(), None if std is None else std.data_ptr(),
                                                     torch.cuda.current_stream(src.device).cuda_stream))
    return mean, std


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
                sample_offset: int = 0, member: int = 0) -> torch.Tensor:
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

        ``member`` (with ``seed``): which draw of every image, 0 being the run described above.  ``denoise(x, seed=s, member=m)``
        is member m of ``denoise_ensemble(x, seed=s)`` run alone (bit for bit with ``batch_invariant=True``).
        """
        if seed is not None:
            if step_noise is not None:
                raise ValueError("pass either seed (noise drawn on the device) or step_noise (a noise tensor), not both")
            seed, sample_offset = check_seed(seed, sample_offset)
        self.model.eval()
        steps = timestep_list(self.noise_steps, inference_steps)
        stochastic = getattr(self.model, "variant", "ddim") == "cddpm"
        if stochastic and step_noise is None and seed is None and member == 0:      # (a member without a seed: run_sampler refuses)
            step_noise = 0.5 * torch.randn((len(steps),) + tuple(noisy_img.shape), device=noisy_img.device)
        if not stochastic:
            step_noise = seed = None
            member = 0
        seeded = {"member": member} if seed is None else {"seed": seed, "sample_offset": sample_offset, "member": member}
        return self.model.run_sampler(noisy_img, steps, self.beta, self.alpha, self.alpha_hat,
                                      clamp_eps=not stochastic, step_noise=step_noise, **seeded)

    @torch.no_grad()
    def denoise_ensemble(self, noisy_img: torch.Tensor, inference_steps: int = 25, members: int = 8, seed: Optional[int] = None,
                         sample_offset: int = 0, member_offset: int = 0, max_batch: int = 16,
                         return_samples: bool = False) -> EnsembleResult:
        """``members`` stochastic (cddpm) draws per image in one native call: their per-pixel mean -- lower error than any
        single draw -- and unbiased standard deviation -- where the network is guessing.  Not a reference call (the reference
        returns one draw, cddpmModels.py:281-308).

        Member m of image b draws the seeded step noise of (seed, sample_offset + b, member_offset + m): member 0 is
        ``denoise(x, seed=seed)``, member m is ``denoise(x, seed=seed, member=m)``.  The B * members (image, member) pairs run as
        the samples of batches of at most ``max_batch`` (16: two programs of 8 on two streams, about 3 GB of workspace at 256x256
        and 12 GB at 512x512; a caller with memory to spare raises it).  ``seed=None`` draws a 64-bit seed from torch's CPU
        generator; the result carries the seed, so the run can be repeated.  ``std`` is None for one member; ``samples``
        ([B, members, C, H, W]) only with ``return_samples=True``.  A DDIM model raises ValueError: a deterministic sampler
        has no ensemble."""
        if getattr(self.model, "variant", "ddim") != "cddpm":
            raise ValueError("denoise_ensemble needs the stochastic (cddpm) variant: a deterministic sampler has no ensemble")
        if seed is None:
            hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
            seed = (hi << 32) | lo
        seed, _ = check_seed(seed, 0)             # (everything else is judged by run_ensemble, before any GPU work)
        self.model.eval()
        steps = timestep_list(self.noise_steps, inference_steps)
        mean, std, samples = self.model.run_ensemble(noisy_img, steps, self.beta, self.alpha, self.alpha_hat, clamp_eps=False,
                                                     members=members, seed=seed, sample_offset=sample_offset,
                                                     member_offset=member_offset, max_batch=max_batch, want_samples=return_samples)
        return EnsembleResult(mean, std, samples, seed)

    # north_star's wording for the same call
    ddim_sample = denoise
