"""The ensemble operators: the seeded step noise as a tensor, mean / std, quantile maps and proper scores over the members of an
ensemble (include/midd.h: mi_step_noise_fill_member, mi_ensemble_reduce, mi_ensemble_quantiles, THE ENSEMBLE SCORES), and what
``DiffusionDenoiser.denoise_ensemble`` returns."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import native
from .rules import _levels_arg, check_levels, check_member, check_quantile_members, check_score_levels, check_seed
from .tensors import _ptr, members_tensor


class EnsembleResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_ensemble`` returns."""
    mean: torch.Tensor                    # [B, C, H, W]: per-pixel mean of the members
    std: Optional[torch.Tensor]           # [B, C, H, W]: unbiased per-pixel standard deviation; None for one member
    samples: Optional[torch.Tensor]       # [B, members, C, H, W] with return_samples=True
    seed: int                             # the seed of the run (drawn when the call had seed=None): pass it to repeat the run


class EnsembleQuantileResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_ensemble(..., quantiles=levels)`` returns: EnsembleResult's fields, then the maps."""
    mean: torch.Tensor
    std: Optional[torch.Tensor]
    samples: Optional[torch.Tensor]
    seed: int
    quantiles: torch.Tensor               # [B, nq, C, H, W]: per-pixel quantile maps of the members, in the order of ``levels``
    levels: Tuple[float, ...]             # the quantile levels, each in [0, 1]


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
    src = members_tensor(samples, "ensemble_reduce")
    B, K = src.shape[:2]
    chw = src[0, 0].numel()
    with torch.cuda.device(src.device):
        mean = torch.empty((B,) + tuple(src.shape[2:]), dtype=torch.float32, device=src.device)
        std = torch.empty_like(mean) if K >= 2 else None
        native.check(native.lib().mi_ensemble_reduce(src.data_ptr(), B, K, chw, mean.data_ptr(), _ptr(std),
                                                     torch.cuda.current_stream(src.device).cuda_stream))
    return mean, std


@torch.no_grad()
def ensemble_quantiles(samples: torch.Tensor, q) -> torch.Tensor:
    """Per-pixel quantile maps [B, nq, ...] over dim 1 of ``samples`` [B, members, ...] at the levels ``q`` (numbers in [0, 1], at
    most 8; members <= 64) with the arithmetic of ``denoise_ensemble(..., quantiles=q)`` (mi_ensemble_quantiles: total-order sort,
    linear interpolation in double precision; a pixel with a NaN member is NaN at every level)."""
    levels = check_levels(q)
    src = members_tensor(samples, "ensemble_quantiles", then=lambda s: check_quantile_members(s.shape[1]))
    B, K = src.shape[:2]
    chw = src[0, 0].numel()
    with torch.cuda.device(src.device):
        out = torch.empty((B, len(levels)) + tuple(src.shape[2:]), dtype=torch.float32, device=src.device)
        native.check(native.lib().mi_ensemble_quantiles(src.data_ptr(), B, K, chw, _levels_arg(levels), len(levels), out.data_ptr(),
                                                        torch.cuda.current_stream(src.device).cuda_stream))
    return out


DEFAULT_SCORE_LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)


class EnsembleScores(NamedTuple):
    """What ``ensemble_scores`` returns (include/midd.h: THE ENSEMBLE SCORES).  Everything but ``crps_map`` lives on the host: the
    scalars are float64 CPU tensors [B] composed in Python floats from the raw ``sums``, the integers int64 CPU tensors."""
    crps: torch.Tensor                    # [B]: mean CRPS of the members' empirical distribution, A/(K N) - G/(K^2 N)
    crps_fair: torch.Tensor               # [B]: the fair (unbiased in K) form, A/(K N) - G/(K (K-1) N); NaN for one member
    rmse: torch.Tensor                    # [B]: root mean squared error of the ensemble mean, sqrt(E/N)
    spread: torch.Tensor                  # [B]: root mean unbiased member variance, sqrt(V/N); ~ rmse for a calibrated ensemble
    rank_hist: torch.Tensor               # int64 [B, 2K+1]: bin 2*lt + eq, the mid-rank of the truth among the members in half steps
    count_lt: torch.Tensor                # int64 [B, nq]: valid pixels with truth <  the level's quantile map
    count_le: torch.Tensor                # int64 [B, nq]: valid pixels with truth <= the level's quantile map
    levels: Tuple[float, ...]             # the quantile levels
    valid: torch.Tensor                   # int64 [B]: N = chw - invalid, the pixels whose truth and members are all finite
    sums: torch.Tensor                    # float64 [B, 4]: the raw (A, G, E, V)
    crps_map: Optional[torch.Tensor]      # float32 [B, ...] on the device with return_map=True: per-pixel CRPS, NaN where invalid

    def coverage(self, lo: int = 0, hi: int = -1) -> torch.Tensor:
        """float64 [B]: the share of valid pixels whose truth lies inside [Q_lo, Q_hi], the quantile maps of ``levels[lo]`` and
        ``levels[hi]`` -- (count_le[:, hi] - count_lt[:, lo]) / valid; compare it with ``levels[hi] - levels[lo]``."""
        return (self.count_le[:, hi] - self.count_lt[:, lo]).to(torch.float64) / self.valid.to(torch.float64)


@torch.no_grad()
def ensemble_scores(samples: torch.Tensor, truth: torch.Tensor, quantiles=DEFAULT_SCORE_LEVELS, return_map: bool = False) -> EnsembleScores:
    """Proper scores of an ensemble ``samples`` [B, K, ...] against ``truth`` [B, ...] in one launch (mi_ensemble_scores; include/midd.h:
    THE ENSEMBLE SCORES): CRPS and fair CRPS, the RMSE of the ensemble mean beside the spread, the rank histogram of the truth among
    the members with exact mid-rank ties, and for every level of ``quantiles`` how many pixels have their truth below that quantile
    map (``EnsembleScores.coverage``: is the 5-95 % interval a 90 % interval?).  K <= 64, at most 8 levels (none: no coverage).  A
    pixel whose truth or any member is not finite is left out of everything and counted (``valid`` = pixels - invalid).  The raw
    outputs are copied to the host once (that waits for the stream); ``return_map=True`` also returns the per-pixel CRPS, which
    stays on the device."""
    levels = check_score_levels(quantiles)
    if not isinstance(samples, torch.Tensor) or samples.dim() < 3 or samples.shape[0] < 1 or samples.shape[1] < 1:
        raise ValueError("samples must be a [B, members, ...] tensor with B >= 1 and members >= 1")
    check_quantile_members(samples.shape[1])
    if not isinstance(truth, torch.Tensor) or tuple(truth.shape) != (samples.shape[0],) + tuple(samples.shape[2:]) or truth.device != samples.device:
        raise ValueError(f"truth must be a tensor of shape {(samples.shape[0],) + tuple(samples.shape[2:])} on {samples.device}: one image per "
                         "ensemble, without the member axis")
    if samples.device.type != "cuda":
        raise RuntimeError(f"ensemble_scores runs only on a ROCm GPU (got {samples.device}): there is no CPU fallback")
    if samples.dtype != torch.float32 or truth.dtype != torch.float32:
        raise TypeError(f"samples and truth must be float32 (got {samples.dtype} and {truth.dtype})")
    src, tru = samples.contiguous(), truth.contiguous()
    B, K = src.shape[:2]
    chw = src[0, 0].numel()
    nq, bins = len(levels), 2 * K + 1
    lib = native.lib()
    dev = src.device
    with torch.cuda.device(dev):
        # one 8-byte-word buffer for the raw outputs [sums B*4 | invalid B | rank_hist B*bins | counts B*nq*2]: one copy to the host
        raw = torch.empty(B * (4 + 1 + bins + 2 * nq), dtype=torch.int64, device=dev)
        o_inv, o_rank, o_cnt = B * 4, B * 5, B * (5 + bins)
        cmap = torch.empty_like(tru) if return_map else None
        nbytes = lib.mi_ensemble_scores_workspace_bytes(B, K, chw)
        if nbytes == 0:
            native.check(-1)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        base = raw.data_ptr()
        native.check(lib.mi_ensemble_scores(src.data_ptr(), tru.data_ptr(), B, K, chw, _levels_arg(levels) if nq else None, nq,
                                            base, base + 8 * o_inv, base + 8 * o_rank, base + 8 * o_cnt if nq else None,
                                            _ptr(cmap), ws.data_ptr(), nbytes,
                                            torch.cuda.current_stream(dev).cuda_stream))
        host = raw.cpu()
    sums = host[:o_inv].view(torch.float64).reshape(B, 4).clone()
    invalid = host[o_inv:o_rank]
    rank_hist = host[o_rank:o_cnt].reshape(B, bins).clone()
    counts = host[o_cnt:].reshape(B, nq, 2)
    valid = chw - invalid
    crps, fair, rmse, spread = [], [], [], []
    nan = float("nan")
    for b in range(B):
        A, G, E, V = (float(v) for v in sums[b])
        N = int(valid[b])
        crps.append(A / (K * N) - G / (K * K * N) if N else nan)
        fair.append(A / (K * N) - G / (K * (K - 1) * N) if N and K > 1 else nan)
        rmse.append((E / N) ** 0.5 if N else nan)
        spread.append((V / N) ** 0.5 if N else nan)
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)
    return EnsembleScores(f64(crps), f64(fair), f64(rmse), f64(spread), rank_hist, counts[:, :, 0].clone(), counts[:, :, 1].clone(), levels,
                          valid.clone(), sums, cmap)
