"""``DiffusionDenoiser``: schedule + reverse loop, same surface as the reference class
(/root/reference/Backend/DDIM/DDIMModel.py:250-289; stochastic cddpm variant
/root/reference/Backend/cddpm/cddpmModels.py:263-308).

The schedule tables are built with the same torch calls as the reference so they are bit
identical; the loop itself (UNet forward + fused x_{t-1} update per timestep) is a single
call into libmidd.so.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import numbers
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


def check_members(members, member_offset, max_batch) -> Tuple[int, int, int]:
    """Argument rules of an ensemble call (include/midd.h: mi_denoise_ensemble) -> (members, member_offset, max_batch)."""
    members, member_offset = check_member(members, "members", low=1), check_member(member_offset, "member_offset")
    max_batch = check_member(max_batch, "max_batch", low=1)
    if member_offset + members > 1 << 32:
        raise ValueError(f"member_offset + members must be <= 2**32 (got {member_offset} + {members})")
    return members, member_offset, max_batch


UPDATE_RULES = ("reference", "ddim", "dpmpp2m")


def check_update(update="reference", eta=0.0, clip_x0=True):
    """Argument rules of the update rule (include/midd.h: THE DDIM UPDATE, THE DPMPP2M UPDATE) -> None for ``"reference"`` (the
    reference's update, the calls and bits of before) or the ``native.UpdateRule`` of ``"ddim"`` / ``"dpmpp2m"`` (kind and
    clip_x0; the native *_dpm calls take no rule struct); raises ValueError before any GPU work.  ``eta`` and ``clip_x0`` belong
    to ``"ddim"``: anything but their defaults together with ``"reference"`` raises; ``"dpmpp2m"`` takes ``clip_x0`` and is
    deterministic, so ``eta`` must stay 0."""
    if update not in UPDATE_RULES:
        raise ValueError(f"update must be 'reference', 'ddim' or 'dpmpp2m' (got {update!r})")
    if isinstance(eta, bool) or not isinstance(eta, numbers.Real) or not 0.0 <= float(eta) <= 1.0:      # (NaN fails the comparison)
        raise ValueError(f"eta must be a number in [0, 1] (got {eta!r})")
    if not isinstance(clip_x0, (bool, int)):
        raise ValueError(f"clip_x0 must be a bool (got {clip_x0!r})")
    if update == "reference":
        if float(eta) != 0.0 or not clip_x0:
            raise ValueError("eta and clip_x0 belong to update='ddim': the reference's update has neither")
        return None
    if update == "dpmpp2m" and float(eta) != 0.0:
        raise ValueError("update='dpmpp2m' is deterministic: it has no eta (an SDE form is not built)")
    return native.UpdateRule(native.MI_UPDATE[update], float(eta), 1 if clip_x0 else 0)


def refuse_update(update, what: str) -> None:
    """The calls the DDIM and DPMPP2M updates are not built for (include/midd.h: NOT BUILT) take ``update`` to say so.  The
    per-slot calls run the rules under another spelling, ``rule=SamplerRule(...)``, which the message names."""
    if update not in UPDATE_RULES:
        raise ValueError(f"update must be 'reference', 'ddim' or 'dpmpp2m' (got {update!r})")
    slots = "for the per-slot calls pass rule=SamplerRule(...) instead: run_slots_rule, denoise_ragged(rule=), SamplerSession(rule=), " \
            "DiffusionService(slot_update=)"
    if update == "dpmpp2m":
        raise ValueError(f"{what} runs the reference's update only: update='dpmpp2m' is built for denoise and denoise_tiled "
                         f"({slots}; ensembles have nothing to draw under it)")
    if update != "reference":
        raise ValueError(f"{what} runs the reference's update only: update='ddim' is built for denoise, denoise_ensemble and "
                         f"denoise_tiled ({slots}; the tiled and the self ensemble do not carry the rule yet)")


@dataclasses.dataclass(frozen=True)
class SamplerRule:
    """The update rule of the per-slot calls (include/midd.h: mi_denoise_slots_rule) -- ``run_slots_rule``, ``denoise_ragged(rule=)``,
    ``SamplerSession(rule=)`` -- as one value: ``update`` "ddim" or "dpmpp2m", ``eta`` and ``clip_x0`` as in ``denoise``.  Judged by
    ``check_update`` when it is made; the reference's update is ``rule=None``, not a SamplerRule."""
    update: str = "ddim"
    eta: float = 0.0
    clip_x0: bool = True

    def __post_init__(self):
        if check_update(self.update, self.eta, self.clip_x0) is None:
            raise ValueError("SamplerRule(update='reference'): the reference's update is rule=None")
        object.__setattr__(self, "eta", float(self.eta))
        object.__setattr__(self, "clip_x0", bool(self.clip_x0))

    @property
    def draws(self) -> bool:
        """Whether the rule has a noise term at all: DDIM with eta > 0."""
        return self.update == "ddim" and self.eta > 0.0

    def native(self):
        return check_update(self.update, self.eta, self.clip_x0)

    def kwargs(self) -> dict:
        """The keywords of ``denoise`` / ``denoise_tiled`` / ``denoise_ensemble`` that name the same rule."""
        return dict(update=self.update, eta=self.eta, clip_x0=self.clip_x0)


def check_rule(rule) -> Optional["SamplerRule"]:
    if rule is not None and not isinstance(rule, SamplerRule):
        raise ValueError(f"rule must be None (the reference's update) or a midd_amd.SamplerRule (got {rule!r})")
    return rule


def ddim_coefficients(t_list: Sequence[int], alpha_hat, eta: float = 0.0):
    """The coefficient table of ``update="ddim"`` for a timestep list (host only; mi_ddim_coefficients): a float32 numpy array
    [len(t_list), 7] of (k0, k1, r0, r1, a, b, s) per iteration, the values the update kernel receives."""
    import numpy as np
    steps = np.ascontiguousarray(np.asarray(list(t_list), dtype=np.int32))
    tab = np.ascontiguousarray(alpha_hat.detach().to("cpu", torch.float32).numpy() if isinstance(alpha_hat, torch.Tensor)
                               else np.asarray(alpha_hat, dtype=np.float32))
    out = np.empty((len(steps), 7), dtype=np.float32)
    native.check(native.lib().mi_ddim_coefficients(steps.ctypes.data_as(C.POINTER(C.c_int32)), len(steps),
                                                   tab.ctypes.data_as(C.POINTER(C.c_float)), int(tab.shape[0]), C.c_double(float(eta)),
                                                   out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def dpm_coefficients(t_list: Sequence[int], alpha_hat):
    """The coefficient table of ``update="dpmpp2m"`` for a timestep list (host only; mi_dpm_coefficients): a float32 numpy array
    [len(t_list), 8] of (k0, k1, r0, r1, a, b, s, g) per iteration -- ``ddim_coefficients`` at eta = 0, then the multistep weight."""
    import numpy as np
    steps = np.ascontiguousarray(np.asarray(list(t_list), dtype=np.int32))
    tab = np.ascontiguousarray(alpha_hat.detach().to("cpu", torch.float32).numpy() if isinstance(alpha_hat, torch.Tensor)
                               else np.asarray(alpha_hat, dtype=np.float32))
    out = np.empty((len(steps), 8), dtype=np.float32)
    native.check(native.lib().mi_dpm_coefficients(steps.ctypes.data_as(C.POINTER(C.c_int32)), len(steps),
                                                  tab.ctypes.data_as(C.POINTER(C.c_float)), int(tab.shape[0]),
                                                  out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


class SamplerTrajectory(NamedTuple):
    """What ``DiffusionDenoiser.denoise(..., update="dpmpp2m", return_x0=True)`` returns."""
    image: torch.Tensor                   # [B, C, H, W]: the call's result, the bits of the call without return_x0
    x0: torch.Tensor                      # [n_iters, B, C, H, W]: the predicted image of every iteration (clipped when clip_x0)


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


MAX_QUANTILE_MEMBERS = 64                 # include/midd.h: mi_ensemble_quantiles sorts a pixel's members in registers
MAX_QUANTILE_LEVELS = 8


def check_levels(q) -> Tuple[float, ...]:
    """Argument rules of the quantile levels (include/midd.h: mi_ensemble_quantiles) -> a tuple of floats; raises ValueError
    before any GPU work.  A single number is one level."""
    if isinstance(q, numbers.Real) and not isinstance(q, bool):
        q = (q,)
    try:
        levels = tuple(q)
    except TypeError:
        raise ValueError(f"quantile levels must be a sequence of numbers in [0, 1] (got {q!r})") from None
    if not 1 <= len(levels) <= MAX_QUANTILE_LEVELS:
        raise ValueError(f"between 1 and {MAX_QUANTILE_LEVELS} quantile levels per call (got {len(levels)})")
    out = []
    for v in levels:
        if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0.0 <= float(v) <= 1.0:      # (NaN fails the comparison)
            raise ValueError(f"every quantile level must be a number in [0, 1] (got {v!r})")
        out.append(float(v))
    return tuple(out)


def check_quantile_members(members: int) -> int:
    if members > MAX_QUANTILE_MEMBERS:
        raise ValueError(f"quantiles need members <= {MAX_QUANTILE_MEMBERS} (got {members}): the kernel sorts a pixel's members in registers")
    return members


def _levels_arg(levels: Tuple[float, ...]):
    return (C.c_double * len(levels))(*levels)


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


@torch.no_grad()
def ensemble_quantiles(samples: torch.Tensor, q) -> torch.Tensor:
    """Per-pixel quantile maps [B, nq, ...] over dim 1 of ``samples`` [B, members, ...] at the levels ``q`` (numbers in [0, 1], at
    most 8; members <= 64) with the arithmetic of ``denoise_ensemble(..., quantiles=q)`` (mi_ensemble_quantiles: total-order sort,
    linear interpolation in double precision; a pixel with a NaN member is NaN at every level)."""
    levels = check_levels(q)
    if not isinstance(samples, torch.Tensor) or samples.dim() < 3 or samples.shape[0] < 1 or samples.shape[1] < 1:
        raise ValueError("samples must be a [B, members, ...] tensor with B >= 1 and members >= 1")
    check_quantile_members(samples.shape[1])
    if samples.device.type != "cuda":
        raise RuntimeError(f"ensemble_quantiles runs only on a ROCm GPU (got {samples.device}): there is no CPU fallback")
    if samples.dtype != torch.float32:
        raise TypeError(f"samples must be float32 (got {samples.dtype})")
    src = samples.contiguous()
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


def check_score_levels(quantiles) -> Tuple[float, ...]:
    """``check_levels``, except that no level at all (None or an empty sequence) is allowed: the scores then carry no coverage."""
    if quantiles is None or (isinstance(quantiles, (tuple, list)) and len(quantiles) == 0):
        return ()
    return check_levels(quantiles)


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
                                            None if cmap is None else cmap.data_ptr(), ws.data_ptr(), nbytes,
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


NPS_ROIS = (32, 64, 128)
NPS_DETREND = {"none": 0, "mean": 1, "plane": 2}


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


def check_nps_args(roi, step, detrend):
    if isinstance(roi, bool) or not isinstance(roi, int) or roi not in NPS_ROIS:
        raise ValueError(f"roi must be one of {NPS_ROIS} (got {roi!r})")
    if step is None:
        step = roi // 2
    if isinstance(step, bool) or not isinstance(step, int) or step < 1:
        raise ValueError(f"step must be an integer >= 1 (got {step!r})")
    if detrend not in NPS_DETREND:
        raise ValueError(f"detrend must be one of {tuple(NPS_DETREND)} (got {detrend!r})")
    return roi, step


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
        native.check(lib.mi_noise_power_spectrum(src.data_ptr(), None if sub is None else sub.data_ptr(), B, K, CH, H, W, roi, step,
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
        native.check(lib.mi_loss_terms(cl.data_ptr(), None if xt is None else xt.data_ptr(), None if eps is None else eps.data_ptr(),
                                       pred.data_ptr(), *tables, 0 if seed is None else 1, C.c_uint64(seed or 0), C.c_int64(sample_offset),
                                       C.c_int64(draw), *counters, native.MI_CLAMP_EPS if clamp_eps else 0, C.c_double(float(edge_weight)),
                                       out.data_ptr(), None if maps is None else maps.data_ptr(), B, Cc, H, W, ws.data_ptr(), ws.numel(),
                                       torch.cuda.current_stream(dev).cuda_stream))
    return out, maps


class TiledResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled`` returns."""
    image: torch.Tensor                   # [B, C, H, W]: the blended image, at the input's own size
    tiles: Optional[torch.Tensor]         # [B, ny * nx, C, th, tw] with return_tiles=True: the denoised tiles, k = ky * nx + kx
    origins_y: Tuple[int, ...]            # row origin of every tile row
    origins_x: Tuple[int, ...]            # column origin of every tile column
    seed: Optional[int]                   # cddpm: the seed of the run (drawn when the call had seed=None); None for DDIM


class TiledEnsembleResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled_ensemble`` returns."""
    mean: torch.Tensor                    # [B, C, H, W]: per-pixel mean of the members' blended images, at the input's own size
    std: Optional[torch.Tensor]           # [B, C, H, W]: unbiased per-pixel standard deviation; None for one member
    samples: Optional[torch.Tensor]       # [B, members, C, H, W] with return_samples=True: every member's blended image
    tiles: Optional[torch.Tensor]         # [members, B, ny * nx, C, th, tw] with return_tiles=True: tiles[m] is a TiledResult.tiles
    origins_y: Tuple[int, ...]            # row origin of every tile row
    origins_x: Tuple[int, ...]            # column origin of every tile column
    seed: int                             # the seed of the run (drawn when the call had seed=None): pass it to repeat the run


class TiledEnsembleQuantileResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled_ensemble(..., quantiles=levels)`` returns: TiledEnsembleResult's fields, then the maps."""
    mean: torch.Tensor
    std: Optional[torch.Tensor]
    samples: Optional[torch.Tensor]
    tiles: Optional[torch.Tensor]
    origins_y: Tuple[int, ...]
    origins_x: Tuple[int, ...]
    seed: int
    quantiles: torch.Tensor               # [B, nq, C, H, W]: per-pixel quantile maps of the members' blended images
    levels: Tuple[float, ...]             # the quantile levels, each in [0, 1]


class TilePlan(NamedTuple):
    """What ``tile_plan`` returns: the tiling of an H x W image (include/midd.h: mi_tile_geometry)."""
    tile: Tuple[int, int]                 # (th, tw)
    overlap: Tuple[int, int]              # (oy, ox): the minimum overlap of neighbouring tiles
    origins_y: Tuple[int, ...]
    origins_x: Tuple[int, ...]


def _pair(v, what: str, low: int) -> Tuple[int, int]:
    a, b = (v if isinstance(v, (tuple, list)) and len(v) == 2 else (v, v))
    return _integer(a, what, 1 << 31, low), _integer(b, what, 1 << 31, low)


def _axis(L: int, T: int, O: int) -> Tuple[int, ...]:
    lib = native.lib()
    n = C.c_int()
    native.check(lib.mi_tile_geometry(L, T, O, C.byref(n), None, 0))
    origins = (C.c_int * n.value)()
    native.check(lib.mi_tile_geometry(L, T, O, C.byref(n), origins, n.value))
    return tuple(origins)


def tile_plan(H: int, W: int, tile, overlap=32) -> TilePlan:
    """The tiling ``denoise_tiled`` uses for an H x W image (host only): ``tile`` and ``overlap`` are ints or (y, x) pairs.
    Raises MiddError for a tile larger than the image or an overlap outside [0, tile / 2]."""
    (th, tw), (oy, ox) = _pair(tile, "tile", 1), _pair(overlap, "overlap", 0)
    H, W = _integer(H, "H", 1 << 31, 1), _integer(W, "W", 1 << 31, 1)
    return TilePlan((th, tw), (oy, ox), _axis(H, th, oy), _axis(W, tw, ox))


def tiling(H: int, W: int, tile, overlap=32) -> Tuple[TilePlan, int, int, int, int, int]:
    """``tile_plan`` with what the native calls take: (plan, th, tw, oy, ox, tiles per image)."""
    plan = tile_plan(H, W, tile, overlap)
    return (plan,) + plan.tile + plan.overlap + (len(plan.origins_y) * len(plan.origins_x),)


def _tile_tensor(x, what: str, dims: int) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dim() != dims or min(x.shape) < 1:
        raise ValueError(f"{what} must be a {dims}-dimensional non-empty tensor")
    if x.device.type != "cuda":
        raise RuntimeError(f"{what} is on {x.device}: tiling runs only on a ROCm GPU, there is no CPU fallback")
    if x.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (got {x.dtype})")
    return x.contiguous()


@torch.no_grad()
def tile_extract(images: torch.Tensor, tile, overlap=32) -> torch.Tensor:
    """[B, C, H, W] -> its tiles [B, ny * nx, C, th, tw] (mi_tile_extract): what ``denoise_tiled`` feeds the sampler."""
    src = _tile_tensor(images, "images", 4)
    B, Cc, H, W = src.shape
    _, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
    with torch.cuda.device(src.device):
        out = torch.empty((B, K, Cc, th, tw), dtype=torch.float32, device=src.device)
        stream = torch.cuda.current_stream(src.device).cuda_stream
        for v0 in range(0, B * K, 65535):
            n = min(65535, B * K - v0)
            native.check(native.lib().mi_tile_extract(src.data_ptr(), B, Cc, H, W, th, tw, oy, ox, v0, n,
                                                      out.data_ptr() + v0 * Cc * th * tw * 4, stream))
    return out


@torch.no_grad()
def tile_blend(tiles: torch.Tensor, H: int, W: int, overlap=32) -> torch.Tensor:
    """tiles [B, ny * nx, C, th, tw] of an H x W tiling -> the blended images [B, C, H, W] with the arithmetic of
    ``denoise_tiled`` (mi_tile_blend: integer ramp windows, double precision, tiles in index order)."""
    src = _tile_tensor(tiles, "tiles", 5)
    B, K, Cc, th, tw = src.shape
    plan = tile_plan(H, W, (th, tw), overlap)
    if K != len(plan.origins_y) * len(plan.origins_x):
        raise ValueError(f"tiles has {K} tiles per image; a {H}x{W} image with tile {th}x{tw} and overlap {plan.overlap} has "
                         f"{len(plan.origins_y)} x {len(plan.origins_x)}")
    with torch.cuda.device(src.device):
        out = torch.empty((B, Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        native.check(native.lib().mi_tile_blend(src.data_ptr(), B, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                out.data_ptr(), torch.cuda.current_stream(src.device).cuda_stream))
    return out


@torch.no_grad()
def tile_blend_reduce(tiles: torch.Tensor, H: int, W: int, overlap=32,
                      return_samples: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """tiles [members, B, ny * nx, C, th, tw] of an H x W tiling -> (mean, std, samples): per-pixel mean and unbiased std
    [B, C, H, W] over the members' blended images and, with ``return_samples``, those images [B, members, C, H, W], in one kernel
    with the arithmetic of ``denoise_tiled_ensemble`` (mi_tile_blend_reduce: ``tile_blend`` per member, then ``ensemble_reduce``
    over the members, bit for bit).  std is None for one member."""
    src = _tile_tensor(tiles, "tiles", 6)
    M, B, K, Cc, th, tw = src.shape
    plan = tile_plan(H, W, (th, tw), overlap)
    if K != len(plan.origins_y) * len(plan.origins_x):
        raise ValueError(f"tiles has {K} tiles per image; a {H}x{W} image with tile {th}x{tw} and overlap {plan.overlap} has "
                         f"{len(plan.origins_y)} x {len(plan.origins_x)}")
    with torch.cuda.device(src.device):
        mean = torch.empty((B, Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        std = torch.empty_like(mean) if M >= 2 else None
        samples = torch.empty((B, M, Cc, int(H), int(W)), dtype=torch.float32, device=src.device) if return_samples else None
        native.check(native.lib().mi_tile_blend_reduce(src.data_ptr(), B, M, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                       mean.data_ptr(), None if std is None else std.data_ptr(),
                                                       None if samples is None else samples.data_ptr(),
                                                       torch.cuda.current_stream(src.device).cuda_stream))
    return mean, std, samples


@torch.no_grad()
def tile_blend_quantiles(tiles: torch.Tensor, H: int, W: int, overlap=32, q=None) -> torch.Tensor:
    """tiles [members, B, ny * nx, C, th, tw] of an H x W tiling -> the per-pixel quantile maps [B, nq, C, H, W] of the members'
    blended images at the levels ``q``, in one kernel with the arithmetic of ``denoise_tiled_ensemble(..., quantiles=q)``
    (mi_tile_blend_quantiles: ``tile_blend`` per member, then ``ensemble_quantiles`` over the members, bit for bit; the blended
    members are never stored).  members <= 64, at most 8 levels."""
    if q is None:
        raise ValueError("tile_blend_quantiles needs the quantile levels: q=(0.05, 0.5, 0.95), say")
    levels = check_levels(q)
    if isinstance(tiles, torch.Tensor) and tiles.dim() == 6:
        check_quantile_members(tiles.shape[0])
    src = _tile_tensor(tiles, "tiles", 6)
    M, B, K, Cc, th, tw = src.shape
    plan = tile_plan(H, W, (th, tw), overlap)
    if K != len(plan.origins_y) * len(plan.origins_x):
        raise ValueError(f"tiles has {K} tiles per image; a {H}x{W} image with tile {th}x{tw} and overlap {plan.overlap} has "
                         f"{len(plan.origins_y)} x {len(plan.origins_x)}")
    with torch.cuda.device(src.device):
        out = torch.empty((B, len(levels), Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        native.check(native.lib().mi_tile_blend_quantiles(src.data_ptr(), B, M, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                          _levels_arg(levels), len(levels), out.data_ptr(),
                                                          torch.cuda.current_stream(src.device).cuda_stream))
    return out


class SelfEnsembleResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_self_ensemble`` returns."""
    mean: torch.Tensor                    # [B, C, H, W]: per-pixel mean over the views, each turned back into the image's frame
    std: Optional[torch.Tensor]           # [B, C, H, W]: unbiased per-pixel standard deviation over the views; None for one view
    samples: Optional[torch.Tensor]       # [B, views, C, H, W] with return_samples=True: the aligned members, in the order of ``views``
    views: Tuple[int, ...]                # the view codes of the run (include/midd.h: THE GEOMETRY), as resolved from the argument
    seed: Optional[int]                   # cddpm: the seed of the run (drawn when the call had seed=None); None for DDIM


class SelfEnsembleQuantileResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_self_ensemble(..., quantiles=levels)`` returns: SelfEnsembleResult's fields, then the maps."""
    mean: torch.Tensor
    std: Optional[torch.Tensor]
    samples: Optional[torch.Tensor]
    views: Tuple[int, ...]
    seed: Optional[int]
    quantiles: torch.Tensor               # [B, nq, C, H, W]: per-pixel quantile maps of the aligned members
    levels: Tuple[float, ...]             # the quantile levels, each in [0, 1]


MAX_VIEWS = 8                             # include/midd.h: view codes g = 4 * transpose + 2 * flip_rows + flip_columns, 0 .. 7
VIEW_SETS = {"flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def view_codes(H: int, W: int, views="auto") -> Tuple[int, ...]:
    """The view list of a self-ensemble over H x W images (host only): ``"auto"`` is all 8 flips and rotations for a square image
    and the 4 that keep the shape otherwise, ``"flips"`` codes 0 .. 3, ``"d4"`` codes 0 .. 7, or a sequence of 1 to 8 distinct
    codes in the order the members are wanted.  Raises ValueError for anything the native call would refuse."""
    H, W = _integer(H, "H", 1 << 31, 1), _integer(W, "W", 1 << 31, 1)
    if isinstance(views, str):
        if views == "auto":
            views = "d4" if H == W else "flips"
        if views not in VIEW_SETS:
            raise ValueError(f"views must be 'auto', 'flips', 'd4' or a sequence of view codes (got {views!r})")
        codes = VIEW_SETS[views]
    else:
        try:
            codes = tuple(views)
        except TypeError:
            raise ValueError(f"views must be 'auto', 'flips', 'd4' or a sequence of view codes (got {views!r})") from None
        if not 1 <= len(codes) <= MAX_VIEWS:
            raise ValueError(f"a view list holds between 1 and {MAX_VIEWS} view codes (got {len(codes)})")
        out = []
        for v in codes:
            try:
                if isinstance(v, bool):
                    raise TypeError
                g = operator.index(v)
            except TypeError:
                raise ValueError(f"every view code must be an integer in [0, 7] (got {v!r})") from None
            if not 0 <= g <= 7:
                raise ValueError(f"every view code must be an integer in [0, 7] (got {v!r})")
            if g in out:
                raise ValueError(f"view code {g} is repeated: the view codes of a list are distinct")
            out.append(g)
        codes = tuple(out)
    for g in codes:
        if g & 4 and H != W:
            raise ValueError(f"view code {g} transposes the image: codes 4 .. 7 need H == W (got {H}x{W}; use views='flips')")
    return codes


def _views_arg(codes: Tuple[int, ...]):
    return (C.c_int32 * len(codes))(*codes)


def _view_tensor(x, what: str, dims: int) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dim() != dims or min(x.shape) < 1:
        raise ValueError(f"{what} must be a {dims}-dimensional non-empty tensor")
    if x.device.type != "cuda":
        raise RuntimeError(f"{what} is on {x.device}: the view kernels run only on a ROCm GPU, there is no CPU fallback")
    if x.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (got {x.dtype})")
    return x.contiguous()


@torch.no_grad()
def dihedral_views(images: torch.Tensor, views="auto") -> torch.Tensor:
    """[B, C, H, W] -> its views [B, G, C, Hv, Wv] (mi_dihedral_views): what ``denoise_self_ensemble`` feeds the sampler.  Bit
    copies; transposing views need H == W, so every view has the image's shape."""
    if isinstance(images, torch.Tensor) and images.dim() == 4:
        codes = view_codes(images.shape[2], images.shape[3], views)
    src = _view_tensor(images, "images", 4)
    B, Cc, H, W = src.shape
    G = len(codes)
    with torch.cuda.device(src.device):
        out = torch.empty((B, G, Cc, H, W), dtype=torch.float32, device=src.device)
        stream = torch.cuda.current_stream(src.device).cuda_stream
        for v0 in range(0, B * G, 65535):
            n = min(65535, B * G - v0)
            native.check(native.lib().mi_dihedral_views(src.data_ptr(), B, Cc, H, W, _views_arg(codes), G, v0, n,
                                                        out.data_ptr() + v0 * Cc * H * W * 4, stream))
    return out


@torch.no_grad()
def dihedral_reduce(view_outputs: torch.Tensor, views="auto",
                    return_samples: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """view_outputs [B, G, C, Hv, Wv], view k in its own frame -> (mean, std, samples): per-pixel mean and unbiased std [B, C, H, W]
    over the views turned back into the image's frame and those aligned members [B, G, C, H, W], in one kernel with the arithmetic
    of ``denoise_self_ensemble`` (mi_dihedral_reduce: unview per view, then ``ensemble_reduce``, bit for bit).  std is None for
    one view; samples is None with ``return_samples=False``."""
    if isinstance(view_outputs, torch.Tensor) and view_outputs.dim() == 5:
        codes = view_codes(view_outputs.shape[3], view_outputs.shape[4], views)
        if len(codes) != view_outputs.shape[1]:
            raise ValueError(f"view_outputs holds {view_outputs.shape[1]} views per image, the view list {len(codes)}")
    src = _view_tensor(view_outputs, "view_outputs", 5)
    B, G, Cc, H, W = src.shape
    with torch.cuda.device(src.device):
        mean = torch.empty((B, Cc, H, W), dtype=torch.float32, device=src.device)
        std = torch.empty_like(mean) if G >= 2 else None
        samples = torch.empty_like(src) if return_samples else None
        native.check(native.lib().mi_dihedral_reduce(src.data_ptr(), B, Cc, H, W, _views_arg(codes), G, mean.data_ptr(),
                                                     None if std is None else std.data_ptr(),
                                                     None if samples is None else samples.data_ptr(),
                                                     torch.cuda.current_stream(src.device).cuda_stream))
    return mean, std, samples


@torch.no_grad()
def dihedral_quantiles(view_outputs: torch.Tensor, views="auto", q=None) -> torch.Tensor:
    """view_outputs [B, G, C, Hv, Wv] -> the per-pixel quantile maps [B, nq, C, H, W] of the aligned members at the levels ``q``
    (mi_dihedral_quantiles: unview per view, then ``ensemble_quantiles``, bit for bit; the aligned members are never stored)."""
    if q is None:
        raise ValueError("dihedral_quantiles needs the quantile levels: q=(0.05, 0.5, 0.95), say")
    levels = check_levels(q)
    if isinstance(view_outputs, torch.Tensor) and view_outputs.dim() == 5:
        codes = view_codes(view_outputs.shape[3], view_outputs.shape[4], views)
        if len(codes) != view_outputs.shape[1]:
            raise ValueError(f"view_outputs holds {view_outputs.shape[1]} views per image, the view list {len(codes)}")
    src = _view_tensor(view_outputs, "view_outputs", 5)
    B, G, Cc, H, W = src.shape
    with torch.cuda.device(src.device):
        out = torch.empty((B, len(levels), Cc, H, W), dtype=torch.float32, device=src.device)
        native.check(native.lib().mi_dihedral_quantiles(src.data_ptr(), B, Cc, H, W, _views_arg(codes), G, _levels_arg(levels), len(levels),
                                                        out.data_ptr(), torch.cuda.current_stream(src.device).cuda_stream))
    return out


class TiledSelfEnsembleResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled_self_ensemble`` returns."""
    mean: torch.Tensor                    # [B, C, H, W]: per-pixel mean over the views' blended images, each turned back, at the input's own size
    std: Optional[torch.Tensor]           # [B, C, H, W]: unbiased per-pixel standard deviation over the views; None for one view
    samples: Optional[torch.Tensor]       # [B, views, C, H, W] with return_samples=True: the aligned blended members, in the order of ``views``
    tiles: Optional[torch.Tensor]         # [views, B, ny * nx, C, th, tw] with return_tiles=True: tiles[k] are view k's tiles in ITS frame
    views: Tuple[int, ...]                # the view codes of the run (include/midd.h: THE GEOMETRY), as resolved from the argument
    origins_y: Tuple[int, ...]            # row origin of every tile row of the UN-TRANSPOSED frame (H x W); a transposing view is cut
    origins_x: Tuple[int, ...]            # by the (W, H) plan: tile_plan(W, H, tile, overlap)
    seed: Optional[int]                   # the seed of the run when it drew noise (drawn when the call had seed=None); else None


class TiledSelfEnsembleQuantileResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled_self_ensemble(..., quantiles=levels)`` returns: TiledSelfEnsembleResult's fields, then the maps."""
    mean: torch.Tensor
    std: Optional[torch.Tensor]
    samples: Optional[torch.Tensor]
    tiles: Optional[torch.Tensor]
    views: Tuple[int, ...]
    origins_y: Tuple[int, ...]
    origins_x: Tuple[int, ...]
    seed: Optional[int]
    quantiles: torch.Tensor               # [B, nq, C, H, W]: per-pixel quantile maps of the aligned blended members
    levels: Tuple[float, ...]             # the quantile levels, each in [0, 1]


def view_codes_tiled(H: int, W: int, tile, overlap=32, views="auto") -> Tuple[int, ...]:
    """The view list of a TILED self-ensemble over H x W images (host only).  A transposed image is still cut into tiles, so the
    transposing codes 4 .. 7 do not need H == W here; they need a square tile and overlap (th == tw and oy == ox), so that the
    W x H frame has as many tiles of the same shape (include/midd.h: TILED SELF-ENSEMBLE).  ``"auto"`` is ``"d4"`` when the tile
    and the overlap are square, whatever H and W, else ``"flips"``; ``"flips"``, ``"d4"`` and sequences as in ``view_codes``.
    Raises ValueError for anything the native call would refuse in the list; the tiling itself is judged by ``tile_plan``."""
    H, W = _integer(H, "H", 1 << 31, 1), _integer(W, "W", 1 << 31, 1)
    (th, tw), (oy, ox) = _pair(tile, "tile", 1), _pair(overlap, "overlap", 0)
    square = th == tw and oy == ox
    if isinstance(views, str) and views == "auto":
        views = "d4" if square else "flips"
    codes = view_codes(1, 1, views)                           # (a 1 x 1 image is square: the list rules without the H == W clause)
    for g in codes:
        if g & 4 and not square:
            raise ValueError(f"view code {g} transposes the image: with tiles, codes 4 .. 7 need a square tile and overlap "
                             f"(got tile {th}x{tw}, overlap {oy}x{ox}; use views='flips')")
    return codes


def _unview_args(tiles, H, W, overlap, views):
    """Shared by the two stand-alone calls: (src, codes, geometry) after every host-side rule."""
    if isinstance(tiles, torch.Tensor) and tiles.dim() == 6:
        th, tw = int(tiles.shape[4]), int(tiles.shape[5])
        codes = view_codes_tiled(H, W, (th, tw), overlap, views)
        if len(codes) != tiles.shape[0]:
            raise ValueError(f"tiles holds {tiles.shape[0]} views, the view list {len(codes)}")
    src = _tile_tensor(tiles, "tiles", 6)
    G, B, K, Cc, th, tw = src.shape
    plan = tile_plan(H, W, (th, tw), overlap)
    if K != len(plan.origins_y) * len(plan.origins_x):
        raise ValueError(f"tiles has {K} tiles per image; a {H}x{W} image with tile {th}x{tw} and overlap {plan.overlap} has "
                         f"{len(plan.origins_y)} x {len(plan.origins_x)}")
    return src, codes, plan


@torch.no_grad()
def tile_blend_unview_reduce(tiles: torch.Tensor, H: int, W: int, overlap=32, views="auto",
                             return_samples: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """tiles [views, B, ny * nx, C, th, tw], view k's tiles in ITS frame (the tiling of the viewed image), of an H x W image ->
    (mean, std, samples): per-pixel mean and unbiased std [B, C, H, W] over the views' blended images turned back into the image's
    frame and, with ``return_samples``, those aligned members [B, views, C, H, W], in one kernel with the arithmetic of
    ``denoise_tiled_self_ensemble`` (mi_tile_blend_unview_reduce: ``tile_blend`` per view in the view's frame, the un-view, then
    ``ensemble_reduce``, bit for bit).  std is None for one view."""
    src, codes, plan = _unview_args(tiles, H, W, overlap, views)
    G, B, K, Cc, th, tw = src.shape
    with torch.cuda.device(src.device):
        mean = torch.empty((B, Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        std = torch.empty_like(mean) if G >= 2 else None
        samples = torch.empty((B, G, Cc, int(H), int(W)), dtype=torch.float32, device=src.device) if return_samples else None
        native.check(native.lib().mi_tile_blend_unview_reduce(src.data_ptr(), B, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                              _views_arg(codes), G, mean.data_ptr(), None if std is None else std.data_ptr(),
                                                              None if samples is None else samples.data_ptr(),
                                                              torch.cuda.current_stream(src.device).cuda_stream))
    return mean, std, samples


@torch.no_grad()
def tile_blend_unview_quantiles(tiles: torch.Tensor, H: int, W: int, overlap=32, views="auto", q=None) -> torch.Tensor:
    """tiles as in ``tile_blend_unview_reduce`` -> the per-pixel quantile maps [B, nq, C, H, W] of the aligned blended members at the
    levels ``q`` (mi_tile_blend_unview_quantiles: ``tile_blend`` per view, the un-view, then ``ensemble_quantiles``, bit for bit; the
    members are never stored)."""
    if q is None:
        raise ValueError("tile_blend_unview_quantiles needs the quantile levels: q=(0.05, 0.5, 0.95), say")
    levels = check_levels(q)
    src, codes, plan = _unview_args(tiles, H, W, overlap, views)
    G, B, K, Cc, th, tw = src.shape
    with torch.cuda.device(src.device):
        out = torch.empty((B, len(levels), Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        native.check(native.lib().mi_tile_blend_unview_quantiles(src.data_ptr(), B, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                                 _views_arg(codes), G, _levels_arg(levels), len(levels), out.data_ptr(),
                                                                 torch.cuda.current_stream(src.device).cuda_stream))
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
        self._alpha_hat_held = None      # (tensor, its version, float32 host copy) of the table the loss calls last saw on THIS denoiser

    def _alpha_hat_host(self):
        """The host copy of ``alpha_hat`` the loss calls pass to the library, made again whenever the attribute is another tensor or
        was written in place.  The entry holds the tensor itself (compared with ``is``), so no other tensor can ever answer to it, and
        it is one tuple read once: threads that share a denoiser see a whole entry."""
        import numpy as np
        ah = self.alpha_hat
        held = getattr(self, "_alpha_hat_held", None)
        if held is None or held[0] is not ah or held[1] != ah._version:
            held = (ah, ah._version, np.array(ah.detach().to("cpu", torch.float32).numpy(), dtype=np.float32, copy=True))
            self._alpha_hat_held = held
        return held[2]

    @torch.no_grad()
    def denoise(self, noisy_img: torch.Tensor, inference_steps: int = 25,
                step_noise: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                sample_offset: int = 0, member: int = 0, *,
                update: str = "reference", eta: float = 0.0, clip_x0: bool = True, return_x0: bool = False):
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

        ``update="ddim"`` (not a reference argument; include/midd.h: THE DDIM UPDATE): the stride-aware DDIM(eta) step -- predict
        x0 from eps, clip it to [0, 1] unless ``clip_x0=False``, re-noise it to the NEXT timestep of the list -- in the place of
        the reference's one-step ancestral update, which on a strided list removes one step's noise per iteration whatever the
        stride.  ``eta=0`` is the deterministic sampler: ``seed`` and ``step_noise`` are ignored for both variants.  ``eta > 0``
        (up to 1, ancestral) adds noise, for BOTH variants, from ``seed`` / ``member`` or ``step_noise`` exactly as above (the
        0.5-scaled convention is kept: the rule's coefficient carries the factor 2); without either, torch.randn up front.
        ``update="reference"`` (the default) is the call of before, bit for bit; ``eta`` or ``clip_x0`` with it raise ValueError.

        ``update="dpmpp2m"`` (not a reference argument; include/midd.h: THE DPMPP2M UPDATE): the second-order multistep step --
        the DDIM (eta = 0) step plus ``g * (x0 - x0_prev)``, the previous iteration's predicted image reused at no extra network
        evaluation, the extrapolation weight bounded at its uniform-step value.  Deterministic for both variants: ``eta != 0``,
        ``seed``, ``step_noise`` or ``member`` raise ValueError.  ``return_x0=True`` (this rule only; any other raises) returns
        ``SamplerTrajectory(image, x0)`` with ``x0`` [n_iters, B, C, H, W], the predicted image of every iteration; ``image`` is
        the bits of the call without it.
        """
        rule = check_update(update, eta, clip_x0)
        dpm = rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"]
        if return_x0 and not dpm:
            raise ValueError("return_x0 belongs to update='dpmpp2m': the other rules do not store the predicted image")
        if dpm:
            if seed is not None or step_noise is not None or member != 0:
                raise ValueError("update='dpmpp2m' is deterministic: it takes no seed, step_noise or member")
            self.model.eval()
            steps = timestep_list(self.noise_steps, inference_steps)
            res = self.model.run_sampler(noisy_img, steps, self.beta, self.alpha, self.alpha_hat,
                                         clamp_eps=getattr(self.model, "variant", "ddim") != "cddpm",
                                         update=update, clip_x0=clip_x0, return_x0=return_x0)
            return SamplerTrajectory(*res) if return_x0 else res
        if seed is not None:
            if step_noise is not None:
                raise ValueError("pass either seed (noise drawn on the device) or step_noise (a noise tensor), not both")
            seed, sample_offset = check_seed(seed, sample_offset)
        self.model.eval()
        steps = timestep_list(self.noise_steps, inference_steps)
        stochastic = getattr(self.model, "variant", "ddim") == "cddpm"
        draws = stochastic if rule is None else rule.eta > 0.0      # whether the call has a noise term at all
        if draws and step_noise is None and seed is None and member == 0:      # (a member without a seed: run_sampler refuses)
            step_noise = 0.5 * torch.randn((len(steps),) + tuple(noisy_img.shape), device=noisy_img.device)
        if not draws:
            step_noise = seed = None
            member = 0
        seeded = {"member": member} if seed is None else {"seed": seed, "sample_offset": sample_offset, "member": member}
        if rule is not None:
            seeded.update(update=update, eta=eta, clip_x0=clip_x0)
        return self.model.run_sampler(noisy_img, steps, self.beta, self.alpha, self.alpha_hat,
                                      clamp_eps=not stochastic, step_noise=step_noise, **seeded)

    @torch.no_grad()
    def denoise_ensemble(self, noisy_img: torch.Tensor, inference_steps: int = 25, members: int = 8, seed: Optional[int] = None,
                         sample_offset: int = 0, member_offset: int = 0, max_batch: int = 16,
                         return_samples: bool = False, quantiles=None, *,
                         update: str = "reference", eta: float = 0.0, clip_x0: bool = True):
        """``members`` stochastic (cddpm) draws per image in one native call: their per-pixel mean -- lower error than any
        single draw -- and unbiased standard deviation -- where the network is guessing.  Not a reference call (the reference
        returns one draw, cddpmModels.py:281-308).

        Member m of image b draws the seeded step noise of (seed, sample_offset + b, member_offset + m): member 0 is
        ``denoise(x, seed=seed)``, member m is ``denoise(x, seed=seed, member=m)``.  The B * members (image, member) pairs run as
        the samples of batches of at most ``max_batch`` (16: two programs of 8 on two streams, about 3 GB of workspace at 256x256
        and 12 GB at 512x512; a caller with memory to spare raises it).  ``seed=None`` draws a 64-bit seed from torch's CPU
        generator; the result carries the seed, so the run can be repeated.  ``std`` is None for one member; ``samples``
        ([B, members, C, H, W]) only with ``return_samples=True``.  A DDIM model raises ValueError: a deterministic sampler
        has no ensemble.

        ``quantiles`` (a sequence of at most 8 levels in [0, 1], e.g. ``(0.05, 0.5, 0.95)``; members <= 64): the call also returns
        the per-pixel quantile maps of the members -- a median and an interval describe outputs clamped to [0, 1] where mean and
        std do not -- as an ``EnsembleQuantileResult``: the fields above, then ``quantiles`` [B, nq, C, H, W] and ``levels``.  The
        members are written to a tensor of the call's own instead of the workspace (which shrinks by the same bytes) and one
        ``ensemble_quantiles`` launch follows on the same stream; mean, std and samples are the bits of the call without it.

        ``update="ddim"`` with ``eta > 0`` (see ``denoise``): the members are draws of the DDIM(eta) sampler, for EITHER variant --
        member m is ``denoise(x, update="ddim", eta=eta, seed=seed, member=m)``.  ``eta=0`` is deterministic and raises as the
        DDIM variant does."""
        levels = None if quantiles is None else check_levels(quantiles)
        rule = check_update(update, eta, clip_x0)
        stochastic = getattr(self.model, "variant", "ddim") == "cddpm"
        if rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"]:
            raise ValueError("denoise_ensemble with update='dpmpp2m': a deterministic sampler has no ensemble")
        if rule is not None and rule.eta == 0.0:
            raise ValueError("denoise_ensemble with update='ddim' needs eta > 0: a deterministic sampler has no ensemble")
        if rule is None and not stochastic:
            raise ValueError("denoise_ensemble needs the stochastic (cddpm) variant: a deterministic sampler has no ensemble")
        seed, _ = check_seed(self._draw_seed() if seed is None else seed, 0)      # (everything else is judged by run_ensemble, before any GPU work)
        if levels is not None:
            check_quantile_members(check_member(members, "members", low=1))
        self.model.eval()
        steps = timestep_list(self.noise_steps, inference_steps)
        rule_kw = {} if rule is None else dict(update=update, eta=eta, clip_x0=clip_x0)
        mean, std, samples = self.model.run_ensemble(noisy_img, steps, self.beta, self.alpha, self.alpha_hat, clamp_eps=not stochastic,
                                                     members=members, seed=seed, sample_offset=sample_offset,
                                                     member_offset=member_offset, max_batch=max_batch,
                                                     want_samples=return_samples or levels is not None, **rule_kw)
        if levels is None:
            return EnsembleResult(mean, std, samples, seed)
        maps = ensemble_quantiles(samples, levels)
        return EnsembleQuantileResult(mean, std, samples if return_samples else None, seed, maps, levels)

    @torch.no_grad()
    def denoise_tiled(self, noisy_img: torch.Tensor, inference_steps: int = 25, tile=256, overlap=32, max_batch: int = 16,
                      seed: Optional[int] = None, sample_offset: int = 0, return_tiles: bool = False,
                      step_noise: None = None, *, update: str = "reference", eta: float = 0.0, clip_x0: bool = True) -> TiledResult:
        """Denoises images of ANY size >= the tile at their own resolution (not a reference call: the reference resizes every
        image to the training size first): every image is cut into overlapping ``tile`` x ``tile`` crops (``tile``: an int or
        (th, tw), a shape the network takes, i.e. multiples of 8; ``overlap``: an int or (oy, ox), at most tile / 2), the
        B * tiles crops run through the sampler as batches of at most ``max_batch``, and a window-weighted blend with fixed
        arithmetic puts them back (``tile_plan`` / ``tile_blend``; include/midd.h: mi_denoise_tiled).  H and W need not be
        multiples of 8.

        cddpm: the step noise is the seeded generator's, indexed by the pixel's place in the WHOLE image -- the noise field
        belongs to the image, overlapping tiles see the same noise -- so ``tile == image size`` is ``denoise(x, seed=s)`` bit
        for bit; ``seed=None`` draws a seed as ``denoise_ensemble`` does and returns it.  A caller's ``step_noise`` tensor is
        not supported here (the argument exists to say so: anything but None raises ValueError).  DDIM: ``seed`` must be None.

        ``update="ddim"`` (see ``denoise``): every tile runs the DDIM(eta) update.  ``eta=0``: deterministic for both variants, a
        ``seed`` is ignored and the result's ``seed`` is None.  ``eta > 0``: seeded as cddpm is above, for BOTH variants.
        ``update="dpmpp2m"``: every tile runs the second-order multistep update with a history of its own; deterministic, so a
        ``seed`` raises ValueError and the result's ``seed`` is None.  There is no trajectory for tiles."""
        rule = check_update(update, eta, clip_x0)
        if rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"] and seed is not None:
            raise ValueError("update='dpmpp2m' is deterministic: denoise_tiled takes no seed with it")
        if step_noise is not None:
            raise ValueError("denoise_tiled does not take a step_noise tensor: its noise is the seeded generator's, indexed by "
                             "image position (pass seed; midd_amd.step_noise(seed, n, x.shape) exports the same values)")
        stochastic = getattr(self.model, "variant", "ddim") == "cddpm"
        draws = stochastic if rule is None else rule.eta > 0.0
        if rule is None and not stochastic and seed is not None:
            raise ValueError("seed selects the step noise of the stochastic (cddpm) variant: the DDIM variant takes seed=None")
        if draws:
            seed, sample_offset = check_seed(self._draw_seed() if seed is None else seed, sample_offset)
        else:
            seed = None
        self.model.eval()
        steps = timestep_list(self.noise_steps, inference_steps)
        rule_kw = {} if rule is None else dict(update=update, eta=eta, clip_x0=clip_x0)
        image, tiles, plan = self.model.run_tiled(noisy_img, steps, self.beta, self.alpha, self.alpha_hat, clamp_eps=not stochastic,
                                                  tile=tile, overlap=overlap, seed=seed, sample_offset=sample_offset,
                                                  max_batch=max_batch, want_tiles=return_tiles, **rule_kw)
        return TiledResult(image, tiles, plan.origins_y, plan.origins_x, seed)

    @torch.no_grad()
    def denoise_tiled_ensemble(self, noisy_img: torch.Tensor, inference_steps: int = 25, members: int = 8, tile=256, overlap=32,
                               max_batch: int = 16, seed: Optional[int] = None, sample_offset: int = 0, member_offset: int = 0,
                               return_samples: bool = False, return_tiles: bool = False,
                               step_noise: None = None, quantiles=None, *, update: str = "reference"):
        """``denoise_ensemble`` for images of ANY size >= the tile: ``members`` stochastic (cddpm) draws of every image as blended
        overlapping tiles in one native call, their per-pixel mean and unbiased standard deviation at the image's own resolution
        (not a reference call; include/midd.h: mi_denoise_tiled_ensemble).

        Member m is ``denoise_tiled(x, seed=seed, sample_offset=sample_offset)`` with the member word ``member_offset + m`` of the
        seeded step noise: with one member at offset 0, ``mean`` is that call's image bit for bit, and a tile of member m is
        ``denoise(crop, step_noise=crop of midd_amd.step_noise(seed, n, x.shape, sample_offset, member=member_offset + m))``.
        Members run one after the other; inside a member the B * tiles crops run as batches of at most ``max_batch`` (the pass
        size is min(max_batch, B * tiles); a batch never mixes members).  ``mean`` and ``std`` are ``ensemble_reduce`` of the
        members' ``tile_blend`` images, computed by one kernel that never stores those images unless ``return_samples=True``
        (``samples``: [B, members, C, H, W]).  ``tiles`` ([members, B, ny * nx, C, th, tw], ``return_tiles=True``): ``tiles[m]`` is
        what ``denoise_tiled(..., return_tiles=True).tiles`` is for member m.  ``std`` is None for one member.  ``seed=None`` draws
        a 64-bit seed and returns it.  A DDIM model raises ValueError (a deterministic sampler has no ensemble); a ``step_noise``
        tensor is not supported (anything but None raises ValueError).

        ``quantiles`` (a sequence of at most 8 levels in [0, 1]; members <= 64): the call also returns the per-pixel quantile maps
        of the members' blended images as a ``TiledEnsembleQuantileResult``: the fields above, then ``quantiles``
        [B, nq, C, H, W] and ``levels``.  The tiles are written to a tensor of the call's own instead of the workspace (which
        shrinks by the same bytes) and one ``tile_blend_quantiles`` launch follows on the same stream: the blended members are
        still never stored.  The other fields are the bits of the call without it."""
        refuse_update(update, "denoise_tiled_ensemble")
        levels = None if quantiles is None else check_levels(quantiles)
        if step_noise is not None:
            raise ValueError("denoise_tiled_ensemble does not take a step_noise tensor: its noise is the seeded generator's, indexed by "
                             "image position and member (pass seed; midd_amd.step_noise(seed, n, x.shape, member=m) exports the same values)")
        if getattr(self.model, "variant", "ddim") != "cddpm":
            raise ValueError("denoise_tiled_ensemble needs the stochastic (cddpm) variant: a deterministic sampler has no ensemble")
        seed, _ = check_seed(self._draw_seed() if seed is None else seed, 0)      # (everything else is judged by run_tiled_ensemble, before any GPU work)
        if levels is not None:
            check_quantile_members(check_member(members, "members", low=1))
        self.model.eval()
        steps = timestep_list(self.noise_steps, inference_steps)
        mean, std, samples, tiles, plan = self.model.run_tiled_ensemble(
            noisy_img, steps, self.beta, self.alpha, self.alpha_hat, clamp_eps=False, tile=tile, overlap=overlap, members=members,
            seed=seed, sample_offset=sample_offset, member_offset=member_offset, max_batch=max_batch,
            want_samples=return_samples, want_tiles=return_tiles or levels is not None)
        if levels is None:
            return TiledEnsembleResult(mean, std, samples, tiles, plan.origins_y, plan.origins_x, seed)
        maps = tile_blend_quantiles(tiles, noisy_img.shape[2], noisy_img.shape[3], plan.overlap, levels)
        return TiledEnsembleQuantileResult(mean, std, samples, tiles if return_tiles else None, plan.origins_y, plan.origins_x, seed, maps, levels)

    @torch.no_grad()
    def denoise_self_ensemble(self, noisy_img: torch.Tensor, inference_steps: int = 25, views="auto", seed: Optional[int] = None,
                              sample_offset: int = 0, member_offset: int = 0, max_batch: int = 16,
                              return_samples: bool = False, quantiles=None, *, update: str = "reference"):
        """The geometric self-ensemble ("x8 test-time augmentation") in one native call, for BOTH variants: the network runs on
        the flipped and rotated copies of every image, every output is turned back, and the call returns their per-pixel mean --
        the usual few tenths of a dB over a single run -- and unbiased standard deviation: where the output depends on the
        orientation.  Not a reference call (the reference denoises the image as given, DDIMModel.py:268-289).

        ``views``: ``"auto"`` (all 8 flips and rotations of a square image, the 4 shape-keeping ones otherwise), ``"flips"``,
        ``"d4"`` or a sequence of 1 to 8 distinct view codes g = 4 * transpose + 2 * flip_rows + flip_columns (``view_codes``;
        include/midd.h: THE GEOMETRY); codes 4 .. 7 need H == W.  The B * views (image, view) pairs run as the samples of batches
        of at most ``max_batch``.  Member k is ``unview(denoise(view(x, g_k)), g_k)`` -- bit for bit with ``batch_invariant=True``
        -- and ``mean``, ``std`` are ``ensemble_reduce`` of the members in list order, computed by one kernel that never stores
        them unless ``return_samples=True`` (``samples``: [B, views, C, H, W]).  ``std`` is None for one view.

        DDIM: ``seed`` must be None; the result's ``seed`` is None.  cddpm: always seeded -- view k of image b draws the step
        noise of (seed, sample_offset + b, member_offset + k) at the pixel's place in the VIEW's frame, i.e. member k is
        ``denoise(view(x), seed=seed, sample_offset=sample_offset + b, member=member_offset + k)`` turned back; ``seed=None`` draws
        a 64-bit seed and returns it.

        ``quantiles`` (a sequence of at most 8 levels in [0, 1]): the call also returns the per-pixel quantile maps of the aligned
        members as a ``SelfEnsembleQuantileResult``: the fields above, then ``quantiles`` [B, nq, C, H, W] and ``levels``.  One
        ``dihedral_quantiles`` launch follows on the same stream and reads the view outputs from the call's workspace; mean, std
        and samples are the bits of the call without it."""
        refuse_update(update, "denoise_self_ensemble")
        levels = None if quantiles is None else check_levels(quantiles)
        stochastic = getattr(self.model, "variant", "ddim") == "cddpm"
        if not stochastic and seed is not None:
            raise ValueError("seed selects the step noise of the stochastic (cddpm) variant: the DDIM variant takes seed=None")
        if isinstance(noisy_img, torch.Tensor) and noisy_img.dim() == 4:
            views = view_codes(noisy_img.shape[2], noisy_img.shape[3], views)      # (before any GPU work; run_self_ensemble judges the rest)
        if stochastic:
            seed, _ = check_seed(self._draw_seed() if seed is None else seed, 0)
        self.model.eval()
        steps = timestep_list(self.noise_steps, inference_steps)
        mean, std, samples, codes, maps = self.model.run_self_ensemble(
            noisy_img, steps, self.beta, self.alpha, self.alpha_hat, clamp_eps=not stochastic, views=views, seed=seed,
            sample_offset=sample_offset, member_offset=member_offset, max_batch=max_batch, want_samples=return_samples, levels=levels)
        if levels is None:
            return SelfEnsembleResult(mean, std, samples, codes, seed)
        return SelfEnsembleQuantileResult(mean, std, samples, codes, seed, maps, levels)

    @torch.no_grad()
    def denoise_tiled_self_ensemble(self, noisy_img: torch.Tensor, inference_steps: int = 25, views="auto", tile=256, overlap=32,
                                    max_batch: int = 16, seed: Optional[int] = None, sample_offset: int = 0, member_offset: int = 0,
                                    return_samples: bool = False, return_tiles: bool = False, quantiles=None, *,
                                    update: str = "reference", eta: float = 0.0, clip_x0: bool = True):
        """``denoise_self_ensemble`` for images of ANY size >= the tile, for BOTH variants: the flip / rotate views of every image,
        each denoised as blended overlapping tiles, turned back, and their per-pixel mean and unbiased standard deviation at the
        image's own resolution, in one native call (not a reference call; include/midd.h: mi_denoise_tiled_self_ensemble).  It is
        the ensemble a deterministic (DDIM) model has for a full-resolution image.

        ``views`` (``view_codes_tiled``): ``"auto"`` is all 8 flips and rotations when ``tile`` and ``overlap`` are square --
        whatever H and W: a transposed image is still cut into tiles -- and the 4 flips otherwise; ``"flips"``, ``"d4"`` or a
        sequence of 1 to 8 distinct codes.  A view's tiles are the tiles of the VIEWED image (a transposing view uses the (W, H)
        plan, ``tile_plan(W, H, tile, overlap)``), so member k is ``unview(denoise_tiled(view(x, g_k)).image, g_k)`` at the same
        ``max_batch``, bit for bit.  Views run one after the other; inside a view the B * tiles crops run as batches of at most
        ``max_batch`` (a batch never mixes views).  ``mean`` and ``std`` are ``ensemble_reduce`` of the members in list order,
        computed by one kernel that never stores them unless ``return_samples=True`` (``samples``: [B, views, C, H, W]).
        ``tiles`` ([views, B, ny * nx, C, th, tw], ``return_tiles=True``): ``tiles[k]`` is ``denoise_tiled(view(x, g_k),
        return_tiles=True).tiles``, in view k's frame.  ``origins_y`` / ``origins_x`` are those of the un-transposed frame.
        ``std`` is None for one view.

        DDIM: ``seed`` must be None; the result's ``seed`` is None.  cddpm: always seeded -- view k draws the member word
        ``member_offset + k`` at the pixel's place in the whole VIEWED image, i.e. member k is the single sample of
        ``denoise_tiled_ensemble(view(x), members=1, seed=seed, member_offset=member_offset + k)`` turned back; ``views=[0]`` is
        ``denoise_tiled(x, seed=seed)``.  ``seed=None`` draws a 64-bit seed and returns it.

        ``update="ddim"`` (see ``denoise_tiled``): every tile of every view runs the DDIM(eta) update; ``eta=0`` is deterministic
        for both variants (a ``seed`` is ignored, the result's is None), ``eta > 0`` is seeded as cddpm is above, for BOTH
        variants.  ``update="dpmpp2m"`` is not built for this call and raises ValueError.

        ``quantiles`` (a sequence of at most 8 levels in [0, 1]): the call also returns the per-pixel quantile maps of the aligned
        blended members as a ``TiledSelfEnsembleQuantileResult``: the fields above, then ``quantiles`` [B, nq, C, H, W] and
        ``levels``.  The tiles are written to a tensor of the call's own instead of the workspace and one
        ``tile_blend_unview_quantiles`` launch follows on the same stream; the other fields are the bits of the call without it.

        Not built: a session ticket (``submit_...``) and a service switch for this call."""
        rule = check_update(update, eta, clip_x0)
        if rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"]:
            raise ValueError("denoise_tiled_self_ensemble runs the reference's update or update='ddim': update='dpmpp2m' is not built "
                             "for it (the native call takes no history buffer; denoise and denoise_tiled run it)")
        levels = None if quantiles is None else check_levels(quantiles)
        stochastic = getattr(self.model, "variant", "ddim") == "cddpm"
        draws = stochastic if rule is None else rule.eta > 0.0
        if rule is None and not stochastic and seed is not None:
            raise ValueError("seed selects the step noise of the stochastic (cddpm) variant: the DDIM variant takes seed=None")
        if isinstance(noisy_img, torch.Tensor) and noisy_img.dim() == 4:
            views = view_codes_tiled(noisy_img.shape[2], noisy_img.shape[3], tile, overlap, views)      # (before any GPU work)
        if draws:
            seed, sample_offset = check_seed(self._draw_seed() if seed is None else seed, sample_offset)
        else:
            seed = None
        self.model.eval()
        steps = timestep_list(self.noise_steps, inference_steps)
        rule_kw = {} if rule is None else dict(update=update, eta=eta, clip_x0=clip_x0)
        mean, std, samples, tiles, codes, plan = self.model.run_tiled_self_ensemble(
            noisy_img, steps, self.beta, self.alpha, self.alpha_hat, clamp_eps=not stochastic, tile=tile, overlap=overlap, views=views,
            seed=seed, sample_offset=sample_offset, member_offset=member_offset, max_batch=max_batch, want_samples=return_samples,
            want_tiles=return_tiles or levels is not None, **rule_kw)
        if levels is None:
            return TiledSelfEnsembleResult(mean, std, samples, tiles, codes, plan.origins_y, plan.origins_x, seed)
        maps = tile_blend_unview_quantiles(tiles, noisy_img.shape[2], noisy_img.shape[3], plan.overlap, codes, levels)
        return TiledSelfEnsembleQuantileResult(mean, std, samples, tiles if return_tiles else None, codes, plan.origins_y, plan.origins_x,
                                               seed, maps, levels)

    @torch.no_grad()
    def score_ensemble(self, clean: torch.Tensor, noisy: torch.Tensor, inference_steps: int = 25, members: int = 8, seed: Optional[int] = None,
                       sample_offset: int = 0, member_offset: int = 0, max_batch: int = 16, quantiles=DEFAULT_SCORE_LEVELS,
                       tile=None, overlap=32, return_map: bool = False):
        """An ensemble of ``noisy`` scored against ``clean`` -> ``(result, scores)``: ``denoise_ensemble(noisy, ..., return_samples=True)``
        -- or, with ``tile``, ``denoise_tiled_ensemble(noisy, ..., tile=tile, overlap=overlap, return_samples=True)``, whose blended
        members are scored -- followed by ``ensemble_scores(result.samples, clean, quantiles, return_map)``, bit for bit that
        composition.  ``scores`` answers whether the std and quantile maps of this checkpoint at these ``members``,
        ``inference_steps`` mean anything: ``scores.rmse`` beside ``scores.spread``, ``scores.coverage()`` beside the levels,
        ``scores.rank_hist``.  members <= 64."""
        levels = check_score_levels(quantiles)
        check_quantile_members(check_member(members, "members", low=1))
        if not isinstance(clean, torch.Tensor) or not isinstance(noisy, torch.Tensor) or clean.shape != noisy.shape or clean.device != noisy.device:
            raise ValueError("clean must be a tensor of the noisy images' shape, on their device")
        if clean.dtype != torch.float32:
            raise TypeError(f"clean must be float32 (got {clean.dtype})")
        if tile is None:
            result = self.denoise_ensemble(noisy, inference_steps, members, seed, sample_offset, member_offset, max_batch, return_samples=True)
        else:
            result = self.denoise_tiled_ensemble(noisy, inference_steps, members, tile, overlap, max_batch, seed, sample_offset, member_offset,
                                                 return_samples=True)
        return result, ensemble_scores(result.samples, clean, levels, return_map)

    @torch.no_grad()
    def ensemble_nps(self, noisy: torch.Tensor, inference_steps: int = 25, members: int = 8, seed: Optional[int] = None, sample_offset: int = 0,
                     member_offset: int = 0, max_batch: int = 16, tile=None, overlap=32, roi: int = 64, step: Optional[int] = None,
                     detrend: str = "plane", window="hann", exclude_axes: bool = False):
        """An ensemble of ``noisy`` and the noise power spectrum of its spread -> ``(result, nps)``: ``denoise_ensemble(noisy, ...,
        return_samples=True)`` -- or, with ``tile``, ``denoise_tiled_ensemble(noisy, ..., tile=tile, overlap=overlap,
        return_samples=True)`` -- followed by ``noise_power_spectrum(result.samples, result.mean, roi, step, detrend, window,
        scale=members / (members - 1), exclude_axes)``, bit for bit that composition.  The std map says how much each pixel varies
        between members; ``nps`` says at which spatial scales (the scale K / (K - 1) makes the deviations from the ensemble mean an
        unbiased variance).  members >= 2."""
        if check_member(members, "members", low=1) < 2:
            raise ValueError("ensemble_nps needs members >= 2: one member has no spread around its own mean")
        check_nps_args(roi, step, detrend)
        nps_window(window, roi)
        if tile is None:
            result = self.denoise_ensemble(noisy, inference_steps, members, seed, sample_offset, member_offset, max_batch, return_samples=True)
        else:
            result = self.denoise_tiled_ensemble(noisy, inference_steps, members, tile, overlap, max_batch, seed, sample_offset, member_offset,
                                                 return_samples=True)
        return result, noise_power_spectrum(result.samples, result.mean, roi, step, detrend, window, members / (members - 1), exclude_axes)

    # ------------------------------------------------------------------ the training objective as an evaluation
    def sample_timesteps(self, n: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``torch.randint(1, noise_steps, (n,))`` on the model's device -- DDIMModel.py:265-266."""
        return torch.randint(low=1, high=self.noise_steps, size=(n,), generator=generator).to(self.beta.device)

    @torch.no_grad()
    def noise_images(self, x: torch.Tensor, t, seed: Optional[int] = None, sample_offset: int = 0, draw: int = 0,
                     noise: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(x_t, eps) = denoiser.noise_images(x, t) -- DDIMModel.py:259-263, on the device (mi_noise_images).

        With neither ``seed`` nor ``noise`` eps is ``torch.randn_like(x)`` as in the reference; ``noise`` is the caller's tensor;
        ``seed`` (not a reference argument) draws eps on the device from the counter generator of the seeded sampler with counter
        words that no sampler step uses (include/midd.h: THE FORWARD NOISE): a pure function of (seed, sample_offset + b, draw,
        element), so the same arguments give the same bits again on any batch split.  x_t has the bits of the reference's
        expression in torch eager on a CPU given the same eps."""
        if seed is None and noise is None:
            if not isinstance(x, torch.Tensor):
                raise ValueError("x must be a [B, C, H, W] tensor")
            noise = torch.randn_like(x)
        return noise_images(x, t, self._alpha_hat_host(), seed=seed, sample_offset=sample_offset, draw=draw, noise=noise)

    def _objective(self, edge_weight) -> Tuple[bool, float]:
        """(clamp_eps, edge_weight) of the variant's training objective: DDIMModel.py:358,375 / cddpmModels.py:374."""
        ddim = getattr(self.model, "variant", "ddim") != "cddpm"
        if edge_weight is None:
            return ddim, 0.2 if ddim else 0.0
        w = float(edge_weight)
        if w != w:
            raise ValueError("edge_weight must not be NaN")
        return ddim, w

    @torch.no_grad()
    def denoising_loss(self, clean: torch.Tensor, noisy: torch.Tensor, t=None, seed: Optional[int] = None, sample_offset: int = 0,
                       draw: int = 0, noise: Optional[torch.Tensor] = None, edge_weight: Optional[float] = None,
                       return_maps: bool = False) -> DenoisingLoss:
        """The objective the checkpoint was trained on, per sample, for (clean, noisy) pairs at timesteps ``t`` -- DDIMModel.py:351-375
        (cddpm: cddpmModels.py:367-374) without the optimiser: noise ``clean`` to x_t, one forward conditioned on ``noisy``, compare
        (mi_denoising_loss: one native call, no host synchronisation inside).

        ``loss = mse + edge_weight * edge``; ``mse`` is the mean squared error of the predicted noise, ``edge`` the mean absolute
        difference of the Sobel edge magnitudes of the predicted clean image and of ``clean``; float64 [B] each (the reference's
        scalars are their batch means).  ``edge_weight=None``: the variant's own objective (DDIM: eps clamped to +-5, weight 0.2;
        cddpm: no clamp, weight 0 -- the edge term is still reported).  ``t=None`` draws timesteps with ``sample_timesteps``;
        ``seed=None`` with ``noise=None`` draws a seed, which the result carries so that the call can be repeated.  ``sample_offset``,
        ``draw``: as ``noise_images``.  ``return_maps``: the per-pixel q, g and p as ``maps``; the scalars are the same bits."""
        if not isinstance(clean, torch.Tensor) or clean.dim() != 4:
            raise ValueError("clean must be a [B, C, H, W] tensor")
        if seed is not None and noise is not None:
            raise ValueError("pass either seed (noise drawn on the device) or noise (a tensor), not both")
        if seed is None and noise is None:
            seed = self._draw_seed()
        clamp, weight = self._objective(edge_weight)
        t = self.sample_timesteps(clean.shape[0]) if t is None else torch.as_tensor(t).reshape(-1)
        if self.model.training:      # (eval() walks every submodule: half a millisecond on the full network, more than the two new launches)
            self.model.eval()
        out, maps = self.model.run_denoising_loss(clean, noisy, t, self._alpha_hat_host(), clamp, weight, noise=noise, seed=seed,
                                                  sample_offset=sample_offset, draw=draw, return_maps=return_maps)
        return DenoisingLoss(out[:, 2], out[:, 0], out[:, 1], t.to(clean.device), seed, None if maps is None else LossMaps(*maps))

    @torch.no_grad()
    def loss_profile(self, clean: torch.Tensor, noisy: torch.Tensor, timesteps=None, seed: Optional[int] = None, max_batch: int = 16,
                     sample_offset: int = 0, edge_weight: Optional[float] = None) -> LossProfile:
        """The loss of every image at every timestep of ``timesteps`` (default: all of ``range(noise_steps)``) -> ``LossProfile`` with
        [T, B] arrays: which timesteps the checkpoint is good at, without a sampler run.

        The B * T (image, timestep) pairs run in passes of at most ``max_batch`` through the call behind ``denoising_loss`` with
        per-sample timesteps.  Pair (image b, k-th timestep) draws the forward noise of (seed, sample_offset + b, draw k) whatever
        shares its pass, so with ``batch_invariant=True`` an entry does not depend on ``max_batch`` or on the other images, bit for
        bit.  ``seed=None`` draws one."""
        if not isinstance(clean, torch.Tensor) or clean.dim() != 4:
            raise ValueError("clean must be a [B, C, H, W] tensor")
        steps = tuple(range(self.noise_steps)) if timesteps is None else tuple(_integer(v, "timesteps", self.noise_steps) for v in timesteps)
        max_batch = check_member(max_batch, "max_batch", low=1)
        seed, sample_offset = check_seed(self._draw_seed() if seed is None else seed, sample_offset)
        clamp, weight = self._objective(edge_weight)
        B, T = clean.shape[0], len(steps)
        pairs = [(b, k) for k in range(T) for b in range(B)]
        out = torch.empty((T * B, 3), dtype=torch.float64, device=clean.device)
        if self.model.training:
            self.model.eval()
        for lo in range(0, len(pairs), max_batch):
            part = pairs[lo:lo + max_batch]
            rows = torch.as_tensor([b for b, _ in part], device=clean.device)
            res, _ = self.model.run_denoising_loss(clean[rows], noisy[rows], [steps[k] for _, k in part], self._alpha_hat_host(), clamp, weight,
                                                   seed=seed, sample_index=[sample_offset + b for b, _ in part], draws=[k for _, k in part],
                                                   workspace_batch=min(max_batch, len(pairs)))
            out[lo:lo + len(part)] = res
        out = out.reshape(T, B, 3).cpu()
        return LossProfile(steps, out[..., 2], out[..., 0], out[..., 1])

    def _draw_seed(self) -> int:
        hi, lo = torch.randint(0, 1 << 32, (2,), dtype=torch.int64).tolist()
        return (hi << 32) | lo

    @torch.no_grad()
    def denoise_ragged(self, noisy_img: torch.Tensor, inference_steps: Sequence[int], seed: Optional[int] = None,
                       sample_offset: int = 0, *, update: str = "reference", rule: Optional[SamplerRule] = None) -> torch.Tensor:
        """Every image of the batch with its OWN step count, in one native call (mi_denoise_slots; not a reference call):
        image b is ``denoise(noisy_img[b:b+1], inference_steps[b], seed=seed, sample_offset=sample_offset + b)`` -- bit for bit
        with ``batch_invariant=True``, within the parity gate otherwise.  The loop runs max(iterations) rows; an image whose
        list has ended idles (its pixels are not touched again).  cddpm: always seeded; ``seed=None`` draws one as
        ``denoise_ensemble`` does (the run then cannot be repeated: pass a seed to keep it).  DDIM ignores ``seed``.

        ``rule=SamplerRule(...)`` (mi_denoise_slots_rule): every image runs that update over its own list -- image b is
        ``denoise(noisy_img[b:b+1], inference_steps[b], update=..., eta=..., clip_x0=..., seed=seed, sample_offset=sample_offset + b)``.
        The rule decides whether anything is drawn, for both variants: seeded as above with ``eta > 0``, ``seed`` ignored at
        ``eta == 0`` and under "dpmpp2m".  ``update=`` stays the refusal it was and names this spelling."""
        refuse_update(update, "denoise_ragged (mi_denoise_slots)")
        rule = check_rule(rule)
        counts = list(inference_steps)
        if not isinstance(noisy_img, torch.Tensor) or noisy_img.dim() != 4 or len(counts) != noisy_img.shape[0]:
            raise ValueError(f"inference_steps must hold one step count per image ({len(counts)} for a batch of "
                             f"{noisy_img.shape[0] if isinstance(noisy_img, torch.Tensor) and noisy_img.dim() else '?'})")
        stochastic = getattr(self.model, "variant", "ddim") == "cddpm"
        if stochastic if rule is None else rule.draws:
            seed, sample_offset = check_seed(self._draw_seed() if seed is None else seed, sample_offset)
        else:
            seed = None
            _, sample_offset = check_seed(0, sample_offset)
        self.model.eval()
        lists = [timestep_list(self.noise_steps, _integer(k, "inference_steps", 1 << 31)) for k in counts]
        n_rows = max((len(t) for t in lists), default=0)
        rows = [[t[i] if i < len(t) else -1 for t in lists] for i in range(n_rows)]
        cond = noisy_img.contiguous()
        x = cond.clone()
        index = [sample_offset + b for b in range(len(counts))]
        if rule is not None:      # (the whole lists are in the call: no neighbour lies outside it)
            x0 = torch.empty_like(x) if rule.update == "dpmpp2m" else None
            return self.model.run_slots_rule(cond, x, rows, self.beta, self.alpha, self.alpha_hat, clamp_eps=not stochastic,
                                             sample_index=index, seed=seed, rule=rule, x0=x0)
        return self.model.run_slots(cond, x, rows, self.beta, self.alpha, self.alpha_hat, clamp_eps=not stochastic,
                                    sample_index=index, seed=seed)

    # north_star's wording for the same call
    ddim_sample = denoise
