"""The ensemble operators: the seeded step noise as a tensor, mean / std, quantile maps, proper scores and principal modes over the
members of an ensemble (include/midd.h: mi_step_noise_fill_member, mi_ensemble_reduce, mi_ensemble_quantiles, THE ENSEMBLE SCORES,
THE ENSEMBLE MODES), and what ``DiffusionDenoiser.denoise_ensemble`` returns."""
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


MAX_MODES, MAX_MODE_MEMBERS = 8, 64


class EnsembleModes(NamedTuple):
    """What ``ensemble_modes`` returns (include/midd.h: THE ENSEMBLE MODES).  Only ``modes`` lives on the device; the rest are float64
    (``valid``: int64) CPU tensors.  Modes of (nearly) equal ``variance`` are not unique: any rotation within their span is as good."""
    modes: torch.Tensor                   # float32 [B, M, C, H, W] on the device: mode j in image units; mean +- modes[:, j] is one std along it
    variance: torch.Tensor                # [B, M]: the variance along mode j, mu_j / (K - 1), descending
    explained: torch.Tensor               # [B, M]: its share of the total, mu_j / sum(mu)
    coefficients: torch.Tensor            # [B, K, M]: member k's position along mode j in standard deviations, v_j[k] * sqrt(K - 1)
    gram: torch.Tensor                    # [B, K, K]: the raw Gram matrix of the centred members
    total_variance: torch.Tensor          # [B]: sum(mu) / (K - 1), the unbiased member variance summed over the valid elements
    valid: torch.Tensor                   # int64 [B]: the elements whose members are all finite; the others are NaN in every mode


def check_modes(modes, members: int) -> int:
    """The ``modes`` argument of ``ensemble_modes`` beside the member count: an int in [1, min(8, members - 1)], members in [2, 64]."""
    if isinstance(members, bool) or not isinstance(members, int) or not 2 <= members <= MAX_MODE_MEMBERS:
        raise ValueError(f"ensemble_modes needs 2 <= members <= {MAX_MODE_MEMBERS} (got {members}): one member has no spread, and the Gram "
                         "kernel tiles at most 64 members")
    if isinstance(modes, bool) or not isinstance(modes, int) or not 1 <= modes <= min(MAX_MODES, members - 1):
        raise ValueError(f"modes must be an int in [1, min({MAX_MODES}, members - 1)] = [1, {min(MAX_MODES, members - 1)}] (got {modes!r}): "
                         f"{members} centred members span at most {members - 1} modes")
    return modes


def gram_eigen(gram, modes: int, eigh=None):
    """The host step of ``ensemble_modes`` in float64 numpy: ``gram`` [B, K, K] -> (mu [B, K], v [B, K, K], weights [B, modes, K]).
    ``numpy.linalg.eigh``; eigenvalues clipped at 0 and sorted descending; each eigenvector (column ``v[b, :, j]``) signed so that
    its component of largest magnitude -- the first of them on ties -- is positive; weights[b, j, k] = v[b, k, j] / sqrt(K - 1)."""
    import numpy as np
    g = np.asarray(gram, dtype=np.float64)
    K = g.shape[-1]
    mu, v = (eigh or np.linalg.eigh)(g)
    mu = np.clip(mu, 0.0, None)[:, ::-1]
    v = v[:, :, ::-1]
    lead = np.argmax(np.abs(v), axis=1)                                     # [B, K]: the first component of largest magnitude
    sign = np.where(np.take_along_axis(v, lead[:, None, :], axis=1) < 0.0, -1.0, 1.0)
    v = np.ascontiguousarray(v * sign)
    weights = np.ascontiguousarray(np.swapaxes(v[:, :, :modes], 1, 2) / np.sqrt(np.float64(K - 1)))
    return np.ascontiguousarray(mu), v, weights


@torch.no_grad()
def ensemble_modes(samples: torch.Tensor, modes: int = 3) -> EnsembleModes:
    """The principal modes of an ensemble's spread: what varies together (mi_ensemble_gram, mi_ensemble_project; include/midd.h:
    THE ENSEMBLE MODES).  ``samples`` is [B, K, C, H, W] or [K, C, H, W] (then every output lacks the batch axis), float32 on the GPU,
    2 <= K <= 64; ``modes`` <= min(8, K - 1).  The K x K Gram matrix of the centred members is reduced on the device, its
    eigenproblem solved on the host in float64 (``gram_eigen``), and the centred members are projected onto the scaled leading
    eigenvectors in one launch: ``modes[:, j]`` is the j-th coherent pattern in grey-level units, so that mean +- mode is a
    one-standard-deviation excursion along it, and with all K - 1 modes the squares add up to the per-pixel variance.  Channels
    are pooled.  An element with a member that is not finite is left out, counted (``valid``) and NaN in every mode.  Modes that
    belong to (nearly) equal eigenvalues are not unique: only their span is.  The Gram matrix is copied to the host (that waits
    for the stream); the members never are."""
    import numpy as np
    if not isinstance(samples, torch.Tensor) or samples.dim() not in (4, 5) or min(samples.shape) < 1:
        raise ValueError("samples must be a [B, members, C, H, W] or [members, C, H, W] tensor without an empty axis")
    batched = samples.dim() == 5
    src = samples if batched else samples.unsqueeze(0)
    B, K = int(src.shape[0]), int(src.shape[1])
    M = check_modes(modes, K)
    if src.device.type != "cuda":
        raise RuntimeError(f"ensemble_modes runs only on a ROCm GPU (got {src.device}): there is no CPU fallback")
    if src.dtype != torch.float32:
        raise TypeError(f"samples must be float32 (got {src.dtype})")
    src = src.contiguous()
    chw = src[0, 0].numel()
    lib = native.lib()
    dev = src.device
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        raw = torch.empty(B * (K * K + 1), dtype=torch.int64, device=dev)       # [gram B*K*K | invalid B]: one copy to the host
        nbytes = lib.mi_ensemble_gram_workspace_bytes(B, K, chw)
        if nbytes == 0:
            native.check(-1)
        ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
        native.check(lib.mi_ensemble_gram(src.data_ptr(), B, K, chw, raw.data_ptr(), raw.data_ptr() + 8 * B * K * K, ws.data_ptr(), nbytes, stream))
        host = raw.cpu()
        gram = host[:B * K * K].view(torch.float64).reshape(B, K, K).clone()
        valid = chw - host[B * K * K:]
        mu, v, weights = gram_eigen(gram.numpy(), M)
        w_dev = torch.from_numpy(weights).to(dev)
        out = torch.empty((B, M) + tuple(src.shape[2:]), dtype=torch.float32, device=dev)
        native.check(lib.mi_ensemble_project(src.data_ptr(), B, K, chw, w_dev.data_ptr(), M, out.data_ptr(), stream))
    total = mu.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        explained = mu[:, :M] / total[:, None]
    fields = (out, torch.from_numpy(mu[:, :M] / (K - 1)), torch.from_numpy(explained),
              torch.from_numpy(np.ascontiguousarray(v[:, :, :M] * np.sqrt(np.float64(K - 1)))), gram, torch.from_numpy(total / (K - 1)), valid.clone())
    return EnsembleModes(*(fields if batched else (t[0] for t in fields)))
