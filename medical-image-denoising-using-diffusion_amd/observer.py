"""Task-based assessment with a model observer: is a faint signal easier or harder to see after the run?

A known low-contrast signal is inserted into a known background, many noisy realisations with and without it go through the
sampler, and a channelized Hotelling observer (CHO) is asked how well it separates the two classes: a detectability index d' and an
AUC, for the outputs and -- the same observer -- for the noisy inputs.  The hot path is ``channel_responses`` (mi_channel_responses;
include/midd.h: THE CHANNEL RESPONSES): the responses of [N, H, W] planes at L locations to C channel templates, on the device in
one fixed order.  Everything after it (``hotelling``) is float64 numpy on [rows, C] arrays.  ``detectability_study`` is the chain
behind ``DiffusionDenoiser.detectability``.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import native
from .rules import _integer, check_member

MIN_ROI, MAX_ROI, MAX_CHANNELS, MAX_LOCATIONS = 4, 128, 32, 4096      # include/midd.h: mi_channel_responses


class ChannelResponses(NamedTuple):
    """What ``channel_responses`` returns, both on the device of the planes."""
    values: torch.Tensor                  # float64 [..., L, C]; the canonical quiet NaN in every channel of an invalid ROI
    invalid: torch.Tensor                 # bool [..., L]: the ROI holds a pixel that is not finite


class Detectability(NamedTuple):
    """What ``hotelling`` returns: float64 numpy, scalars as Python numbers."""
    dprime: float                         # (mean t1 - mean t0) / sqrt((var t1 + var t0) / 2) of the scored rows
    auc: float                            # Mann-Whitney statistic of the scored rows, ties counted 1/2
    template: np.ndarray                  # [C]: w = S^-1 delta
    mean_difference: np.ndarray           # [C]: delta = mean(v1) - mean(v0) of the training rows
    covariance: np.ndarray                # [C, C]: S = (cov(v0) + cov(v1)) / 2 of the training rows, unbiased
    t_absent: np.ndarray                  # [n_test of class 0]: the scores v w of the scored rows
    t_present: np.ndarray                 # [n_test of class 1]
    n_train: Tuple[int, int]              # training rows per class
    n_test: Tuple[int, int]               # scored rows per class (resubstitution: the training rows again)
    dropped: Tuple[int, int]              # rows with a NaN per class, left out before anything else


class DetectabilityStudy(NamedTuple):
    """What ``DiffusionDenoiser.detectability`` returns."""
    denoised: Detectability               # the observer on the sampler's outputs
    noisy: Detectability                  # the same observer on the sampler's inputs
    responses_denoised: ChannelResponses  # [2 trials, L, C]: trials 0 .. trials - 1 are signal-absent, the rest signal-present
    responses_noisy: ChannelResponses
    centres: np.ndarray                   # int32 [L, 2] as (cy, cx)
    channels: np.ndarray                  # float64 [C, roi, roi]
    seed: int                             # the seed of the measurement noise (and of the cddpm step noise): given or drawn
    images: Optional[Tuple[torch.Tensor, torch.Tensor]]      # (noisy, denoised) [2 trials, 1, H, W] with return_images, else None


def _in_range(v, what: str, lo: int, hi: int) -> int:
    i = _integer(v, what, 1 << 31, -(1 << 31))
    if not lo <= i <= hi:
        raise ValueError(f"{what} must be in [{lo}, {hi}] (got {v!r})")
    return i


# ---------------------------------------------------------------------------------------------- channels and locations
def laguerre_gauss_channels(roi: int, n: int = 6, width: Optional[float] = None) -> np.ndarray:
    """The first ``n`` Laguerre-Gauss channels on a ``roi`` x ``roi`` grid -> float64 [n, roi, roi]:

        u_j(r) = (sqrt(2) / a) * exp(-pi r^2 / a^2) * L_j(2 pi r^2 / a^2),      j = 0 .. n - 1

    r measured from ROI index (roi // 2, roi // 2) -- the pixel ``channel_responses`` puts on the centre --, L_j the Laguerre
    polynomial by its three-term recurrence (k + 1) L_{k+1} = (2 k + 1 - x) L_k - k L_{k-1} in float64, a = ``width`` (default
    roi / 4).  The u_j are orthonormal over the plane, so on a grid that holds them their Gram matrix is close to the identity.
    ``a = sigma * sqrt(2 pi)`` matches a Gaussian signal of standard deviation sigma: channel 0 is then the signal's shape,
    exp(-r^2 / (2 sigma^2)), up to scale.  Rotationally symmetric channels suit rotationally symmetric signals at a known location;
    any other float64 [C, R, R] array is accepted as channels by every call of this module."""
    roi = _in_range(roi, "roi", MIN_ROI, MAX_ROI)
    n = _in_range(n, "n", 1, MAX_CHANNELS)
    a = roi / 4.0 if width is None else float(width)
    if not (a > 0.0 and a < float("inf")):
        raise ValueError(f"width must be a positive finite number (got {width!r})")
    d = np.arange(roi, dtype=np.float64) - float(roi // 2)
    r2 = d[:, None] ** 2 + d[None, :] ** 2
    x = 2.0 * np.pi * r2 / (a * a)
    gauss = (np.sqrt(2.0) / a) * np.exp(-np.pi * r2 / (a * a))
    out = np.empty((n, roi, roi), np.float64)
    prev, cur = np.zeros_like(x), np.ones_like(x)
    for k in range(n):
        out[k] = gauss * cur
        prev, cur = cur, ((2 * k + 1 - x) * cur - k * prev) / (k + 1)
    return out


def roi_grid(H: int, W: int, roi: int) -> np.ndarray:
    """The centres of the non-overlapping ``roi`` x ``roi`` ROIs of an H x W image -> int32 [L, 2] as (cy, cx), row by row: centres
    at roi // 2 + i * roi for as long as the ROI fits, so L = (H // roi) * (W // roi)."""
    roi = _in_range(roi, "roi", MIN_ROI, MAX_ROI)
    H, W = _integer(H, "H", 1 << 31, 1), _integer(W, "W", 1 << 31, 1)
    if H < roi or W < roi:
        raise ValueError(f"the image ({H} x {W}) is smaller than the ROI ({roi} x {roi}): there are no partial ROIs")
    ys = roi // 2 + roi * np.arange(H // roi)
    xs = roi // 2 + roi * np.arange(W // roi)
    return np.ascontiguousarray(np.stack(np.meshgrid(ys, xs, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int32))


def check_centres(centres, H: int, W: int, h: int, w: int, what: str) -> np.ndarray:
    """``centres`` as int32 [L, 2]; every h x w window centred (index (h // 2, w // 2)) on one must lie inside the H x W image."""
    try:
        c = np.asarray(centres)
        if c.dtype.kind not in "iu" or c.ndim != 2 or c.shape[1] != 2 or c.shape[0] < 1:
            raise TypeError
    except TypeError:
        raise ValueError("centres must be an integer array [L, 2] of (cy, cx) with at least one row") from None
    c = c.astype(np.int64)
    y0, x0 = c[:, 0] - h // 2, c[:, 1] - w // 2
    bad = np.nonzero((y0 < 0) | (x0 < 0) | (y0 + h > H) | (x0 + w > W))[0]
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"centre {i} = ({int(c[i, 0])}, {int(c[i, 1])}): its {what} of {h} x {w} leaves the {H} x {W} image "
                         f"(refused, not clipped)")
    return np.ascontiguousarray(c.astype(np.int32))


def check_channels(channels) -> np.ndarray:
    """``channels`` as a contiguous float64 [C, R, R] numpy array, 1 <= C <= 32, 4 <= R <= 128."""
    if isinstance(channels, torch.Tensor):
        channels = channels.detach().cpu().numpy()
    u = np.asarray(channels)
    if u.dtype != np.float64 or u.ndim != 3 or u.shape[1] != u.shape[2]:
        raise ValueError(f"channels must be a float64 [C, R, R] array (got {u.dtype} {tuple(u.shape)})")
    if not 1 <= u.shape[0] <= MAX_CHANNELS or not MIN_ROI <= u.shape[1] <= MAX_ROI:
        raise ValueError(f"channels [C, R, R] needs 1 <= C <= {MAX_CHANNELS} and {MIN_ROI} <= R <= {MAX_ROI} (got C = {u.shape[0]}, R = {u.shape[1]})")
    return np.ascontiguousarray(u)


# ---------------------------------------------------------------------------------------------- the signal
@torch.no_grad()
def insert_signal(images: torch.Tensor, signal, centres, amplitude: float = 1.0) -> torch.Tensor:
    """``images`` [..., H, W] float32 with ``float32(amplitude) * signal`` added on every centre -> a new tensor.  ``signal`` is
    [h, w], its index (h // 2, w // 2) lands on the centre.  float32 throughout: one multiplication per signal element, then one
    addition per centre and element, the centres in order, so where two copies overlap they add up in that order.  Nothing is
    clamped.  A copy that leaves the image is refused.  Plain torch operations on the images' device: it runs once per study on
    L h w elements."""
    if not isinstance(images, torch.Tensor) or images.dim() < 2 or images.dtype != torch.float32:
        raise ValueError("images must be a float32 tensor [..., H, W]")
    s = torch.as_tensor(signal)
    if s.dim() != 2 or min(s.shape) < 1 or not s.dtype.is_floating_point:
        raise ValueError("signal must be a floating-point [h, w] array")
    h, w = int(s.shape[0]), int(s.shape[1])
    c = check_centres(centres, int(images.shape[-2]), int(images.shape[-1]), h, w, "signal")
    term = torch.tensor(np.float32(amplitude), dtype=torch.float32, device=images.device) * s.to(images.device, torch.float32)
    out = images.clone()
    for cy, cx in c.tolist():
        y0, x0 = cy - h // 2, cx - w // 2
        out[..., y0:y0 + h, x0:x0 + w] += term
    return out


# ---------------------------------------------------------------------------------------------- the device call
@torch.no_grad()
def channel_responses(x: torch.Tensor, centres, channels) -> ChannelResponses:
    """The responses of the planes ``x`` [..., H, W] (float32, on the GPU; the leading axes are flattened to N planes) at the L
    ``centres`` (integer [L, 2] as (cy, cx), a host array) to the C ``channels`` (float64 [C, R, R]) -> ``ChannelResponses(values
    [..., L, C] float64, invalid [..., L] bool)`` on the same device (mi_channel_responses; include/midd.h: THE CHANNEL RESPONSES).
    The ROI of a centre is rows cy - R // 2 .. cy - R // 2 + R - 1 and likewise columns; one that leaves the image is refused, not
    clipped.  ``values[..., l, c]`` is the dot product of ROI l with channel c in double precision and one fixed summation order,
    whatever the alignment of ``x``.  An ROI with a pixel that is not finite is flagged and NaN in every channel.  Nothing is copied
    to the host."""
    if not isinstance(x, torch.Tensor) or x.dim() < 2 or min(x.shape) < 1:
        raise ValueError("x must be a tensor [..., H, W] without an empty axis")
    u = check_channels(channels)
    Cn, R = int(u.shape[0]), int(u.shape[1])
    H, W = int(x.shape[-2]), int(x.shape[-1])
    c = check_centres(centres, H, W, R, R, "ROI")
    L = int(c.shape[0])
    if L > MAX_LOCATIONS:
        raise ValueError(f"centres holds {L} locations (limit: 1 <= L <= {MAX_LOCATIONS} a call)")
    if x.device.type != "cuda":
        raise RuntimeError(f"channel_responses runs only on a ROCm GPU (got {x.device}): there is no CPU fallback")
    if x.dtype != torch.float32:
        raise TypeError(f"x must be float32 (got {x.dtype})")
    lead = tuple(x.shape[:-2])
    src = x.contiguous()
    N = src.numel() // (H * W)
    dev = src.device
    with torch.cuda.device(dev):
        ud = torch.from_numpy(u).to(dev)
        values = torch.empty(lead + (L, Cn), dtype=torch.float64, device=dev)
        flags = torch.empty(lead + (L,), dtype=torch.int32, device=dev)
        native.check(native.lib().mi_channel_responses(src.data_ptr(), N, H, W, c.ctypes.data_as(C.POINTER(C.c_int32)), L, R, ud.data_ptr(), Cn,
                                                       values.data_ptr(), flags.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
    return ChannelResponses(values, flags != 0)


# ---------------------------------------------------------------------------------------------- the host statistics
def mann_whitney_auc(t_absent, t_present) -> float:
    """P(t1 > t0) + P(t1 == t0) / 2 over all pairs: the area under the empirical ROC curve, ties counted 1/2."""
    t0 = np.sort(np.asarray(t_absent, np.float64))
    t1 = np.asarray(t_present, np.float64)
    below = np.searchsorted(t0, t1, side="left").astype(np.float64)
    upto = np.searchsorted(t0, t1, side="right").astype(np.float64)
    return float((below + 0.5 * (upto - below)).sum() / (t0.size * t1.size))


def hotelling(v_absent, v_present, train: Optional[int] = None) -> Detectability:
    """The Hotelling observer on channel responses ``v_absent`` [n0, C] and ``v_present`` [n1, C], float64 numpy on the host.

    Rows with a NaN (the responses of an invalid ROI) are dropped first and counted (``dropped``).  From the training rows
    delta = mean(v1) - mean(v0), S = (cov(v0) + cov(v1)) / 2 with unbiased covariances and w = numpy.linalg.solve(S, delta); the
    scored rows give t = v w, ``dprime`` = (mean t1 - mean t0) / sqrt((var t1 + var t0) / 2) with unbiased variances, and ``auc``,
    the Mann-Whitney statistic with ties counted 1/2.

    ``train=None`` is RESUBSTITUTION: template and scores come from the same rows, so dprime equals sqrt(delta^T S^-1 delta) and is
    biased UPWARDS -- the template has seen the noise it is scored on; the bias grows with C / rows.  ``train=k`` is a hold-out: the
    first k rows of each class (in index order, after the NaN rows are gone) estimate delta, S and w, and the remaining rows are
    scored; that estimate is biased downwards, and the truth lies between the two.

    Refused by name: fewer than 2 training rows in a class; n0_train + n1_train - 2 < C (S would be singular); an empty test set;
    an S that is not finite."""
    v0, v1 = np.asarray(v_absent, np.float64), np.asarray(v_present, np.float64)
    if v0.ndim != 2 or v1.ndim != 2 or v0.shape[1] != v1.shape[1] or v0.shape[1] < 1:
        raise ValueError(f"v_absent and v_present must be [rows, C] arrays with the same C >= 1 (got {v0.shape} and {v1.shape})")
    Cn = v0.shape[1]
    keep0, keep1 = ~np.isnan(v0).any(axis=1), ~np.isnan(v1).any(axis=1)
    dropped = (int((~keep0).sum()), int((~keep1).sum()))
    v0, v1 = v0[keep0], v1[keep1]
    if train is None:
        a0, a1, s0, s1 = v0, v1, v0, v1
    else:
        k = _integer(train, "train", 1 << 31, 0)
        a0, a1, s0, s1 = v0[:k], v1[:k], v0[k:], v1[k:]
    n_train = (a0.shape[0], a1.shape[0])
    if min(n_train) < 2:
        raise ValueError(f"hotelling: fewer than 2 training rows in a class (absent {n_train[0]}, present {n_train[1]}): a covariance needs two")
    if n_train[0] + n_train[1] - 2 < Cn:
        raise ValueError(f"hotelling: n0_train + n1_train - 2 = {n_train[0] + n_train[1] - 2} < C = {Cn}: the pooled covariance S would be singular")
    n_test = (s0.shape[0], s1.shape[0])
    if min(n_test) < 1:
        raise ValueError(f"hotelling: an empty test set (absent {n_test[0]}, present {n_test[1]} rows after train={train})")
    delta = a1.mean(axis=0) - a0.mean(axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        S = 0.5 * (np.cov(a0, rowvar=False, ddof=1).reshape(Cn, Cn) + np.cov(a1, rowvar=False, ddof=1).reshape(Cn, Cn))
    if not np.isfinite(S).all():
        raise ValueError("hotelling: the pooled covariance S is not finite (a response is infinite or overflows)")
    w = np.linalg.solve(S, delta)
    t0, t1 = s0 @ w, s1 @ w
    with np.errstate(invalid="ignore", divide="ignore"):
        var0 = t0.var(ddof=1) if t0.size > 1 else np.float64("nan")
        var1 = t1.var(ddof=1) if t1.size > 1 else np.float64("nan")
        dprime = (t1.mean() - t0.mean()) / np.sqrt(0.5 * (var1 + var0))
    return Detectability(float(dprime), mann_whitney_auc(t0, t1), w, delta, S, t0, t1, n_train, n_test, dropped)


# ---------------------------------------------------------------------------------------------- the study
def default_roi(h: int, w: int) -> int:
    """The study's ROI side for an h x w signal: its larger side rounded up to a multiple of 8, at least 16."""
    return max(16, -(-max(h, w) // 8) * 8)


@torch.no_grad()
def study_inputs(denoiser, clean: torch.Tensor, first_index: int, sigma: float, seed: int) -> torch.Tensor:
    """The noisy images of trials first_index .. first_index + B - 1 from their clean images [B, 1, H, W]:
    clamp(clean + float32(sigma) * eps, 0, 1), eps the forward noise of (seed, sample index = the trial, draw 0) as
    ``noise_images`` returns it (include/midd.h: THE FORWARD NOISE: counter words that no sampler step draws, so the measurement
    noise is independent of the cddpm step noise of the same seed).  float32: one multiplication, one addition, the clamp."""
    _, eps = denoiser.noise_images(clean, [0] * int(clean.shape[0]), seed=seed, sample_offset=first_index, draw=0)
    return (clean + torch.tensor(np.float32(sigma), dtype=torch.float32, device=clean.device) * eps).clamp(0.0, 1.0)


@torch.no_grad()
def detectability_study(denoiser, background: torch.Tensor, signal, inference_steps: int = 25, trials: int = 64, centres=None,
                        amplitude: float = 1.0, sigma: float = 0.05, seed: Optional[int] = None, channels=None, n_channels: int = 6,
                        width: Optional[float] = None, roi: Optional[int] = None, train: Optional[int] = None, max_batch: int = 16,
                        degrade: Optional[Callable] = None, return_images: bool = False) -> DetectabilityStudy:
    """The chain behind ``DiffusionDenoiser.detectability`` (documented there)."""
    if not isinstance(background, torch.Tensor) or background.dtype != torch.float32 or \
            not (background.dim() == 2 or (background.dim() == 4 and tuple(background.shape[:2]) == (1, 1))):
        raise ValueError("detectability: background must be a float32 [H, W] or [1, 1, H, W] tensor (one single-channel image)")
    if int(getattr(getattr(denoiser.model, "cfg", None), "in_channels", 1)) != 1:
        raise ValueError("detectability: single-channel models only (the signal, the channels and the ROIs are planes)")
    trials = check_member(trials, "trials", low=1)
    max_batch = check_member(max_batch, "max_batch", low=1)
    sig = torch.as_tensor(signal)
    if sig.dim() != 2 or min(sig.shape) < 1:
        raise ValueError("signal must be a floating-point [h, w] array")
    H, W = int(background.shape[-2]), int(background.shape[-1])
    if channels is None:
        roi = default_roi(int(sig.shape[0]), int(sig.shape[1])) if roi is None else roi
        channels = laguerre_gauss_channels(roi, n_channels, width)
    u = check_channels(channels)
    if roi is not None and int(roi) != u.shape[1]:
        raise ValueError(f"roi {roi} and channels of side {u.shape[1]} disagree")
    R = int(u.shape[1])
    c = check_centres(roi_grid(H, W, R) if centres is None else centres, H, W, R, R, "ROI")
    if degrade is None and not (float(sigma) >= 0.0 and float(sigma) < float("inf")):
        raise ValueError(f"sigma must be a finite number >= 0 (got {sigma!r})")
    seed = denoiser._draw_seed() if seed is None else seed
    seed = _integer(seed, "seed", 1 << 64)
    _integer(2 * trials, "2 * trials", 1 << 63)
    bg0 = background.reshape(1, 1, H, W).contiguous()
    bg1 = insert_signal(bg0, sig, c, amplitude)
    if bg0.device.type != "cuda":
        raise RuntimeError(f"detectability runs only on a ROCm GPU (got {bg0.device}): there is no CPU fallback")
    stochastic = denoiser._stochastic
    total = 2 * trials
    noisy = torch.empty((total, 1, H, W), dtype=torch.float32, device=bg0.device)
    out = torch.empty_like(noisy)
    for lo in range(0, total, max_batch):
        hi = min(total, lo + max_batch)
        clean = torch.cat([bg0 if j < trials else bg1 for j in range(lo, hi)], dim=0)
        batch = study_inputs(denoiser, clean, lo, sigma, seed) if degrade is None else degrade(clean, lo)
        if not isinstance(batch, torch.Tensor) or batch.shape != clean.shape or batch.dtype != torch.float32 or batch.device != clean.device:
            raise ValueError("degrade(clean_batch, first_index) must return a float32 tensor of the batch's shape on its device")
        noisy[lo:hi] = batch
        out[lo:hi] = denoiser.denoise(batch, inference_steps, seed=seed, sample_offset=lo) if stochastic else denoiser.denoise(batch, inference_steps)
    resp_out = channel_responses(out[:, 0], c, u)
    resp_in = channel_responses(noisy[:, 0], c, u)
    stats = []
    for resp in (resp_out, resp_in):
        v = resp.values.cpu().numpy()
        stats.append(hotelling(v[:trials].reshape(-1, u.shape[0]), v[trials:].reshape(-1, u.shape[0]), train))
    return DetectabilityStudy(stats[0], stats[1], resp_out, resp_in, c, u, seed, (noisy, out) if return_images else None)
