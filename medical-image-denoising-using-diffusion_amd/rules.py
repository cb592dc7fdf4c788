"""The argument rules of the Python calls -- what an entry judges before any GPU work -- and the host-only coefficient oracles of
the update rules (include/midd.h: THE DDIM UPDATE, THE DPMPP2M UPDATE).  Nothing here touches a device; ``modules.py`` and the
operator modules (``ensemble``, ``nps``, ``loss``, ``tiles``, ``views``) stand on it."""
from __future__ import annotations

import ctypes as C
import dataclasses
import numbers
import operator
from typing import Optional, Sequence, Tuple

import torch

from . import native


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


def check_score_levels(quantiles) -> Tuple[float, ...]:
    """``check_levels``, except that no level at all (None or an empty sequence) is allowed: the scores then carry no coverage."""
    if quantiles is None or (isinstance(quantiles, (tuple, list)) and len(quantiles) == 0):
        return ()
    return check_levels(quantiles)


NPS_ROIS = (32, 64, 128)
NPS_DETREND = {"none": 0, "mean": 1, "plane": 2}


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


def _pair(v, what: str, low: int) -> Tuple[int, int]:
    a, b = (v if isinstance(v, (tuple, list)) and len(v) == 2 else (v, v))
    return _integer(a, what, 1 << 31, low), _integer(b, what, 1 << 31, low)
