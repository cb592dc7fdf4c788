"""``DiffusionDenoiser``: schedule + reverse loop, same surface as the reference class
(/root/reference/Backend/DDIM/DDIMModel.py:250-289; stochastic cddpm variant
/root/reference/Backend/cddpm/cddpmModels.py:263-308).

The schedule tables are built with the same torch calls as the reference so they are bit
identical; the loop itself (UNet forward + fused x_{t-1} update per timestep) is a single
call into libmidd.so.

The argument rules and the stand-alone operators live in ``rules``, ``ensemble``, ``nps``, ``loss``, ``tiles`` and ``views``; every
name this module has exported is still importable from it.
"""
from __future__ import annotations

import ctypes as C, dataclasses, math, numbers, operator      # noqa: E401,F401  (names this module has always carried)
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import native
from .config import timestep_list
from .ensemble import (DEFAULT_SCORE_LEVELS, EnsembleModes, EnsembleQuantileResult, EnsembleResult, EnsembleScores, check_modes,  # noqa: F401
                       ensemble_modes, ensemble_quantiles, ensemble_reduce, ensemble_scores, gram_eigen, step_noise)
from .loss import (DenoisingLoss, LossMaps, LossProfile, _loss_tensor, check_loss_source, loss_counter_args, loss_table_args,  # noqa: F401
                   loss_terms, noise_images)
from .nps import NoisePowerSpectrum, noise_power_spectrum, nps_window  # noqa: F401
from .observer import (ChannelResponses, Detectability, DetectabilityStudy, channel_responses, detectability_study, hotelling,  # noqa: F401
                       insert_signal, laguerre_gauss_channels, roi_grid)
from .spectral import CrossSpectrum, cross_spectrum  # noqa: F401
from .rules import (MAX_QUANTILE_LEVELS, MAX_QUANTILE_MEMBERS, NPS_DETREND, NPS_ROIS, UPDATE_RULES, SamplerRule, _integer,  # noqa: F401
                    _levels_arg, _pair, check_levels, check_member, check_members, check_nps_args, check_quantile_members, check_rule,
                    check_score_levels, check_seed, check_update, ddim_coefficients, dpm_coefficients, refuse_update)
from .tiles import (TiledEnsembleQuantileResult, TiledEnsembleResult, TiledResult, TilePlan, _axis, _tile_tensor, tile_blend,  # noqa: F401
                    tile_blend_quantiles, tile_blend_reduce, tile_consensus, tile_extract, tile_plan, tiling)
from .views import (MAX_VIEWS, VIEW_SETS, SelfEnsembleQuantileResult, SelfEnsembleResult, TiledSelfEnsembleQuantileResult,  # noqa: F401
                    TiledSelfEnsembleResult, _unview_args, _view_tensor, _views_arg, dihedral_quantiles, dihedral_reduce, dihedral_views,
                    tile_blend_unview_quantiles, tile_blend_unview_reduce, view_codes, view_codes_tiled)

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")    # DDIMModel.py:10


class SamplerTrajectory(NamedTuple):
    """What ``DiffusionDenoiser.denoise(..., update="dpmpp2m", return_x0=True)`` returns."""
    image: torch.Tensor                   # [B, C, H, W]: the call's result, the bits of the call without return_x0
    x0: torch.Tensor                      # [n_iters, B, C, H, W]: the predicted image of every iteration (clipped when clip_x0)


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

    # ------------------------------------------------------------------ what the entries share
    @property
    def _stochastic(self) -> bool:
        return getattr(self.model, "variant", "ddim") == "cddpm"

    def _draws(self, rule, seed=None) -> bool:
        """Does a call under ``rule`` (None: the reference's update) draw noise?  cddpm does under the reference's update, a rule
        with eta > 0 does for both variants.  A ``seed`` given to the DDIM variant under the reference's update is refused."""
        if rule is None and not self._stochastic and seed is not None:
            raise ValueError("seed selects the step noise of the stochastic (cddpm) variant: the DDIM variant takes seed=None")
        return self._stochastic if rule is None else rule.eta > 0.0

    def _seed(self, draws: bool, seed, sample_offset=0) -> Tuple[Optional[int], int]:
        """From which seed?  -> ``check_seed`` of (the caller's seed or a fresh one, sample_offset) where the call draws, else
        (None, sample_offset as given)."""
        if not draws:
            return None, sample_offset
        return check_seed(self._draw_seed() if seed is None else seed, sample_offset)

    @staticmethod
    def _rule_kw(rule, update, eta, clip_x0) -> dict:
        """The rule's keywords for a ``run_*`` call; none for the reference's update, so that call is the call of before."""
        return {} if rule is None else dict(update=update, eta=eta, clip_x0=clip_x0)

    def _steps(self, inference_steps):
        self.model.eval()
        return timestep_list(self.noise_steps, inference_steps)

    def _ensemble_with_samples(self, noisy, tile, overlap, **kw):
        """``denoise_ensemble`` or, with ``tile``, ``denoise_tiled_ensemble``, with the members returned."""
        if tile is None:
            return self.denoise_ensemble(noisy, return_samples=True, **kw)
        return self.denoise_tiled_ensemble(noisy, tile=tile, overlap=overlap, return_samples=True, **kw)

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
            res = self.model.run_sampler(noisy_img, self._steps(inference_steps), self.beta, self.alpha, self.alpha_hat,
                                         clamp_eps=not self._stochastic, update=update, clip_x0=clip_x0, return_x0=return_x0)
            return SamplerTrajectory(*res) if return_x0 else res
        if seed is not None:
            if step_noise is not None:
                raise ValueError("pass either seed (noise drawn on the device) or step_noise (a noise tensor), not both")
            seed, sample_offset = check_seed(seed, sample_offset)
        steps = self._steps(inference_steps)
        stochastic = self._stochastic
        draws = self._draws(rule)                                   # whether the call has a noise term at all
        if draws and step_noise is None and seed is None and member == 0:      # (a member without a seed: run_sampler refuses)
            step_noise = 0.5 * torch.randn((len(steps),) + tuple(noisy_img.shape), device=noisy_img.device)
        if not draws:
            step_noise = seed = None
            member = 0
        seeded = {"member": member} if seed is None else {"seed": seed, "sample_offset": sample_offset, "member": member}
        return self.model.run_sampler(noisy_img, steps, self.beta, self.alpha, self.alpha_hat, clamp_eps=not stochastic,
                                      step_noise=step_noise, **seeded, **self._rule_kw(rule, update, eta, clip_x0))

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
        stochastic = self._stochastic
        if rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"]:
            raise ValueError("denoise_ensemble with update='dpmpp2m': a deterministic sampler has no ensemble")
        if rule is not None and rule.eta == 0.0:
            raise ValueError("denoise_ensemble with update='ddim' needs eta > 0: a deterministic sampler has no ensemble")
        if rule is None and not stochastic:
            raise ValueError("denoise_ensemble needs the stochastic (cddpm) variant: a deterministic sampler has no ensemble")
        seed, _ = self._seed(True, seed)      # (everything else is judged by run_ensemble, before any GPU work)
        if levels is not None:
            check_quantile_members(check_member(members, "members", low=1))
        mean, std, samples = self.model.run_ensemble(noisy_img, self._steps(inference_steps), self.beta, self.alpha, self.alpha_hat,
                                                     clamp_eps=not stochastic, members=members, seed=seed, sample_offset=sample_offset,
                                                     member_offset=member_offset, max_batch=max_batch,
                                                     want_samples=return_samples or levels is not None,
                                                     **self._rule_kw(rule, update, eta, clip_x0))
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
        seed, sample_offset = self._seed(self._draws(rule, seed), seed, sample_offset)
        image, tiles, plan = self.model.run_tiled(noisy_img, self._steps(inference_steps), self.beta, self.alpha, self.alpha_hat,
                                                  clamp_eps=not self._stochastic, tile=tile, overlap=overlap, seed=seed,
                                                  sample_offset=sample_offset, max_batch=max_batch, want_tiles=return_tiles,
                                                  **self._rule_kw(rule, update, eta, clip_x0))
        return TiledResult(image, tiles, plan.origins_y, plan.origins_x, seed)

    @torch.no_grad()
    def denoise_tiled_fused(self, noisy_img: torch.Tensor, inference_steps: int = 25, tile=256, overlap=32, max_batch: int = 16,
                            seed: Optional[int] = None, sample_offset: int = 0, return_tiles: bool = False,
                            *, update: str = "reference", eta: float = 0.0, clip_x0: bool = True) -> TiledResult:
        """``denoise_tiled`` whose overlapping tiles AGREE AFTER EVERY STEP (not a reference call; include/midd.h:
        mi_denoise_tiled_fused).  ``denoise_tiled`` runs the whole sampler loop on every tile alone and cross-fades what the tiles
        ended up with; the network has attention, so two tiles decide differently about the strip they share and the ramp only
        hides it.  Here the steps are the outer loop: after each one a single ``tile_consensus`` launch replaces every tile element
        by the blend of all the elements over its pixel (the usual per-step fusion of tiled diffusion), so every tile enters the
        next forward with the same values wherever it shares pixels with a neighbour, and the result's ``tiles`` are exactly
        ``tile_extract(image)``.  Same tiling, same arguments and the same ``TiledResult`` as ``denoise_tiled``; ``tile == image
        size`` is ``denoise`` bit for bit.  The call equals, bit for bit, the composition of ``run_slots_rule`` rows and
        ``tile_consensus`` at the same ``max_batch``; with ``batch_invariant=True`` it does not depend on ``max_batch`` at all.

        The seed rules are ``denoise_tiled``'s: cddpm and ``update="ddim"`` with ``eta > 0`` are always seeded -- the noise field
        belongs to the image, overlapping tiles draw the same noise, so fusing does not shrink it -- and ``seed=None`` draws a seed
        and returns it; DDIM takes ``seed=None``; ``update="ddim"`` with ``eta=0`` ignores a seed; ``update="dpmpp2m"`` raises
        ValueError on one (its ``x0`` history is every tile's own and is not fused).  There is no ``step_noise`` tensor.  The
        workspace keeps the condition tiles of the whole batch (``UNetDiffusion.tiled_fused_workspace_bytes``)."""
        rule = check_update(update, eta, clip_x0)
        if rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"] and seed is not None:
            raise ValueError("update='dpmpp2m' is deterministic: denoise_tiled_fused takes no seed with it")
        seed, sample_offset = self._seed(self._draws(rule, seed), seed, sample_offset)
        image, tiles, plan = self.model.run_tiled_fused(noisy_img, self._steps(inference_steps), self.beta, self.alpha, self.alpha_hat,
                                                        clamp_eps=not self._stochastic, tile=tile, overlap=overlap, seed=seed,
                                                        sample_offset=sample_offset, max_batch=max_batch, want_tiles=return_tiles,
                                                        **self._rule_kw(rule, update, eta, clip_x0))
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
        if not self._stochastic:
            raise ValueError("denoise_tiled_ensemble needs the stochastic (cddpm) variant: a deterministic sampler has no ensemble")
        seed, _ = self._seed(True, seed)      # (everything else is judged by run_tiled_ensemble, before any GPU work)
        if levels is not None:
            check_quantile_members(check_member(members, "members", low=1))
        mean, std, samples, tiles, plan = self.model.run_tiled_ensemble(
            noisy_img, self._steps(inference_steps), self.beta, self.alpha, self.alpha_hat, clamp_eps=False, tile=tile, overlap=overlap, members=members,
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
        draws = self._draws(None, seed)
        if isinstance(noisy_img, torch.Tensor) and noisy_img.dim() == 4:
            views = view_codes(noisy_img.shape[2], noisy_img.shape[3], views)      # (before any GPU work; run_self_ensemble judges the rest)
        seed, _ = self._seed(draws, seed)
        mean, std, samples, codes, maps = self.model.run_self_ensemble(
            noisy_img, self._steps(inference_steps), self.beta, self.alpha, self.alpha_hat, clamp_eps=not draws, views=views, seed=seed,
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
        draws = self._draws(rule, seed)
        if isinstance(noisy_img, torch.Tensor) and noisy_img.dim() == 4:
            views = view_codes_tiled(noisy_img.shape[2], noisy_img.shape[3], tile, overlap, views)      # (before any GPU work)
        seed, sample_offset = self._seed(draws, seed, sample_offset)
        mean, std, samples, tiles, codes, plan = self.model.run_tiled_self_ensemble(
            noisy_img, self._steps(inference_steps), self.beta, self.alpha, self.alpha_hat, clamp_eps=not self._stochastic, tile=tile,
            overlap=overlap, views=views, seed=seed, sample_offset=sample_offset, member_offset=member_offset, max_batch=max_batch,
            want_samples=return_samples, want_tiles=return_tiles or levels is not None, **self._rule_kw(rule, update, eta, clip_x0))
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
        result = self._ensemble_with_samples(noisy, tile, overlap, inference_steps=inference_steps, members=members, seed=seed,
                                             sample_offset=sample_offset, member_offset=member_offset, max_batch=max_batch)
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
        result = self._ensemble_with_samples(noisy, tile, overlap, inference_steps=inference_steps, members=members, seed=seed,
                                             sample_offset=sample_offset, member_offset=member_offset, max_batch=max_batch)
        return result, noise_power_spectrum(result.samples, result.mean, roi, step, detrend, window, members / (members - 1), exclude_axes)

    @torch.no_grad()
    def ensemble_modes(self, noisy: torch.Tensor, inference_steps: int = 25, members: int = 16, modes: int = 3, seed: Optional[int] = None,
                       sample_offset: int = 0, member_offset: int = 0, max_batch: int = 16, tile=None, overlap=32):
        """An ensemble of ``noisy`` and the principal modes of its spread -> ``(result, modes)``: ``denoise_ensemble(noisy, ...,
        return_samples=True)`` -- or, with ``tile``, ``denoise_tiled_ensemble(noisy, ..., tile=tile, overlap=overlap,
        return_samples=True)`` -- followed by ``ensemble_modes(result.samples, modes)``, bit for bit that composition.  The std map
        says how much each pixel varies between members; ``modes.modes`` says what varies together: mean +- mode j is a
        one-standard-deviation excursion along the j-th coherent pattern.  2 <= members <= 64, modes <= min(8, members - 1)."""
        check_modes(modes, check_member(members, "members", low=1))
        result = self._ensemble_with_samples(noisy, tile, overlap, inference_steps=inference_steps, members=members, seed=seed,
                                             sample_offset=sample_offset, member_offset=member_offset, max_batch=max_batch)
        return result, ensemble_modes(result.samples, modes)

    @torch.no_grad()
    def spectral_fidelity(self, clean: torch.Tensor, noisy: torch.Tensor, inference_steps: int = 25, members: Optional[int] = None,
                          seed: Optional[int] = None, sample_offset: int = 0, member_offset: int = 0, max_batch: int = 16, tile=None,
                          overlap=32, roi: int = 64, step: Optional[int] = None, detrend: str = "plane", window="hann",
                          exclude_axes: bool = False, return_planes: bool = False):
        """A run on ``noisy`` and, against ``clean``, at which spatial frequencies the signal survives it ->
        ``(result, fidelity, baseline)``.  The run: ``denoise(noisy, inference_steps, seed=seed, sample_offset=sample_offset)``, with
        ``tile`` ``denoise_tiled(..., tile=tile, overlap=overlap, max_batch=max_batch)``, with ``members`` ``denoise_ensemble(...,
        return_samples=True)`` or ``denoise_tiled_ensemble(..., return_samples=True)``.  ``fidelity = cross_spectrum(clean, output,
        roi, step, detrend, window, exclude_axes, return_planes)``, output being the image or, with ``members``, the samples
        [B, K, C, H, W] beside the broadcast truth; ``baseline = cross_spectrum(clean, noisy, ...)`` with the same arguments: bit for
        bit those compositions.  ``fidelity.transfer()`` and ``fidelity.frc()`` beside the baseline's give the per-frequency gain of
        the run."""
        check_nps_args(roi, step, detrend)
        nps_window(window, roi)
        if not isinstance(clean, torch.Tensor) or not isinstance(noisy, torch.Tensor) or clean.shape != noisy.shape or clean.device != noisy.device:
            raise ValueError("clean must be a tensor of the noisy images' shape, on their device")
        if clean.dtype != torch.float32:
            raise TypeError(f"clean must be float32 (got {clean.dtype})")
        if members is not None:
            result = self._ensemble_with_samples(noisy, tile, overlap, inference_steps=inference_steps, members=members, seed=seed,
                                                 sample_offset=sample_offset, member_offset=member_offset, max_batch=max_batch)
            output = result.samples
        elif tile is not None:
            result = self.denoise_tiled(noisy, inference_steps, tile=tile, overlap=overlap, max_batch=max_batch, seed=seed, sample_offset=sample_offset)
            output = result.image
        else:
            result = output = self.denoise(noisy, inference_steps, seed=seed, sample_offset=sample_offset)
        spec = dict(roi=roi, step=step, detrend=detrend, window=window, exclude_axes=exclude_axes, return_planes=return_planes)
        return result, cross_spectrum(clean, output, **spec), cross_spectrum(clean, noisy, **spec)

    @torch.no_grad()
    def ensemble_frc(self, noisy: torch.Tensor, inference_steps: int = 25, members: int = 8, seed: Optional[int] = None, sample_offset: int = 0,
                     member_offset: int = 0, max_batch: int = 16, tile=None, overlap=32, roi: int = 64, step: Optional[int] = None,
                     detrend: str = "plane", window="hann", exclude_axes: bool = False, return_planes: bool = False):
        """An ensemble of ``noisy`` and the Fourier ring correlation between its independent draws, which needs no truth ->
        ``(result, spectrum)``: ``denoise_ensemble(noisy, ..., return_samples=True)`` -- or, with ``tile``,
        ``denoise_tiled_ensemble(noisy, ..., tile=tile, overlap=overlap, return_samples=True)`` -- followed by
        ``cross_spectrum(result.samples[:, 0::2], result.samples[:, 1::2], roi, step, detrend, window, exclude_axes, return_planes)``,
        bit for bit that composition: the draws are paired two by two.  ``spectrum.frc()`` says up to which frequency two draws
        agree, ``spectrum.resolution()`` where it falls below 1/7.  cddpm only; ``members`` even and >= 2."""
        if check_member(members, "members", low=1) < 2 or members % 2:
            raise ValueError(f"ensemble_frc needs an even members >= 2 (got {members}): the draws are paired two by two")
        check_nps_args(roi, step, detrend)
        nps_window(window, roi)
        result = self._ensemble_with_samples(noisy, tile, overlap, inference_steps=inference_steps, members=members, seed=seed,
                                             sample_offset=sample_offset, member_offset=member_offset, max_batch=max_batch)
        return result, cross_spectrum(result.samples[:, 0::2], result.samples[:, 1::2], roi, step, detrend, window, exclude_axes, return_planes)

    @torch.no_grad()
    def detectability(self, background: torch.Tensor, signal, inference_steps: int = 25, trials: int = 64, centres=None,
                      amplitude: float = 1.0, sigma: float = 0.05, seed: Optional[int] = None, channels=None, n_channels: int = 6,
                      width: Optional[float] = None, roi: Optional[int] = None, train: Optional[int] = None, max_batch: int = 16,
                      degrade=None, return_images: bool = False) -> DetectabilityStudy:
        """Is a faint signal easier or harder to see after the run?  A signal-known-exactly, location-known detection study with a
        channelized Hotelling observer -> ``DetectabilityStudy(denoised, noisy, responses_denoised, responses_noisy, centres,
        channels, seed, images)``: the observer's d' and AUC on the sampler's outputs beside the same observer on its noisy inputs.
        Not a reference call.

        ``background``: one clean single-channel image, [H, W] or [1, 1, H, W] (anything else, or a model with more than one image
        channel, is refused by name).  ``signal``: [h, w], added with ``insert_signal(background, signal, centres, amplitude)`` on
        every centre.  ``roi`` defaults to the signal's larger side rounded up to a multiple of 8 and to at least 16, ``centres`` to
        ``roi_grid(H, W, roi)``, ``channels`` to ``laguerre_gauss_channels(roi, n_channels, width)``; ``seed=None`` draws a seed as
        ``denoise_ensemble`` does and the result carries it.

        Trial j = 0 .. 2 * trials - 1 is signal-absent for j < trials and signal-present otherwise.  Its noisy image is
        clamp(bg_k + float32(sigma) * eps_j, 0, 1) with bg_0 the background, bg_1 the background with the signal, and eps_j the eps
        that ``noise_images(bg, t, seed=seed, sample_offset=j, draw=0)`` returns: THE FORWARD NOISE words (include/midd.h), which
        no sampler step draws, so the measurement noise is independent of the cddpm step noise of the same seed.
        ``degrade(clean_batch, first_index) -> noisy_batch`` replaces that rule when given.  The trials run in index order, in
        passes of ``max_batch``, through the unchanged ``denoise``: cddpm with ``seed=seed, sample_offset=j`` -- trial j is that
        image's plain seeded run --, DDIM unseeded.  One ``channel_responses`` launch then runs over the 2 * trials outputs and one
        over the noisy inputs, and ``hotelling(absent rows, present rows, train)`` is applied to each with the L locations of an
        image pooled as rows in (trial, location) order.  The call is exactly that chain, bit for bit; with
        ``batch_invariant=True`` it does not depend on ``max_batch``.

        Pooling treats the locations of one image as independent samples.  They share the image's noise realisation only through
        the network's receptive field and the background differs between them, so the pooled d' is an average over locations and
        its rows are less independent than their count suggests.  ``train=None`` scores the rows the template was built from
        (resubstitution, biased upwards); ``train=k`` holds out all but the first k pooled rows of each class (``hotelling``)."""
        return detectability_study(self, background, signal, inference_steps=inference_steps, trials=trials, centres=centres,
                                   amplitude=amplitude, sigma=sigma, seed=seed, channels=channels, n_channels=n_channels, width=width,
                                   roi=roi, train=train, max_batch=max_batch, degrade=degrade, return_images=return_images)

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
        ddim = not self._stochastic
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
        seed, sample_offset = self._seed(True, seed, sample_offset)
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
        stochastic = self._stochastic
        seed, sample_offset = self._seed(self._draws(rule), seed, sample_offset)      # (DDIM ignores ``seed``: nothing to refuse)
        _, sample_offset = check_seed(0, sample_offset)                               # (judged whether the call draws or not)
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
