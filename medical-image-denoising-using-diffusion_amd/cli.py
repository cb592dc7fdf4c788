"""Single-image inference harness — the MI355X counterpart of
``denoise_image_diffusion`` (/root/reference/Backend/cddpm/cddpmModels.py:470-504, DDIM twin
/root/reference/Backend/DDIM/DDIMModel.py:470-504) and of the script that calls it
(/root/reference/Backend/cddpminference.py:13-18): load checkpoint -> grayscale -> bicubic resize to
img_size -> sampler -> uint8 -> bicubic resize back -> PNG, with the reference's timing print.

    python -m midd_amd.cli --image in.png --out out.png [--checkpoint ckpt.pth] [--variant cddpm|ddim]
                           [--img-size 512] [--inference-steps 25] [--seed N] [--samples K [--std-out std.npy]
                           [--quantiles 0.05,0.5,0.95 --quantiles-out q.npy]]
                           [--tile N [--overlap O] [--tile-fuse end|step] [--views [auto|flips|d4] | --members K] [--std-out std.npy]
                            [--quantiles Q,Q --quantiles-out q.npy]]
                           [--self-ensemble [auto|flips|d4] [--std-out std.npy] [--quantiles Q,Q --quantiles-out q.npy]]
                           [--update reference|ddim|dpmpp2m [--eta F] [--no-clip-x0] [--x0-out traj.npy]]
                           [--bit-depth 8|16 [--window P_LO,P_HI | --window-levels LO,HI]]
                           [--clean clean.png [--loss-out loss.json]]
                           [--nps-out nps.json [--nps-roi 32|64|128] [--nps-step S]]
                           [--fidelity-out fidelity.json [--fidelity-roi 32|64|128] [--fidelity-step S]]

Without a checkpoint (the trained weights are not distributed with the reference) the network is
random-init, which exercises the path but does not denoise.  The reference helper has a latent
bug — it builds the sampler on a module-global device instead of ``device_type``
(cddpmModels.py:472 vs :268) — which is not reproduced: everything runs on the model's device.
"""
from __future__ import annotations

import argparse
import time
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from . import image16, prepost
from .modules import UNetDiffusion
from .recipe import ImageRecipe
from .sampler import (DEFAULT_SCORE_LEVELS, MAX_QUANTILE_MEMBERS, NPS_ROIS, DiffusionDenoiser, check_levels, check_nps_args, check_update,
                      check_modes, cross_spectrum, ensemble_modes, ensemble_scores, noise_power_spectrum)


class Options(NamedTuple):
    """What check_options makes of the options it judged."""
    rule: dict                                  # the update rule as keywords of the sampler calls; {} for the reference's
    quantiles: Optional[Tuple[float, ...]]      # the checked quantile levels
    recipe: ImageRecipe                         # bit_depth and the window
    nps_roi: Optional[int]                      # ROI and step with their defaults (64, ROI / 2); as given without --nps-out
    nps_step: Optional[int]
    fidelity_roi: Optional[int]
    fidelity_step: Optional[int]
    tiled_ensemble: bool                        # --views or --members


def check_options(device_type: str = "cuda", img_size: int = 512, variant: str = "cddpm", step_noise=None, seed=None, samples=None,
                  std_out=None, tile=None, quantiles=None, quantiles_out=None, self_ensemble=None, update: str = "reference",
                  eta: float = 0.0, clip_x0: bool = True, x0_out=None, bit_depth: int = 8, window=None, window_levels=None, views=None,
                  members=None, clean=None, loss_out=None, truth=None, scores_out=None, nps_out=None, nps_roi=None, nps_step=None,
                  fidelity_out=None, fidelity_roi=None, fidelity_step=None, modes=None, modes_out=None, modes_json=None,
                  tile_fuse: str = "end") -> Options:
    """The rules of denoise_image_diffusion's options (its docstring says what each option is), all of them and nowhere else: the
    function and main both call this.  Opens no file and touches no device; the two rules that compare an ROI with the image file
    itself follow the call in denoise_image_diffusion.  Raises ValueError, and RuntimeError for what runs only on a GPU."""
    on_gpu = torch.device(device_type).type == "cuda"
    if tile_fuse not in ("end", "step"):
        raise ValueError(f"--tile-fuse takes end or step (got {tile_fuse!r})")
    if tile_fuse == "step":
        if tile is None:
            raise ValueError(f"--tile-fuse {tile_fuse} fuses the tiles of the tiled run after every step: it needs --tile N")
        for flag, given in (("--members", members), ("--views", views), ("--samples", samples), ("--self-ensemble", self_ensemble)):
            if given is not None:
                raise ValueError(f"--tile-fuse {tile_fuse} cannot be combined with {flag}: the fused tiled run is one run of the image "
                                 "(fused ensembles are not built)")

    def spectrum(flag, kernel, receives, out, roi, step, missing=None):
        """--nps-out and --fidelity-out: one rule list under two flag names."""
        if (roi is not None or step is not None) and out is None:
            raise ValueError(f"--{flag}-roi and --{flag}-step need --{flag}-out PATH.json (the file that receives the {receives})")
        if out is None:
            return roi, step
        roi, step = check_nps_args(64 if roi is None else roi, step, "plane")
        if missing is not None:
            raise ValueError(missing)
        if not on_gpu:
            raise RuntimeError(f"--{flag}-out ({kernel}) runs only on a ROCm GPU: the kernel has no CPU fallback")
        if tile is None and img_size < roi:
            raise ValueError(f"--{flag}-out: the sampler's image ({img_size}x{img_size}) is smaller than the ROI ({roi}x{roi}); "
                             f"use a smaller --{flag}-roi")
        return roi, step

    n_draws = samples if samples is not None else (members if tile is not None else None)
    fidelity_roi, fidelity_step = spectrum(
        "fidelity", "cross-spectrum", "curves", fidelity_out, fidelity_roi, fidelity_step,
        None if n_draws is not None and (truth is not None or (n_draws >= 2 and n_draws % 2 == 0)) else
        "--fidelity-out needs --truth PATH beside --samples K or --tile N --members K (transfer and FRC against the "
        "truth), or an even K >= 2 of them (the FRC between the draws, which needs no truth)")
    nps_roi, nps_step = spectrum("nps", "noise power spectrum", "spectra", nps_out, nps_roi, nps_step)
    if loss_out is not None and clean is None:
        raise ValueError("--loss-out needs --clean PATH (the evaluation's clean image)")
    if scores_out is not None and truth is None:
        raise ValueError("--scores-out needs --truth PATH (the image the ensemble is scored against)")
    if truth is not None:
        if samples is None and (tile is None or members is None):
            raise ValueError("--truth scores an ensemble: it needs --samples K, or --tile N --members K")
        if (samples if samples is not None else members) > MAX_QUANTILE_MEMBERS:
            raise ValueError(f"--truth needs K <= {MAX_QUANTILE_MEMBERS} members: the scores kernel sorts a pixel's members in registers")
        if not on_gpu:
            raise RuntimeError("--truth (ensemble scores) runs only on a ROCm GPU: the scores kernel has no CPU fallback")
    if modes is not None or modes_out is not None or modes_json is not None:
        if modes is None or modes_out is None:
            raise ValueError(f"--modes M and --modes-out PATH.npy come together{'' if modes_json is None else ', and --modes-json needs both'}")
        if n_draws is None:
            raise ValueError(f"--modes {modes} takes the principal modes of an ensemble: it needs --samples K, or --tile N --members K")
        check_modes(modes, n_draws)
        if not on_gpu:
            raise RuntimeError(f"--modes {modes} (ensemble modes) runs only on a ROCm GPU: the Gram kernel has no CPU fallback")
    if clean is not None:
        for flag, given in (("--tile", tile), ("--samples", samples), ("--views", views), ("--members", members), ("--self-ensemble", self_ensemble)):
            if given is not None:
                raise ValueError(f"--clean (evaluation) cannot be combined with {flag}: the loss is taken on the resized image, one sampler run")
        if step_noise is not None or x0_out is not None:
            raise ValueError("--clean (evaluation) cannot be combined with a step_noise tensor or --x0-out")
        if not on_gpu:      # (before the sampler run, not after it)
            raise RuntimeError("--clean (evaluation) runs only on a ROCm GPU: the loss kernels have no CPU fallback")
    bit_depth = image16.check_bit_depth(bit_depth)
    if window is not None and window_levels is not None:
        raise ValueError("--window and --window-levels cannot be combined: percentiles or absolute levels, not both")
    if (window is not None or window_levels is not None) and bit_depth != 16:
        raise ValueError("--window and --window-levels need --bit-depth 16 (the window acts on 16-bit files)")
    recipe = ImageRecipe(bit_depth, window=window, window_levels=window_levels)
    rule = {} if check_update(update, eta, clip_x0) is None else {"update": update, "eta": eta, "clip_x0": clip_x0}
    if rule and self_ensemble is not None:
        raise ValueError(f"--update {update} cannot be combined with --self-ensemble (the self-ensemble runs the reference's update only)")
    if update == "dpmpp2m":
        if seed is not None or samples is not None or step_noise is not None:
            raise ValueError("--update dpmpp2m is deterministic: it takes no --seed, --samples or step_noise")
        rule = {"update": update, "clip_x0": clip_x0}
    if x0_out is not None and (update != "dpmpp2m" or tile is not None):
        raise ValueError("--x0-out needs --update dpmpp2m and no --tile: the trajectory of predicted images is that rule's")
    if self_ensemble is not None:
        if samples is not None:
            raise ValueError("--self-ensemble cannot be combined with --samples")
        if tile is not None:
            raise ValueError("--self-ensemble cannot be combined with --tile")
        if step_noise is not None:
            raise ValueError("--self-ensemble draws its noise from the seed: step_noise cannot be given as well")
        if self_ensemble not in ("auto", "flips", "d4"):
            raise ValueError(f"--self-ensemble takes auto, flips or d4 (got {self_ensemble!r})")
    if (views is not None or members is not None) and tile is None:
        raise ValueError("--views and --members are the ensembles of the tiled run: they need --tile N (without it: --self-ensemble, --samples)")
    if views is not None and members is not None:
        raise ValueError("--views and --members cannot be combined: flip / rotate views or seeded draws, not both")
    if views is not None and views not in ("auto", "flips", "d4"):
        raise ValueError(f"--views takes auto, flips or d4 (got {views!r})")
    if views is not None and update == "dpmpp2m":
        raise ValueError("--update dpmpp2m cannot be combined with --views (the tiled self-ensemble runs the reference's update or ddim)")
    if members is not None:
        if rule:
            raise ValueError(f"--update {update} cannot be combined with --members (the tiled ensemble runs the reference's update only)")
        if variant != "cddpm":
            raise ValueError("--members needs the stochastic (cddpm) variant: a deterministic sampler has no ensemble (use --views)")
        if members < 1:
            raise ValueError("--members needs K >= 1")
    tiled_ensemble = views is not None or members is not None
    if tile is not None and (samples is not None or step_noise is not None):
        raise ValueError("--tile cannot be combined with --samples or a step_noise tensor")
    if samples is not None and variant != "cddpm" and not (rule and eta > 0):
        raise ValueError("--samples needs the stochastic (cddpm) variant: a deterministic sampler has no ensemble")
    if std_out is not None and members is not None and members < 2:
        raise ValueError("--std-out needs --members K with K >= 2")
    if std_out is not None and self_ensemble is None and not tiled_ensemble and (samples is None or samples < 2):
        raise ValueError("--std-out needs --samples K with K >= 2")
    if (quantiles is None) != (quantiles_out is None):
        raise ValueError("--quantiles and --quantiles-out come together")
    if quantiles is not None:
        if members is not None and members > MAX_QUANTILE_MEMBERS:
            raise ValueError(f"--quantiles needs --members K with K <= {MAX_QUANTILE_MEMBERS}")
        if self_ensemble is None and not tiled_ensemble and (samples is None or samples > MAX_QUANTILE_MEMBERS):
            raise ValueError(f"--quantiles needs --samples K with K <= {MAX_QUANTILE_MEMBERS}")
        quantiles = check_levels(quantiles)
    if samples is not None and step_noise is not None:
        raise ValueError("samples draws its noise from the seed: step_noise cannot be given as well")
    return Options(rule, quantiles, recipe, nps_roi, nps_step, fidelity_roi, fidelity_step, tiled_ensemble)


def denoise_image_diffusion(model_path: Optional[str], test_image_path: str, device_type: str = "cuda",
                            img_size: int = 512, inference_steps: int = 50, variant: str = "cddpm",
                            step_noise: Optional[torch.Tensor] = None, compute: Optional[str] = None,
                            seed: Optional[int] = None, samples: Optional[int] = None,
                            std_out: Optional[str] = None, tile: Optional[int] = None, overlap: int = 32,
                            quantiles: Optional[Sequence[float]] = None, quantiles_out: Optional[str] = None,
                            self_ensemble: Optional[str] = None, update: str = "reference", eta: float = 0.0,
                            clip_x0: bool = True, x0_out: Optional[str] = None, bit_depth: int = 8, window: Optional[Sequence[float]] = None,
                            window_levels: Optional[Sequence[int]] = None, views: Optional[str] = None,
                            members: Optional[int] = None, clean: Optional[str] = None, loss_out: Optional[str] = None,
                            truth: Optional[str] = None, scores_out: Optional[str] = None, nps_out: Optional[str] = None,
                            nps_roi: Optional[int] = None, nps_step: Optional[int] = None, fidelity_out: Optional[str] = None,
                            fidelity_roi: Optional[int] = None, fidelity_step: Optional[int] = None, modes: Optional[int] = None,
                            modes_out: Optional[str] = None, modes_json: Optional[str] = None, tile_fuse: str = "end") -> Image.Image:
    """compute (not a reference argument): arithmetic of the network, see UNetDiffusion -- None keeps the default.
    seed (not a reference argument; cddpm): the stochastic sampler's noise is drawn on the device from this seed, so the same
    call gives the same image again (DiffusionDenoiser.denoise); None: torch.randn, as the reference.
    samples (not a reference argument; cddpm): the returned image is the MEAN of this many seeded draws
    (DiffusionDenoiser.denoise_ensemble; seed None: a seed is drawn and printed) through the same recipe; std_out: path of a
    .npy file that receives their per-pixel standard deviation, float32 [img_size, img_size] (needs samples >= 2).
    quantiles, quantiles_out (not reference arguments; cddpm, with samples <= 64): the per-pixel quantile maps of the draws at these
    levels (numbers in [0, 1], at most 8) are written to the .npy file quantiles_out, float32 [len(quantiles), img_size, img_size];
    the two come together.
    tile (not a reference argument): the image is denoised at its OWN size as blended overlapping tile x tile crops with at least
    `overlap` shared pixels (DiffusionDenoiser.denoise_tiled) -- no resize to img_size and back; both sides must be >= tile.
    views, members (not reference arguments; with tile only, one of the two): the ensembles of the TILED run, named as the Python
    calls name them.  views ("auto", "flips" or "d4"; both variants): the returned image is the MEAN over the flipped and rotated
    views of the image, each denoised as blended tiles at the image's own size (DiffusionDenoiser.denoise_tiled_self_ensemble; "auto"
    is all 8 views: the tile is square); update "ddim" works with it.  members (cddpm): the MEAN of this many seeded draws of the tiled
    run (DiffusionDenoiser.denoise_tiled_ensemble; the reference's update only).  std_out, quantiles and quantiles_out then describe
    the views / the draws, float32 at the image's own size [H, W] / [levels, H, W]; bit_depth 16 and window store the mean as they
    store the tiled image.  (samples and self_ensemble stay the ensembles of the RESIZED image and are refused together with tile.)
    tile_fuse (not a reference argument; with tile only): "end" (the default) blends the tiles once, after each has run the whole
    sampler loop alone (denoise_tiled); "step" makes the overlapping tiles agree after EVERY step (DiffusionDenoiser.denoise_tiled_fused),
    so that no tile carries its own version of a shared strip into the blend.  update, bit_depth and window work with it as with tile;
    not together with views, members, samples or self_ensemble.
    self_ensemble (not a reference argument; both variants): "auto", "flips" or "d4" -- the returned image is the MEAN over the
    flipped and rotated views of the image (DiffusionDenoiser.denoise_self_ensemble); std_out, quantiles and quantiles_out then
    describe the views instead of seeded draws.  Not together with samples or tile.
    update, eta, clip_x0 (not reference arguments; both variants): "ddim" runs the stride-aware DDIM(eta) update
    (DiffusionDenoiser.denoise) in the place of the reference's; with eta > 0 samples works for the DDIM variant too.  Not together
    with self_ensemble.  "dpmpp2m" runs the second-order multistep update: deterministic, so not together with eta, seed, samples
    or step_noise; x0_out (that rule only, not with tile): the predicted image of every iteration is saved there as float32
    [iterations, img_size, img_size].
    bit_depth (not a reference argument): 8 is the reference's recipe, unchanged.  16 keeps a 16-bit file's 65536 levels (image16.py;
    include/midd.h: THE FLOAT RESIZE): decode to unit float (/ 65535; any other file: `convert("L")` / 255), float bicubic resize to
    img_size and clip, the sampler, float resize back, clip, and a mode "I;16" image rounded to nearest -- with tile no resize at
    all.  On the GPU the resizes and conversions are the HIP kernels (prepost), bit-identical to the Pillow mode "F" / numpy recipe
    that runs around the sampler call on a CPU device.
    window, window_levels (not reference arguments; bit_depth 16 and a 16-bit file only; one of the two): the grey range [lo, hi] of
    the file is mapped to [0, 1] before the sampler and back afterwards (include/midd.h: THE WINDOW) -- window gives two percentiles
    (p_lo, p_hi) whose levels are read off the image's histogram ((0, 100): its minimum and maximum), window_levels the two levels
    themselves.  The recipe is decode, histogram, levels, windowed load (+ resize), the sampler call of any kind, (resize +) windowed
    store; values outside the window come back as lo or hi (the window clips).  With samples / self_ensemble the mean is stored through
    the window; std_out and quantiles_out stay float, in window units: one unit is hi - lo grey levels.  The levels are printed.
    clean, loss_out (not reference arguments; both variants): EVALUATION.  clean is the path of the clean counterpart of the image; it
    is loaded by the same recipe (bit_depth, the resize to img_size, and the noisy image's window if there is one).  The call prints the
    checkpoint's training objective on the pair at every timestep (DiffusionDenoiser.loss_profile; seed: the forward noise's, drawn
    and printed when None) and the PSNR / SSIM of the ordinary sampler run against the clean image (prepost.compute_metrics); loss_out
    is the path of a .json file that receives both.  The sampler run and the returned image are those of the call without clean.
    Not together with tile, samples, views, members or self_ensemble, and on a GPU only.
    truth, scores_out (not reference arguments; with samples, or with tile and members; on a GPU only): EVALUATION OF THE ENSEMBLE.
    truth is the path of the clean counterpart of the image, loaded by the recipe of clean (with tile: at its own size, which must be
    the image's).  The call prints the CRPS, the fair CRPS, the RMSE of the mean beside the spread and the coverage of the outermost
    pair of levels (quantiles if given, else 0.05, 0.25, 0.5, 0.75, 0.95) of the members against it (sampler.ensemble_scores; K <= 64);
    scores_out is the path of a .json file that receives everything, rank histogram and level counts included.  The sampler run and
    the returned image are those of the call without truth.
    nps_out, nps_roi, nps_step (not reference arguments; every kind of run; on a GPU only): THE TEXTURE OF WHAT WAS REMOVED.  nps_out is
    the path of a .json file that receives radial noise power spectra (sampler.noise_power_spectrum: Welch's method, plane detrend,
    Hann window, ROIs of nps_roi = 32, 64 (default) or 128 pixels at step nps_step, default nps_roi / 2) taken at the sampler's
    resolution (img_size, or with tile the image's own): always the method noise, input - output, which is flat if only noise was
    removed; with samples, or tile and members, K >= 2, also the ensemble's spread, member - mean scaled by K / (K - 1); with truth
    also the residual, output - truth.  Refused where the sampler's image is smaller than the ROI.  The sampler run and the returned
    image are those of the call without nps_out.
    fidelity_out, fidelity_roi, fidelity_step (not reference arguments; with samples, or with tile and members; on a GPU only): AT WHICH
    FREQUENCIES THE SIGNAL SURVIVES.  fidelity_out is the path of a .json file that receives, per radial frequency, the signal transfer
    and the Fourier ring correlation of Welch cross-spectra (sampler.cross_spectrum; plane detrend, Hann window, ROIs as for nps_out)
    and the frequency at which the FRC falls below 1/7: with truth, of (truth, output) and of (truth, noisy input); with an even
    K >= 2, between the draws 0, 2, .. and 1, 3, .., which needs no truth.  Refused with neither, and where the sampler's image is
    smaller than the ROI.  The sampler run and the returned image are those of the call without fidelity_out.
    modes, modes_out, modes_json (not reference arguments; with samples, or with tile and members, 2 <= K <= 64; on a GPU only): WHAT
    VARIES TOGETHER.  The modes leading principal modes of the draws (sampler.ensemble_modes; modes <= min(8, K - 1)) are written to
    the .npy file modes_out, float32 [modes, 1, H, W] at the sampler's resolution, in window units under window: mean +- mode j is a
    one-standard-deviation excursion along the j-th coherent pattern.  modes and modes_out come together; modes_json is the path of
    a .json file that receives the variance along each mode, its explained share, every draw's coefficients and the valid element
    count.  The sampler run and the returned image are those of the call without modes."""
    opt = check_options(device_type=device_type, img_size=img_size, variant=variant, step_noise=step_noise, seed=seed, samples=samples,
                        std_out=std_out, tile=tile, quantiles=quantiles, quantiles_out=quantiles_out, self_ensemble=self_ensemble,
                        update=update, eta=eta, clip_x0=clip_x0, x0_out=x0_out, bit_depth=bit_depth, window=window,
                        window_levels=window_levels, views=views, members=members, clean=clean, loss_out=loss_out, truth=truth,
                        scores_out=scores_out, nps_out=nps_out, nps_roi=nps_roi, nps_step=nps_step, fidelity_out=fidelity_out,
                        fidelity_roi=fidelity_roi, fidelity_step=fidelity_step, modes=modes, modes_out=modes_out, modes_json=modes_json,
                        tile_fuse=tile_fuse)
    rule, quantiles, recipe, tiled_ensemble = opt.rule, opt.quantiles, opt.recipe, opt.tiled_ensemble
    nps_roi, nps_step, fidelity_roi, fidelity_step = opt.nps_roi, opt.nps_step, opt.fidelity_roi, opt.fidelity_step
    for flag, out, roi in (("fidelity", fidelity_out, fidelity_roi), ("nps", nps_out, nps_roi)):
        if out is not None and tile is not None:      # the tiled run keeps the image's own size
            with Image.open(test_image_path) as probe:
                if min(probe.size) < roi:
                    raise ValueError(f"--{flag}-out: the image ({probe.size[1]}x{probe.size[0]}) is smaller than the ROI ({roi}x{roi}); "
                                     f"use a smaller --{flag}-roi")
    device = torch.device(device_type)
    model = UNetDiffusion(in_channels=1, model_channels=48, channel_mult=(1, 2, 3, 4), num_res_blocks=2,
                          attention_resolutions=(3,), dropout=0.0, time_emb_dim=192, variant=variant, compute=compute)
    checkpoint = {}
    if model_path:
        checkpoint = torch.load(model_path, map_location="cpu", weights_only=True)
        model.load_state_dict(checkpoint["model_state_dict"])
    model = model.to(device).eval()
    diffusion = DiffusionDenoiser(model, noise_steps=int(checkpoint.get("noise_steps", 50)))
    print(f"Loaded model - PSNR: {checkpoint.get('best_psnr', 'N/A')} dB | SSIM: {checkpoint.get('best_ssim', 'N/A')}")

    img = Image.open(test_image_path)
    on_gpu = device.type == "cuda"
    size = None if tile is not None else img_size      # the sampler's resolution: img_size, or with tile the image's own (no resize)
    input_tensor, source = recipe.load(img, None if size is None else (size, size), device)
    win = source.levels       # the window's levels: int32 [1,2] on the device (they stay there: no synchronisation), or (lo, hi) on the host
    if win is not None and not on_gpu:
        print(f"Window: grey levels {win[0]} .. {win[1]}")

    def restored(image: torch.Tensor) -> Image.Image:
        if win is not None and on_gpu:
            print("Window: grey levels {} .. {}".format(*win[0].tolist()))
        return Image.fromarray(recipe.store(image, source))

    keep = truth is not None or nps_out is not None or fidelity_out is not None or modes is not None      # the members are needed after the run
    truth_img = None
    if tile is not None:
        if min(img.size) < tile:
            raise ValueError(f"the image is {img.size[1]}x{img.size[0]}: a side is shorter than the tile ({tile}); use a smaller "
                             "--tile, or leave it out so that the image is resized to img_size")
        start_time = time.time()
        if views is not None:
            draws = variant == "cddpm" if not rule else eta > 0
            res = diffusion.denoise_tiled_self_ensemble(input_tensor, inference_steps=inference_steps, views=views, tile=tile, overlap=overlap,
                                                        seed=seed if draws else None, quantiles=quantiles, **rule)
            what = f"Self-ensemble of {len(res.views)} views {res.views}, tiled"
        elif members is not None:
            res = diffusion.denoise_tiled_ensemble(input_tensor, inference_steps=inference_steps, members=members, tile=tile, overlap=overlap,
                                                   seed=seed, quantiles=quantiles, return_samples=keep)
            what = f"Ensemble of {members} samples, tiled"
        else:
            run = diffusion.denoise_tiled_fused if tile_fuse == "step" else diffusion.denoise_tiled
            res = run(input_tensor, inference_steps=inference_steps, tile=tile, overlap=overlap, seed=seed, **rule)
            what = "Tiled, fused after every step" if tile_fuse == "step" else "Tiled"
        if on_gpu:
            torch.cuda.synchronize(device)
        print(f"{what}: {len(res.origins_y)} x {len(res.origins_x)} tiles of {tile}" + (f", seed {res.seed}" if res.seed is not None else ""))
        print(f"Inference time: {time.time() - start_time:.2f} seconds")
        image = res.mean if tiled_ensemble else res.image      # the mean of values in [0, 1] is in [0, 1]: stored as the tiled image is
        if truth is not None:
            truth_img = load_truth(truth, res.samples, size, recipe, win)
            score(res.samples, truth_img, quantiles if quantiles is not None else DEFAULT_SCORE_LEVELS, res.seed, scores_out)
        if nps_out is not None:
            write_nps(nps_out, nps_roi, nps_step, input_tensor, image, res.samples if members is not None else None, truth_img, res.seed)
        if fidelity_out is not None:
            write_fidelity(fidelity_out, fidelity_roi, fidelity_step, input_tensor, image, res.samples, truth_img, res.seed)
        if modes is not None:
            write_modes(modes, modes_out, modes_json, res.samples, res.seed)
        if tiled_ensemble:      # the maps stay float, at the image's size
            if std_out is not None:
                np.save(std_out, res.std[0, 0].cpu().numpy())
            if quantiles is not None:
                np.save(quantiles_out, res.quantiles[0, :, 0].cpu().numpy())
        return restored(image)

    start_time = time.time()
    kw = {"step_noise": step_noise} if step_noise is not None else {}
    if seed is not None:
        kw["seed"] = seed
    if self_ensemble is not None:
        ens = diffusion.denoise_self_ensemble(input_tensor, inference_steps=inference_steps, views=self_ensemble,
                                              seed=seed if variant == "cddpm" else None, quantiles=quantiles)
        denoised = ens.mean                               # a mean of values in [0, 1]: in [0, 1]
        print(f"Self-ensemble of {len(ens.views)} views {ens.views}" + (f", seed {ens.seed}" if ens.seed is not None else ""))
    elif samples is not None:
        ens = diffusion.denoise_ensemble(input_tensor, inference_steps=inference_steps, members=samples, seed=seed, quantiles=quantiles,
                                         return_samples=keep, **rule)
        denoised = ens.mean                               # a mean of values in [0, 1]: in [0, 1]
        print(f"Ensemble of {samples} samples, seed {ens.seed}")
        if truth is not None:
            truth_img = load_truth(truth, ens.samples, size, recipe, win)
            score(ens.samples, truth_img, quantiles if quantiles is not None else DEFAULT_SCORE_LEVELS, ens.seed, scores_out)
    elif x0_out is not None:
        denoised, traj = diffusion.denoise(input_tensor, inference_steps=inference_steps, return_x0=True, **rule)
        np.save(x0_out, traj.reshape(traj.shape[0], img_size, img_size).cpu().numpy())      # float32 [n_iters, H, W], model resolution
    else:
        denoised = diffusion.denoise(input_tensor, inference_steps=inference_steps, **kw, **rule)
    if self_ensemble is not None or samples is not None:
        if std_out is not None:
            np.save(std_out, ens.std.reshape(img_size, img_size).cpu().numpy())
        if quantiles is not None:
            np.save(quantiles_out, ens.quantiles.reshape(len(quantiles), img_size, img_size).cpu().numpy())
    if on_gpu:
        torch.cuda.synchronize(device)
    print(f"Inference time: {time.time() - start_time:.2f} seconds")
    denoised = denoised.reshape(1, 1, img_size, img_size)
    if clean is not None:
        evaluate(diffusion, clean, input_tensor, denoised, img_size, recipe, win, seed, loss_out)
    if nps_out is not None:
        write_nps(nps_out, nps_roi, nps_step, input_tensor, denoised, ens.samples if samples is not None else None, truth_img,
                  ens.seed if samples is not None else seed)
    if fidelity_out is not None:
        write_fidelity(fidelity_out, fidelity_roi, fidelity_step, input_tensor, denoised, ens.samples, truth_img, ens.seed)
    if modes is not None:
        write_modes(modes, modes_out, modes_json, ens.samples, ens.seed)
    return restored(denoised)


def load_counterpart(path: str, device, img_size: Optional[int], recipe: ImageRecipe, win) -> torch.Tensor:
    """The clean counterpart of the noisy image (--clean, --truth) as the [1, 1, H, W] tensor the sampler's input is: the same
    recipe -- bit_depth, the resize to img_size (None: --tile, the image's own size, no resize) and the NOISY image's window levels
    `win` (on the GPU a device int32 [1, 2]) if it has a window."""
    return recipe.load(Image.open(path), None if img_size is None else (img_size, img_size), device, levels=win)[0]


def load_truth(path: str, samples: torch.Tensor, img_size: Optional[int], recipe: ImageRecipe, win) -> torch.Tensor:
    """--truth for the ensemble `samples` [1, K, 1, H, W]: load_counterpart, float32 [1, 1, H, W], refused at another size."""
    truth = load_counterpart(path, samples.device, img_size, recipe, win).float()
    if tuple(truth.shape[2:]) != tuple(samples.shape[3:]):
        raise ValueError(f"--truth is {truth.shape[2]}x{truth.shape[3]}, the ensemble {samples.shape[3]}x{samples.shape[4]}: the truth image "
                         "must have the size of --image")
    return truth


def score(samples: torch.Tensor, truth: torch.Tensor, levels, seed, scores_out: Optional[str]) -> dict:
    """--truth: the scores of the ensemble `samples` [1, K, 1, H, W] against the truth image (sampler.ensemble_scores), printed and,
    with scores_out, written as JSON.  The truth went through the recipe of the noisy image (load_truth)."""
    import json
    sc = ensemble_scores(samples, truth, levels)
    result = {"members": int(samples.shape[1]), "height": int(truth.shape[2]), "width": int(truth.shape[3]), "seed": seed,
              "crps": float(sc.crps[0]), "crps_fair": float(sc.crps_fair[0]), "rmse": float(sc.rmse[0]), "spread": float(sc.spread[0]),
              "valid": int(sc.valid[0]), "sums": sc.sums[0].tolist(), "rank_hist": sc.rank_hist[0].tolist(), "levels": list(sc.levels),
              "count_lt": sc.count_lt[0].tolist(), "count_le": sc.count_le[0].tolist(),
              "coverage": None if not sc.levels else float(sc.coverage()[0])}
    print(f"Ensemble of {result['members']} members against the truth image ({result['valid']} valid pixels):")
    print(f"  CRPS {result['crps']:.6f} | fair CRPS {result['crps_fair']:.6f} | RMSE of the mean {result['rmse']:.6f} | spread {result['spread']:.6f}")
    if sc.levels:
        print(f"  coverage of the {sc.levels[0]:g} .. {sc.levels[-1]:g} interval: {result['coverage']:.4f} (nominal {sc.levels[-1] - sc.levels[0]:.4f})")
    if scores_out is not None:
        with open(scores_out, "w") as f:
            json.dump(result, f, indent=1)
        print(f"Scores saved: {scores_out}")
    return result


def write_modes(modes: int, modes_out: str, modes_json: Optional[str], samples: torch.Tensor, seed) -> dict:
    """--modes: the leading principal modes of the ensemble `samples` [1, K, 1, H, W] (sampler.ensemble_modes), saved as float32
    [modes, 1, H, W] in the sampler's units (window units under --window), their figures printed and, with modes_json, written as JSON."""
    import json
    pm = ensemble_modes(samples, modes)
    np.save(modes_out, pm.modes[0].cpu().numpy())
    result = {"members": int(samples.shape[1]), "modes": modes, "height": int(samples.shape[3]), "width": int(samples.shape[4]), "seed": seed,
              "variance": pm.variance[0].tolist(), "explained": pm.explained[0].tolist(), "coefficients": pm.coefficients[0].tolist(),
              "total_variance": float(pm.total_variance[0]), "valid": int(pm.valid[0])}
    print(f"Principal modes of {result['members']} members ({result['valid']} valid elements): explained " +
          ", ".join(f"{v:.4f}" for v in result["explained"]))
    print(f"Modes saved: {modes_out}")
    if modes_json is not None:
        with open(modes_json, "w") as f:
            json.dump(result, f, indent=1)
        print(f"Mode figures saved: {modes_json}")
    return result


def write_nps(nps_out: str, roi: int, step: int, noisy: torch.Tensor, output: torch.Tensor, samples: Optional[torch.Tensor],
              truth: Optional[torch.Tensor], seed) -> dict:
    """--nps-out: the radial noise power spectra of the run at the sampler's resolution, printed in short and written as JSON.  noisy,
    output and the truth (load_truth, or None) are [1, 1, H, W]; samples [1, K, 1, H, W] or None."""
    import json

    def entry(sp, **more):
        return dict(radial=sp.radial[0, 0].tolist(), radial_count=sp.radial_count.tolist(), rois_used=int(sp.rois_used[0, 0]),
                    rois_skipped=int(sp.rois_skipped[0, 0]), variance=float(sp.variance()[0, 0]), **more)

    out = output.float().contiguous()
    first = noise_power_spectrum(noisy.float(), out, roi, step)
    result = {"roi": roi, "step": step, "detrend": "plane", "window": "hann", "height": int(out.shape[2]), "width": int(out.shape[3]),
              "seed": seed, "freqs": first.freqs.tolist(), "method_noise": entry(first)}
    if samples is not None and samples.shape[1] >= 2:
        K = int(samples.shape[1])
        result["ensemble_spread"] = entry(noise_power_spectrum(samples, out, roi, step, scale=K / (K - 1)), members=K)
    if truth is not None:
        result["residual"] = entry(noise_power_spectrum(out, truth, roi, step))
    print(f"Noise power spectrum ({roi} x {roi} ROIs at step {step}, plane detrend, Hann window; cycles per pixel):")
    for name in ("method_noise", "ensemble_spread", "residual"):
        if name in result:
            e = result[name]
            lowf, highf = e["radial"][1], e["radial"][roi // 4]
            print(f"  {name}: {e['rois_used']} ROIs, variance {e['variance']:.3e}, NPS at f = {1 / roi:.4f}: {lowf:.3e}, at f = 0.25: {highf:.3e}")
    with open(nps_out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"Noise power spectra saved: {nps_out}")
    return result


def write_fidelity(fidelity_out: str, roi: int, step: int, noisy: torch.Tensor, output: torch.Tensor, samples: torch.Tensor,
                   truth: Optional[torch.Tensor], seed) -> dict:
    """--fidelity-out: at which spatial frequencies the signal survives the run (sampler.cross_spectrum), printed in short and written
    as JSON.  noisy and output are [1, 1, H, W], samples [1, K, 1, H, W].  With a truth ([1, 1, H, W], load_truth): the
    transfer, the FRC and the resolution of (truth, output) and of (truth, noisy).  With an even K >= 2: the FRC between the draws
    samples[:, 0::2] and samples[:, 1::2], which needs no truth."""
    import json

    def entry(sp, **more):
        return dict(transfer=sp.transfer()[0, 0].tolist(), frc=sp.frc()[0, 0].tolist(), resolution=float(sp.resolution()[0, 0]),
                    rois_used=int(sp.rois_used[0, 0]), rois_skipped=int(sp.rois_skipped[0, 0]), **more)

    out = output.float().contiguous()
    K = int(samples.shape[1])
    result = {"roi": roi, "step": step, "detrend": "plane", "window": "hann", "height": int(out.shape[2]), "width": int(out.shape[3]),
              "seed": seed, "freqs": [r / roi for r in range(roi // 2 + 1)]}
    if truth is not None:
        result["truth_output"] = entry(cross_spectrum(truth, out, roi, step))
        result["truth_noisy"] = entry(cross_spectrum(truth, noisy.float(), roi, step))
    if K >= 2 and K % 2 == 0:
        result["draws"] = entry(cross_spectrum(samples[:, 0::2], samples[:, 1::2], roi, step), members=K)
    print(f"Spectral fidelity ({roi} x {roi} ROIs at step {step}, plane detrend, Hann window; cycles per pixel):")
    for name in ("truth_output", "truth_noisy", "draws"):
        if name in result:
            e = result[name]
            print(f"  {name}: {e['rois_used']} ROIs, FRC at f = 0.25: {e['frc'][roi // 4]:.3f}, transfer at f = 0.25: {e['transfer'][roi // 4]:.3f}, "
                  f"FRC below 1/7 at f = {e['resolution']:.4f}")
    with open(fidelity_out, "w") as f:
        json.dump(result, f, indent=1)
    print(f"Spectral fidelity saved: {fidelity_out}")
    return result


def evaluate(diffusion: DiffusionDenoiser, clean_path: str, noisy: torch.Tensor, denoised: torch.Tensor, img_size: int, recipe: ImageRecipe,
             win, seed: Optional[int], loss_out: Optional[str]) -> dict:
    """--clean: the loss profile of the (clean, noisy) pair over all timesteps and the PSNR / SSIM of `denoised` against the clean
    image, printed and, with loss_out, written as JSON.  The clean image goes through the recipe the noisy one went through; a
    window's levels are the noisy image's."""
    import json
    clean = load_counterpart(clean_path, noisy.device, img_size, recipe, win)
    prof = diffusion.loss_profile(clean, noisy, seed=seed)
    psnr, ssim = prepost.compute_metrics(denoised.float(), clean)
    variant = getattr(diffusion.model, "variant", "ddim")
    result = {"variant": variant, "noise_steps": diffusion.noise_steps, "img_size": img_size, "t": list(prof.t),
              "loss": prof.loss[:, 0].tolist(), "mse": prof.mse[:, 0].tolist(), "edge": prof.edge[:, 0].tolist(),
              "psnr": float(psnr), "ssim": float(ssim)}
    print(f"Denoising loss of the checkpoint on this pair ({variant} objective), per timestep:")
    print("    t        loss         mse        edge")
    for k, t in enumerate(prof.t):
        print(f"  {t:3d}  {result['loss'][k]:10.6f}  {result['mse'][k]:10.6f}  {result['edge'][k]:10.6f}")
    print(f"Sampler run against the clean image: PSNR {psnr:.2f} dB | SSIM {ssim:.4f}")
    if loss_out is not None:
        with open(loss_out, "w") as f:
            json.dump(result, f, indent=1)
        print(f"Loss profile saved: {loss_out}")
    return result


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--image", required=True)
    ap.add_argument("--out", default="denoised_diffusion_result.png")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--variant", default="cddpm", choices=["cddpm", "ddim"])
    ap.add_argument("--img-size", type=int, default=512)
    ap.add_argument("--inference-steps", type=int, default=25)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--seed", type=int, default=None,
                    help="cddpm: draw the sampler's noise on the device from this seed (reproducible); default: torch.randn")
    ap.add_argument("--samples", type=int, default=None,
                    help="cddpm: save the mean of this many seeded samples of the image (with --seed: reproducible)")
    ap.add_argument("--std-out", default=None, metavar="PATH.npy",
                    help="with --samples K >= 2: write the per-pixel standard deviation of the samples (float32, model resolution)")
    ap.add_argument("--quantiles", default=None, metavar="Q,Q,...",
                    help="with --samples K <= 64 and --quantiles-out: per-pixel quantile maps of the samples at these levels in [0, 1] (at most 8)")
    ap.add_argument("--quantiles-out", default=None, metavar="PATH.npy",
                    help="with --quantiles: write the quantile maps (float32 [levels, H, W], model resolution)")
    ap.add_argument("--tile", type=int, default=None, metavar="N",
                    help="denoise the image at its own size as blended overlapping N x N tiles (N: a multiple of 8) instead of resizing it to --img-size")
    ap.add_argument("--overlap", type=int, default=32, help="with --tile: minimum overlap of neighbouring tiles (<= N / 2)")
    ap.add_argument("--tile-fuse", default="end", choices=["end", "step"],
                    help="with --tile: end (the default) blends the tiles once, after the last step; step makes the overlapping tiles "
                         "agree after every sampler step (not with --views, --members, --samples or --self-ensemble)")
    ap.add_argument("--views", nargs="?", const="auto", default=None, choices=["auto", "flips", "d4"],
                    help="with --tile, both variants: save the mean over the flipped and rotated views of the image, each denoised as "
                         "blended tiles at the image's own size (auto: all 8); --std-out and --quantiles / --quantiles-out then describe "
                         "the views, at the image's size")
    ap.add_argument("--members", type=int, default=None, metavar="K",
                    help="with --tile, cddpm: save the mean of this many seeded samples of the tiled run; --std-out (K >= 2) and "
                         "--quantiles / --quantiles-out (K <= 64) then describe them, at the image's size")
    ap.add_argument("--self-ensemble", nargs="?", const="auto", default=None, choices=["auto", "flips", "d4"],
                    help="both variants: save the mean over the flipped and rotated views of the image (auto: all 8); --std-out and "
                         "--quantiles / --quantiles-out then describe the views")
    ap.add_argument("--update", default="reference", choices=["reference", "ddim", "dpmpp2m"],
                    help="the sampler's update rule: reference (one-step ancestral, the default), ddim (stride-aware DDIM(eta) step) or "
                         "dpmpp2m (second-order multistep step, deterministic)")
    ap.add_argument("--eta", type=float, default=0.0, help="with --update ddim: 0 (deterministic, the default) .. 1 (ancestral)")
    ap.add_argument("--no-clip-x0", action="store_true", help="with --update ddim or dpmpp2m: do not clip the predicted image to [0, 1]")
    ap.add_argument("--x0-out", default=None, metavar="PATH.npy",
                    help="with --update dpmpp2m: write the predicted image of every iteration (float32 [iterations, H, W], model resolution)")
    ap.add_argument("--bit-depth", type=int, default=8, choices=[8, 16],
                    help="8 (the default): the reference's 8-bit recipe; 16: keep a 16-bit file's levels -- float resize, 16-bit PNG out")
    ap.add_argument("--window", default=None, metavar="P_LO,P_HI",
                    help="with --bit-depth 16 and a 16-bit file: map the grey range between these two percentiles of the image (0,100: its "
                         "minimum and maximum) to [0, 1] for the sampler and back afterwards; values outside come back clipped to the "
                         "range.  --std-out and --quantiles-out stay float in window units: one unit is hi - lo grey levels")
    ap.add_argument("--window-levels", default=None, metavar="LO,HI",
                    help="as --window, with the two grey levels given (0 <= LO < HI <= 65535) instead of read off the histogram")
    ap.add_argument("--clean", default=None, metavar="PATH",
                    help="evaluation: the clean counterpart of --image; prints the checkpoint's denoising loss on the pair at every timestep "
                         "and the PSNR / SSIM of the sampler run against it (not with --tile, --samples, --views, --members, --self-ensemble)")
    ap.add_argument("--loss-out", default=None, metavar="PATH.json", help="with --clean: write the loss profile and the metrics as JSON")
    ap.add_argument("--truth", default=None, metavar="PATH",
                    help="with --samples K, or --tile N --members K (K <= 64): the clean counterpart of --image; prints the CRPS, fair CRPS, "
                         "RMSE, spread and interval coverage of the ensemble against it (levels: --quantiles, else 0.05,0.25,0.5,0.75,0.95)")
    ap.add_argument("--scores-out", default=None, metavar="PATH.json",
                    help="with --truth: write the scores, the rank histogram and the level counts as JSON")
    ap.add_argument("--nps-out", default=None, metavar="PATH.json",
                    help="write radial noise power spectra (Welch, plane detrend, Hann window) at the sampler's resolution: the method noise "
                         "input - output; with --samples K or --tile N --members K (K >= 2) also the ensemble's spread; with --truth also "
                         "the residual output - truth")
    ap.add_argument("--nps-roi", type=int, default=None, metavar="R", help="with --nps-out: the ROI size, 32, 64 (default) or 128")
    ap.add_argument("--nps-step", type=int, default=None, metavar="S", help="with --nps-out: the ROI step (default R / 2)")
    ap.add_argument("--fidelity-out", default=None, metavar="PATH.json",
                    help="write the signal transfer and the Fourier ring correlation per radial frequency as JSON: with --truth (beside "
                         "--samples K or --tile N --members K) of (truth, output) and (truth, noisy input); with an even K also between the "
                         "draws, which needs no truth")
    ap.add_argument("--fidelity-roi", type=int, default=None, metavar="R", help="with --fidelity-out: the ROI size, 32, 64 (default) or 128")
    ap.add_argument("--fidelity-step", type=int, default=None, metavar="S", help="with --fidelity-out: the ROI step (default R / 2)")
    ap.add_argument("--modes", type=int, default=None, metavar="M",
                    help="with --samples K, or --tile N --members K (2 <= K <= 64), and --modes-out: the M <= min(8, K - 1) leading principal "
                         "modes of the draws, what varies together; mean +- a mode is a one-standard-deviation excursion along it")
    ap.add_argument("--modes-out", default=None, metavar="PATH.npy",
                    help="with --modes: the modes as float32 [M, 1, H, W] at the sampler's resolution (window units under --window)")
    ap.add_argument("--modes-json", default=None, metavar="PATH.json",
                    help="with --modes: write the variance along each mode, its explained share, the draws' coefficients and the valid count")
    args = ap.parse_args(argv)
    # the rules that are main's own: the text arguments and the ranges argv words; every other rule is check_options'
    for flag, roi, step in (("fidelity", args.fidelity_roi, args.fidelity_step), ("nps", args.nps_roi, args.nps_step)):
        if roi is not None and roi not in NPS_ROIS:
            ap.error(f"--{flag}-roi needs one of {NPS_ROIS}")
        if step is not None and step < 1:
            ap.error(f"--{flag}-step needs S >= 1")
    if args.update == "reference" and (args.eta != 0.0 or args.no_clip_x0):
        ap.error("--eta and --no-clip-x0 need --update ddim")
    if not 0.0 <= args.eta <= 1.0:
        ap.error("--eta needs a value in [0, 1]")
    if args.update == "dpmpp2m" and args.eta != 0.0:
        ap.error("--update dpmpp2m is deterministic: it takes no --eta, --seed or --samples")
    if args.tile is not None and args.tile < 1:
        ap.error("--tile needs N >= 1")
    if args.samples is not None and args.samples < 1:
        ap.error("--samples needs K >= 1")
    options = dict(device_type=args.device, img_size=args.img_size, variant=args.variant, seed=args.seed, samples=args.samples,
                   std_out=args.std_out, tile=args.tile, quantiles=None, quantiles_out=args.quantiles_out, self_ensemble=args.self_ensemble,
                   update=args.update, eta=args.eta, clip_x0=not args.no_clip_x0, bit_depth=args.bit_depth)
    later = dict(x0_out=args.x0_out, window=None, window_levels=None, views=args.views, members=args.members, clean=args.clean,
                 loss_out=args.loss_out, truth=args.truth, scores_out=args.scores_out, nps_out=args.nps_out, nps_roi=args.nps_roi,
                 nps_step=args.nps_step, fidelity_out=args.fidelity_out, fidelity_roi=args.fidelity_roi, fidelity_step=args.fidelity_step,
                 modes=args.modes, modes_out=args.modes_out, modes_json=args.modes_json,
                 tile_fuse=None if args.tile_fuse == "end" else args.tile_fuse)
    try:
        if args.quantiles is not None:
            options["quantiles"] = check_levels([float(v) for v in args.quantiles.split(",")])
    except ValueError as exc:
        ap.error(f"--quantiles needs up to 8 comma-separated levels in [0, 1]: {exc}")
    try:
        if args.window is not None:
            later["window"] = image16.parse_pair(args.window, "--window")
        if args.window_levels is not None:
            later["window_levels"] = image16.parse_pair(args.window_levels, "--window-levels")
        options.update({k: v for k, v in later.items() if v is not None})      # the later options are passed on only where given
        opt = check_options(**options)
    except ValueError as exc:
        ap.error(str(exc))
    options.update(quantiles=opt.quantiles, **{k: v for k, v in (("window", opt.recipe.window), ("window_levels", opt.recipe.window_levels))
                                              if v is not None})
    restored = denoise_image_diffusion(args.checkpoint, args.image, inference_steps=args.inference_steps, overlap=args.overlap, **options)
    restored.save(args.out, quality=95)
    print(f"\nResult saved: {args.out}")


if __name__ == "__main__":
    main()
