"""Detectability study from the command line: is a faint Gaussian blob easier or harder to see after the sampler run?

    python -m midd_amd.observer_cli clean.png ckpt.pth --out study.json [--variant cddpm|ddim] [--img-size 256]
                                    [--trials 64] [--sigma 0.05] [--amplitude 0.05] [--signal-sigma 3.0]
                                    [--roi R] [--channels 6] [--train K] [--steps 25] [--seed N] [--max-batch 16]

The clean image is the background (grayscale, bicubic resize to --img-size, unit range); the signal is a Gaussian blob of standard
deviation --signal-sigma pixels, inserted on the non-overlapping ROI grid with --amplitude; the measurement noise is white with
standard deviation --sigma.  2 * trials noisy images, half of them with the signal, go through the sampler, and a channelized
Hotelling observer with --channels Laguerre-Gauss channels of the width matched to the blob is applied to the outputs and to the
inputs (DiffusionDenoiser.detectability).  The d' and AUC of both are printed and everything else goes to the JSON file.  The
checkpoint is loaded into the topology of ``midd_amd.cli``; pass "none" for random weights, which exercise the path and say nothing
about a trained denoiser.  ``midd_amd.cli`` itself has no option for this.
"""
from __future__ import annotations

import argparse
import json
import math

import numpy as np
import torch


def gaussian_blob(signal_sigma: float) -> np.ndarray:
    """exp(-r^2 / (2 sigma^2)) on an odd grid of half-width ceil(3 sigma), float32, 1 at its centre."""
    half = max(1, int(math.ceil(3.0 * signal_sigma)))
    d = np.arange(-half, half + 1, dtype=np.float64)
    return np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * signal_sigma ** 2)).astype(np.float32)


def _stats(det) -> dict:
    return {"dprime": det.dprime, "auc": det.auc, "template": det.template.tolist(), "mean_difference": det.mean_difference.tolist(),
            "covariance": det.covariance.tolist(), "n_train": list(det.n_train), "n_test": list(det.n_test), "dropped": list(det.dropped)}


def write_study(path: str, study, settings: dict) -> dict:
    """The study as one JSON object: the settings, the seed, the locations, and d', AUC, template and counts of both observers."""
    doc = dict(settings)
    doc.update(seed=study.seed, locations=int(study.centres.shape[0]), centres=study.centres.tolist(), roi=int(study.channels.shape[1]),
               channels=int(study.channels.shape[0]), denoised=_stats(study.denoised), noisy=_stats(study.noisy))
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(prog="python -m midd_amd.observer_cli", description=__doc__.split("\n")[0])
    ap.add_argument("image", help="the clean background image")
    ap.add_argument("checkpoint", help='a checkpoint of the reference\'s training script, or "none" for random weights')
    ap.add_argument("--out", default="study.json", help="the JSON file that receives the study")
    ap.add_argument("--variant", choices=("cddpm", "ddim"), default="cddpm")
    ap.add_argument("--img-size", type=int, default=256)
    ap.add_argument("--trials", type=int, default=64, help="noisy realisations per class")
    ap.add_argument("--sigma", type=float, default=0.05, help="standard deviation of the white measurement noise")
    ap.add_argument("--amplitude", type=float, default=0.05, help="peak of the inserted blob")
    ap.add_argument("--signal-sigma", type=float, default=3.0, help="standard deviation of the Gaussian blob in pixels")
    ap.add_argument("--roi", type=int, default=None, help="ROI side (default: the blob's side rounded up to a multiple of 8, at least 16)")
    ap.add_argument("--channels", type=int, default=6, help="number of Laguerre-Gauss channels")
    ap.add_argument("--train", type=int, default=None, help="hold out: the first K pooled rows of each class train the template (default: resubstitution)")
    ap.add_argument("--steps", type=int, default=25, help="inference steps of the sampler")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    for flag, value, low in (("--trials", a.trials, 1), ("--steps", a.steps, 1), ("--max-batch", a.max_batch, 1), ("--img-size", a.img_size, 8)):
        if value < low:
            ap.error(f"{flag} must be at least {low}")
    if a.train is not None and a.train < 2:
        ap.error("--train must be at least 2: a covariance needs two rows")
    if not a.signal_sigma > 0.0 or not math.isfinite(a.signal_sigma):
        ap.error("--signal-sigma must be positive")
    if not (a.sigma >= 0.0 and math.isfinite(a.sigma)):
        ap.error("--sigma must be a finite number >= 0")
    if a.roi is not None and not 4 <= a.roi <= 128:
        ap.error("--roi must be in [4, 128]")
    if not 1 <= a.channels <= 32:
        ap.error("--channels must be in [1, 32]")
    if torch.device(a.device).type != "cuda":
        ap.error("the study runs only on a ROCm GPU: there is no CPU fallback")

    from PIL import Image
    from .modules import UNetDiffusion
    from .sampler import DiffusionDenoiser
    model = UNetDiffusion(in_channels=1, model_channels=48, channel_mult=(1, 2, 3, 4), num_res_blocks=2,
                          attention_resolutions=(3,), dropout=0.0, time_emb_dim=192, variant=a.variant)
    checkpoint = {}
    if a.checkpoint.lower() != "none":
        checkpoint = torch.load(a.checkpoint, map_location="cpu", weights_only=True)
        model.load_state_dict(checkpoint["model_state_dict"])
    else:
        print("No checkpoint: random-init weights exercise the path; their d' says nothing about a trained denoiser")
    denoiser = DiffusionDenoiser(model.to(a.device).eval(), noise_steps=int(checkpoint.get("noise_steps", 50)))
    with Image.open(a.image) as img:
        grey = img.convert("L").resize((a.img_size, a.img_size), Image.BICUBIC)
    background = torch.from_numpy(np.asarray(grey, dtype=np.float32) / 255.0).to(a.device)
    blob = gaussian_blob(a.signal_sigma)
    study = denoiser.detectability(background, blob, inference_steps=a.steps, trials=a.trials, amplitude=a.amplitude, sigma=a.sigma,
                                   seed=a.seed, n_channels=a.channels, width=a.signal_sigma * math.sqrt(2.0 * math.pi), roi=a.roi,
                                   train=a.train, max_batch=a.max_batch)
    settings = dict(image=a.image, checkpoint=a.checkpoint, variant=a.variant, img_size=a.img_size, trials=a.trials, sigma=a.sigma,
                    amplitude=a.amplitude, signal_sigma=a.signal_sigma, train=a.train, steps=a.steps, max_batch=a.max_batch)
    write_study(a.out, study, settings)
    rows = study.noisy.n_test
    print(f"Detectability of a sigma = {a.signal_sigma} px blob of amplitude {a.amplitude} in noise of sigma {a.sigma}: "
          f"{study.centres.shape[0]} locations x {a.trials} trials a class, seed {study.seed}")
    print(f"  noisy input : d' = {study.noisy.dprime:.3f}  AUC = {study.noisy.auc:.4f}")
    print(f"  denoised    : d' = {study.denoised.dprime:.3f}  AUC = {study.denoised.auc:.4f}")
    print(f"  ({'hold-out, ' + str(a.train) + ' training rows a class' if a.train else 'resubstitution: biased upwards'}; "
          f"{rows[0]} + {rows[1]} scored rows; locations pooled as independent)")
    print(f"Study saved to {a.out}")


if __name__ == "__main__":
    main()
