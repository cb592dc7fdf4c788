"""Time of one denoising-loss evaluation (DiffusionDenoiser.denoising_loss: noising, forward, loss kernels in one native call) next
to the same forward wrapped in torch ops and to the forward alone, in one process:

    native    den.denoising_loss(clean, noisy, t, seed=S)
    torch     torch.randn_like + the noising expression, den.model(x_t, noisy, t), clamp, the predicted image, per-sample mean of
              the squared error, four F.conv2d Sobel convolutions, the magnitudes, per-sample mean of their absolute difference
    forward   den.model(x_t, noisy, t) on a prepared x_t

at B = 8, 256 x 256, per-sample timesteps, full-width DDIM-variant network with random-init weights.  The arms are interleaved
(native, torch, forward, native, ...) so that clock drift hits all alike; median [min - max] of at least 5 timed calls per arm is
reported, never a single run.  The two new launches are also timed on their own (a batch of launches between two events), with the
bytes each has to move and the rate that makes -- to be read against the copy rate of the same device in profiles/r03_mb_hbm_rate.txt.

    python tools/denoising_loss_ab.py [--reps 7] [--warmup 2] > profiles/denoising_loss_ab.json

Prints ONE JSON object; `mi_source_hash` names the library build the numbers belong to."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import midd_loader  # noqa: E402

midd_loader.load()
import midd_amd  # noqa: E402
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

B, SIZE, SEED = 8, 256, 20261020
T = (49, 40, 33, 25, 18, 11, 5, 1)
LAUNCHES = 50             # launches between the two events of a kernel-alone timing


def torch_loss(den, clean, noisy, t, kx, ky):
    """The objective with torch ops round the native forward -> (mse, edge, loss) [B]."""
    ah = den.alpha_hat[t][:, None, None, None]
    a, s = torch.sqrt(ah), torch.sqrt(1 - ah)
    eps = torch.randn_like(clean)
    x_t = a * clean + s * eps
    e = torch.clamp(den.model(x_t, noisy, t), -5, 5)
    p = torch.clamp((x_t - s * e) / a, 0, 1)
    mse = ((e - eps) ** 2).mean(dim=(1, 2, 3))
    mp = torch.sqrt(F.conv2d(p, kx, padding=1) ** 2 + F.conv2d(p, ky, padding=1) ** 2 + 1e-8)
    mc = torch.sqrt(F.conv2d(clean, kx, padding=1) ** 2 + F.conv2d(clean, ky, padding=1) ** 2 + 1e-8)
    edge = (mp - mc).abs().mean(dim=(1, 2, 3))
    return mse, edge, mse + 0.2 * edge


def summary(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def alone(fn, reps, warmup):
    """-> us per launch {median, min, max} of `fn`, LAUNCHES launches between two events per timed sample."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out = []
    for rep in range(warmup + reps):
        ev[0].record()
        for _ in range(LAUNCHES):
            fn()
        ev[1].record()
        ev[1].synchronize()
        if rep >= warmup:
            out.append(1e3 * ev[0].elapsed_time(ev[1]) / LAUNCHES)
    return summary(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7, help="timed calls per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("denoising_loss_ab.py needs a GPU")
    model = UNetDiffusion()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(UNetConfig(), seed=42).items()})
    den = DiffusionDenoiser(model.to("cuda").eval(), noise_steps=50)
    clean = torch.from_numpy(synthetic_xray(B, SIZE, SIZE, seed=77)).cuda()
    noisy = (clean + 0.1 * torch.randn_like(clean)).clamp(0, 1)
    t = torch.tensor(T, device="cuda")
    kx = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=torch.float32, device="cuda").view(1, 1, 3, 3)
    ky = kx.transpose(2, 3).contiguous()
    x_t, eps = den.noise_images(clean, T, seed=SEED)
    pred = den.model(x_t, noisy, t)
    arms = {"native": lambda: den.denoising_loss(clean, noisy, T, seed=SEED),
            "torch": lambda: torch_loss(den, clean, noisy, t, kx, ky),
            "forward": lambda: den.model(x_t, noisy, t)}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = {name: [] for name in arms}
    for rep in range(a.warmup + a.reps):
        for name, fn in arms.items():
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            if rep >= a.warmup:
                per[name].append(ev[0].elapsed_time(ev[1]))
    row = {name: {"ms_per_call": summary(ms)} for name, ms in per.items()}
    fwd = row["forward"]["ms_per_call"]
    row["native_over_forward_time"] = row["native"]["ms_per_call"]["median"] / fwd["median"]
    row["torch_over_forward_time"] = row["torch"]["ms_per_call"]["median"] / fwd["median"]
    row["native_over_torch_time"] = row["native"]["ms_per_call"]["median"] / row["torch"]["ms_per_call"]["median"]
    row["forward_spread"] = (fwd["max"] - fwd["min"]) / fwd["median"]
    # agreement of the two evaluations on a caller's noise tensor (the torch arm fuses nothing and sums in fp32)
    nat = den.denoising_loss(clean, noisy, T, noise=eps)
    e = torch.clamp(pred, -5, 5)
    row["native_mse_vs_torch_mse_max_rel"] = float(((nat.mse - ((e - eps) ** 2).mean(dim=(1, 2, 3)).double()).abs() / nat.mse).max())

    alone_rows = {}
    ah = den.alpha_hat.cpu().numpy()      # a host table: the plan-free calls copy a device tensor per call, which waits for the stream
    for shape in ((B, 1, SIZE, SIZE), (64, 1, 512, 512)):       # the measured batch, and one whose launches outlast their own host path
        n = shape[0]
        c = clean if n == B else torch.rand(shape, device="cuda")
        tt = T if n == B else tuple(T[i % len(T)] for i in range(n))
        xt, e = midd_amd.noise_images(c, tt, ah, seed=SEED)
        pr = pred if n == B else torch.randn(shape, device="cuda")
        image_bytes = c.numel() * 4
        kernels = {
            "noise_images explicit": (lambda: midd_amd.noise_images(c, tt, ah, noise=e), 3 * image_bytes),
            "noise_images seeded, eps exported": (lambda: midd_amd.noise_images(c, tt, ah, seed=SEED), 3 * image_bytes),
            "loss_terms explicit": (lambda: midd_amd.loss_terms(c, pr, tt, ah, x_t=xt, noise=e), 4 * image_bytes),
            "loss_terms seeded": (lambda: midd_amd.loss_terms(c, pr, tt, ah, seed=SEED), 2 * image_bytes),
        }
        rows = {}
        for name, (fn, nbytes) in kernels.items():
            us = alone(fn, a.reps, a.warmup)
            rows[name] = {"us_per_call": us, "bytes": nbytes, "GB_per_s_at_median": nbytes / us["median"] / 1e3}
        alone_rows["x".join(str(v) for v in shape)] = rows
    print(json.dumps({
        "tool": "tools/denoising_loss_ab.py",
        "metric": "wall time of one loss evaluation (events around the call, status word read back in every arm) -- the native chained call, "
                  "the same forward wrapped in torch ops, the forward alone -- interleaved in one process; and the new launches alone: "
                  "us per Python call over %d back-to-back calls (host launch path and output allocation included), with the bytes the "
                  "launch must move (halo re-reads not counted)" % LAUNCHES,
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "shape": [B, 1, SIZE, SIZE], "t": list(T), "reps": a.reps, "warmup": a.warmup,
        "weights": "random-init (make_state_dict seed 42)", "calls": row, "launches_alone": alone_rows}))


if __name__ == "__main__":
    main()
