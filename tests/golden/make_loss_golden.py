"""Records the fixture of the denoising-loss checks (tests/test_denoising_loss_cpu.py) FROM THE REFERENCE ITSELF.
Build container only (needs the reference):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_loss_golden.py

Same recipe as the other generators (reference imported in-process by ref_import.py, the reduced topology with weights from the
package's portable generator, formula-generated inputs, arrays only).  Per variant the reference's own objects do the work: its
DiffusionDenoiser.noise_images noises the clean images (torch.randn_like substituted, so that the noise is a stored array), its
UNetDiffusion predicts the noise, and the objective of its training loop (DDIMModel.py:351-375, cddpmModels.py:367-374) is
evaluated on those tensors per sample, without autocast, with torch's own mse_loss / l1_loss / conv2d -- once in fp32 and once in
float64: schedule, noising and every expression of the objective in double, on the double of the fp32 prediction (the reference's
time embedding is float32 by construction, so its network has no float64 form; the objective's own arithmetic is what is judged).
Stored in denoising_loss_ref.npz: the inputs, t, eps, the schedule, x_t, the fp32 predictions and predicted clean images, and both
sets of per-sample scalars (mse, edge, loss)."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import midd_loader  # noqa: E402

midd_loader.load()
from midd_amd.config import UNetConfig  # noqa: E402
from midd_amd.weights import synthetic_xray  # noqa: E402
from tests.golden import save  # noqa: E402
from tests.golden.make_golden import SMALL, build  # noqa: E402
from tests.golden.ref_import import import_reference  # noqa: E402

WEIGHT_SEED, IMAGE_SEED, NOISE_KEY, SIZE = 42, 4321, 777, 64
T = (49, 7)
EDGE_WEIGHT = {"ddim": 0.2, "cddpm": 0.0}


def objective(model, den, clean, noisy, t, eps, variant, dtype, pred=None):
    """The training objective on explicit tensors in `dtype`, per sample -> (x_t, eps_pred, p, scalars [B, 3]).  `pred`: a prediction
    to judge in the place of the model's."""
    orig = torch.randn_like
    torch.randn_like = lambda x_, **kw: eps.to(dtype)
    try:
        x_t, noise = den.noise_images(clean.to(dtype), t)
    finally:
        torch.randn_like = orig
    kx = torch.tensor([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=dtype).view(1, 1, 3, 3)
    ky = kx.transpose(2, 3).contiguous()
    with torch.no_grad():
        pred = model(x_t, noisy.to(dtype), t) if pred is None else pred.to(dtype)
        e = torch.clamp(pred, -5, 5) if variant == "ddim" else pred
        ah = den.alpha_hat[t][:, None, None, None]
        p = torch.clamp((x_t - torch.sqrt(1 - ah) * e) / torch.sqrt(ah), 0, 1)
        rows = []
        for b in range(clean.shape[0]):
            mse = F.mse_loss(e[b:b + 1], noise[b:b + 1])
            mags = [torch.sqrt(F.conv2d(u[b:b + 1], kx, padding=1) ** 2 + F.conv2d(u[b:b + 1], ky, padding=1) ** 2 + 1e-8)
                    for u in (p, clean.to(dtype))]
            edge = F.l1_loss(mags[0], mags[1])
            rows.append([mse.item(), edge.item(), (mse + EDGE_WEIGHT[variant] * edge).item()])
    return x_t.numpy().copy(), pred.numpy().copy(), p.numpy().copy(), np.asarray(rows, np.float64)


def main():
    torch.set_num_threads(8)
    ref = import_reference()
    clean = torch.from_numpy(synthetic_xray(2, SIZE, SIZE, seed=IMAGE_SEED))
    g = np.random.Generator(np.random.Philox(key=NOISE_KEY))
    noisy = torch.from_numpy(np.clip(clean.numpy() + 0.1 * g.standard_normal(clean.shape, dtype=np.float32), 0, 1).astype(np.float32))
    eps = torch.from_numpy(g.standard_normal(clean.shape, dtype=np.float32))
    t = torch.tensor(T, dtype=torch.long)
    arrays = {"clean": clean.numpy(), "noisy": noisy.numpy(), "eps": eps.numpy(), "t": np.asarray(T, np.int64),
              "seed_weights": np.int64(WEIGHT_SEED), "seed_image": np.int64(IMAGE_SEED)}
    for variant in ("ddim", "cddpm"):
        refmod = getattr(ref, variant)
        model = build(refmod, UNetConfig(variant=variant, **SMALL), seed=WEIGHT_SEED, perturb=True)
        den = refmod.DiffusionDenoiser(model, noise_steps=50)
        den.alpha_hat = den.alpha_hat.cpu()
        x_t, pred, p, s32 = objective(model, den, clean, noisy, t, eps, variant, torch.float32)
        den.alpha_hat = den.alpha_hat.double()          # the fp32 table's values, the square roots in float64
        _, _, _, s64 = objective(model, den, clean, noisy, t, eps, variant, torch.float64, pred=torch.from_numpy(pred))
        rel = np.abs(s32 - s64) / np.abs(s64)
        print(f"{variant}: fp32 {s32.tolist()}\n   float64 {s64.tolist()}\n   relative distance {rel.tolist()}", flush=True)
        if variant == "ddim":
            arrays["alpha_hat"] = den.alpha_hat.float().numpy().copy()
            arrays["x_t"] = x_t
        else:
            assert np.array_equal(arrays["x_t"], x_t)      # the two variants noise alike
        arrays.update({f"eps_pred_{variant}": pred, f"p_{variant}": p, f"scalars32_{variant}": s32, f"scalars64_{variant}": s64})
    save("denoising_loss_ref", arrays)
    print("loss fixture done")


if __name__ == "__main__":
    main()
