"""Records what tests/test_oracle_vs_reference.py and the router test of tests/test_hybrid_cpu.py compare against, FROM THE
REFERENCE ITSELF, so that those tests need nothing outside the repository.  Build container only (needs the reference):

    PYTHONDONTWRITEBYTECODE=1 MPLBACKEND=Agg python tests/golden/make_golden_pins.py

Same recipe as make_golden.py (reference imported in-process by ref_import.py, weights from the package's portable
generator, formula-generated inputs).  Written:
  reference_pins.json        state-dict names and shapes of both reference UNets; the reference HybridDenoisingRouter's
                             state-dict layout (name, shape, dtype, parameter or buffer) for the side networks below
  reference_pins.npz         the reference's denoise() outputs of the two sampler pins, the router's beta
  forward_blocks_<variant>   every top-level block's output of one reference forward (tests/golden/__init__.py parts)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import midd_loader  # noqa: E402

midd_loader.load()
from midd_amd.config import UNetConfig  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402
from tests.golden import save  # noqa: E402
from tests.golden.make_golden import build, traced_forward  # noqa: E402
from tests.golden.ref_import import import_hybrid, import_reference  # noqa: E402

# the parameters tests/test_oracle_vs_reference.py and tests/test_hybrid_cpu.py use
SMALL = dict(model_channels=16, time_emb_dim=32)
NAF = dict(width=8, middle_blk_num=1, enc_blk_nums=[1, 1], dec_blk_nums=[1, 1])


def main():
    torch.set_num_threads(8)
    ref = import_reference()
    pins, arrays = {"state_dict": {}}, {}

    for variant in ("ddim", "cddpm"):
        sd = getattr(ref, variant).UNetDiffusion().state_dict()
        pins["state_dict"][variant] = [[k, list(v.shape)] for k, v in sd.items()]

        cfg = UNetConfig(variant=variant, **SMALL)
        model = build(getattr(ref, variant), cfg, seed=7, perturb=True)
        x = torch.from_numpy(synthetic_xray(2, 32, 40, seed=3, kind="uniform"))
        cond = torch.from_numpy(synthetic_xray(2, 32, 40, seed=5))
        out, cap = traced_forward(model, x, cond, torch.tensor([13, 13]))
        save(f"forward_blocks_{variant}", {**{f"layer/{k}": v for k, v in cap.items()}, "out": out})

    cfg = UNetConfig(**SMALL)
    den = ref.ddim.DiffusionDenoiser(build(ref.ddim, cfg, seed=11, perturb=True), noise_steps=50)
    noisy = torch.from_numpy(synthetic_xray(2, 32, 32, seed=21))
    arrays["ddim_out"] = den.denoise(noisy, inference_steps=8).numpy()
    arrays["ddim_noisy_after"] = noisy.numpy()                  # the input as the reference left it

    cfg = UNetConfig(variant="cddpm", **SMALL)
    den = ref.cddpm.DiffusionDenoiser(build(ref.cddpm, cfg, seed=12, perturb=True), noise_steps=50)
    noisy = torch.from_numpy(synthetic_xray(1, 32, 32, seed=22))
    torch.manual_seed(1234)
    arrays["cddpm_out"] = den.denoise(noisy, inference_steps=5).numpy()

    hyb = import_hybrid()
    router = hyb.HybridDenoisingRouter(NAF, {"noise_steps": 50}, inference_diffusion_steps=7)
    params = {k for k, _ in router.named_parameters()}
    pins["router"] = [[k, list(v.shape), str(v.dtype).replace("torch.", ""), k in params]
                      for k, v in router.state_dict().items()]
    arrays["router_beta"] = router.diffusion_wrapper.beta.cpu().numpy()

    with open(os.path.join(HERE, "reference_pins.json"), "w") as f:
        json.dump(pins, f, indent=0)
    np.savez_compressed(os.path.join(HERE, "reference_pins.npz"), **arrays)
    print("pins done")


if __name__ == "__main__":
    main()
