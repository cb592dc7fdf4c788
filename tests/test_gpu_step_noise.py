"""GPU: the seeded, device-side step noise of the cddpm sampler (include/midd.h: mi_denoise_seeded, mi_step_noise_fill).

The generator is a specification (Philox4x32-10 + Box-Muller, tests/step_noise_reference.py restates it in float64), so its
values are checked against that restatement, its distribution against the normal law, and the fused draw inside the sampler
update against the replay of the same values through the existing `step_noise` argument -- bit for bit, in every topology of
the call (two programs on two streams, one program, one image, MI_NO_SPLIT) and every arithmetic mode."""
import math

import numpy as np
import pytest
import torch
from PIL import Image

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, timestep_list, topology
from midd_amd.cli import denoise_image_diffusion
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import step_noise_reference as ref

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # north_star: |delta| < 1e-3 fp32 per pixel (tests/test_gpu_parity.py)
SEED = 0x1234567890ABCDEF
K = 5                     # inference_steps of the sampler cases


@pytest.fixture(scope="module")
def cddpm_sd():
    return make_state_dict(UNetConfig(variant="cddpm"), seed=42)


_models = {}


def _model(sd, compute="f16x3", batch_invariant=False):
    key = (compute, batch_invariant)
    if key not in _models:
        m = UNetDiffusion(variant="cddpm", compute=compute, batch_invariant=batch_invariant)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models[key]


def _images(B, S=64, seed=77):
    return torch.from_numpy(synthetic_xray(B, S, S, seed=seed)).cuda()


# ------------------------------------------------------------------------------ 1. values
def test_values_match_the_float64_specification():
    """fp32 chain on the device: log, sqrt, cospif and two multiplies, each within ~2 ulp: under 10 ulp relative at
    |z| <= 5.77, i.e. 3.4e-6 on z and half that on the 0.5-scaled value; the bound is 1e-5."""
    shape = (3, 2, 37, 53)
    got = midd_amd.step_noise(SEED, 3, shape, sample_offset=5)
    assert got.shape == (3,) + shape and got.dtype == torch.float32 and got.is_cuda
    want = ref.step_noise(SEED, 3, shape, sample_offset=5)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"step noise vs float64 specification: max|delta| = {err:.3e}")
    assert err <= 1e-5
    # the offset IS the sample index: rows 2.. of offset 3 are rows 0.. of offset 5
    shifted = midd_amd.step_noise(SEED, 3, shape, sample_offset=3)
    assert torch.equal(shifted[:, 2], got[:, 0])


# ------------------------------------------------------------------------------ 2. distribution
def test_distribution_and_independence():
    n = 1 << 22
    shape = (2, 1, 2048, 2048)
    a = midd_amd.step_noise(SEED, 9, shape, sample_offset=3)
    z = 2.0 * a[7, 0].reshape(-1).double()                      # sample 3, iteration 7
    z_sample = 2.0 * a[7, 1].reshape(-1).double()               # sample 4
    z_iter = 2.0 * a[8, 0].reshape(-1).double()                 # iteration 8
    del a
    z_seed = 2.0 * midd_amd.step_noise(SEED ^ 1, 8, (1, 1, 2048, 2048), sample_offset=3)[7, 0].reshape(-1).double()
    assert z.numel() == n
    mean = float(z.mean())
    c = z - mean
    var = float((c * c).mean())
    kurt = float((c ** 4).mean()) / var ** 2
    s_mean, s_var, s_kurt = abs(mean) * math.sqrt(n), abs(var - 1) * math.sqrt(n / 2), abs(kurt - 3) * math.sqrt(n / 24)
    srt = torch.sort(z).values
    cdf = 0.5 * (1.0 + torch.special.erf(srt / math.sqrt(2.0)))
    i = torch.arange(1, n + 1, device=z.device, dtype=torch.float64)
    ks = float(torch.maximum((i / n - cdf).max(), (cdf - (i - 1) / n).max())) * math.sqrt(n)
    corr = {"element": float((z[:-1] * z[1:]).mean()) * math.sqrt(n), "sample": float((z * z_sample).mean()) * math.sqrt(n),
            "iteration": float((z * z_iter).mean()) * math.sqrt(n), "seed bit": float((z * z_seed).mean()) * math.sqrt(n)}
    print(f"scaled mean {s_mean:.2f} var {s_var:.2f} kurtosis {s_kurt:.2f} KS {ks:.2f} correlations "
          + " ".join(f"{k} {v:.2f}" for k, v in corr.items()) + f" max|z| {float(z.abs().max()):.3f}")
    assert s_mean < 4.5 and s_var < 4.5 and s_kurt < 4.5
    assert ks < 1.95
    for k, v in corr.items():
        assert abs(v) < 4.5, (k, v)
    assert float(z.abs().max()) <= 5.77


# ------------------------------------------------------------------------------ 3. the fused draw == the replayed tensor
@pytest.mark.parametrize("compute,B", [("f16x3", 8), ("f16x3", 3), ("f16x3", 1), ("f32", 8), ("f32", 3), ("f32", 1), ("f16", 8)])
def test_seeded_run_equals_its_replay_bit_for_bit(cddpm_sd, compute, B):
    """B = 8: two programs of 4 on two streams (the second one's samples start at global index 4); 3: one program; 1."""
    den = _model(cddpm_sd, compute)
    x = _images(B)
    n_iters = len(timestep_list(50, K))
    seeded = den.denoise(x, inference_steps=K, seed=SEED)
    replay = den.denoise(x, inference_steps=K, step_noise=midd_amd.step_noise(SEED, n_iters, x.shape))
    assert torch.isfinite(seeded).all() and torch.equal(seeded, replay)


def test_seeded_run_equals_its_replay_without_the_split(cddpm_sd):
    den = _model(cddpm_sd)
    x = _images(8)
    steps = timestep_list(50, K)
    args = (x, steps, den.beta, den.alpha, den.alpha_hat)
    seeded = den.model.run_sampler(*args, clamp_eps=False, no_split=True, seed=SEED)
    replay = den.model.run_sampler(*args, clamp_eps=False, no_split=True, step_noise=midd_amd.step_noise(SEED, len(steps), x.shape))
    assert torch.equal(seeded, replay)


# ------------------------------------------------------------------------------ 4. against the oracle
def test_seeded_run_matches_the_oracle_given_the_same_noise(cddpm_sd):
    cfg = UNetConfig(variant="cddpm")
    den = _model(cddpm_sd)
    x = _images(3)
    noise = midd_amd.step_noise(SEED, len(timestep_list(50, K)), x.shape)
    got = den.denoise(x, inference_steps=K, seed=SEED)
    want = orc.denoise(orc.to_torch(cddpm_sd), topology(cfg), x.cpu(), 50, K, step_noise=list(noise.cpu()))
    err = float((got.cpu() - want).abs().max())
    print(f"seeded cddpm vs oracle with the exported noise: max|delta| = {err:.3e}")
    assert err < TOL_FINAL


# ------------------------------------------------------------------------------ 5. shard invariance
def test_a_block_of_the_batch_with_its_offset_equals_the_block_of_the_whole(cddpm_sd):
    den = _model(cddpm_sd, batch_invariant=True)
    x = _images(8)
    whole = den.denoise(x, inference_steps=K, seed=SEED)
    block = den.denoise(x[2:6], inference_steps=K, seed=SEED, sample_offset=2)
    assert torch.equal(whole[2:6], block)
    assert not torch.equal(whole[2:6], den.denoise(x[2:6], inference_steps=K, seed=SEED))      # offset 0: other samples' noise


# ------------------------------------------------------------------------------ 6. reproducibility
def test_same_seed_same_bits_other_seed_other_bits(cddpm_sd):
    den = _model(cddpm_sd)
    x = _images(8)
    first = den.denoise(x, inference_steps=K, seed=SEED)
    assert torch.equal(den.denoise(x, inference_steps=K, seed=SEED), first)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = den.denoise(x, inference_steps=K, seed=SEED)
    side.synchronize()
    assert torch.equal(on_side, first)
    assert not torch.equal(den.denoise(x, inference_steps=K, seed=SEED + 1), first)
    # nothing is drawn at t == 0: a seeded call over t_list = [0] is the unseeded one
    args = (x, [0], den.beta, den.alpha, den.alpha_hat)
    assert torch.equal(den.model.run_sampler(*args, clamp_eps=False, seed=SEED), den.model.run_sampler(*args, clamp_eps=False))


def test_ddim_ignores_the_seed():
    kw = dict(model_channels=16, time_emb_dim=64)
    m = UNetDiffusion(**kw)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state_dict(UNetConfig(**kw), seed=5).items()})
    den = DiffusionDenoiser(m.cuda().eval(), noise_steps=50)
    x = _images(2, 32)
    assert torch.equal(den.denoise(x, inference_steps=3, seed=SEED), den.denoise(x, inference_steps=3))


# ------------------------------------------------------------------------------ 7. memory
def test_seeded_call_allocates_no_noise_tensor(cddpm_sd):
    den = _model(cddpm_sd)
    B, S, steps = 8, 256, 50
    assert len(timestep_list(50, steps)) == 50
    noise_bytes = 50 * B * S * S * 4
    x = _images(B, S)
    den.denoise(x, inference_steps=steps, seed=SEED)           # warm-up: the workspace is cached per shape and stream
    torch.cuda.synchronize()

    def rise(**kw):
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = den.denoise(x, inference_steps=steps, **kw)
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated() - base

    seeded, default = rise(seed=SEED), rise()
    print(f"peak rise across one call: seeded {seeded / 1e6:.1f} MB, default {default / 1e6:.1f} MB (noise tensor {noise_bytes / 1e6:.1f} MB)")
    assert seeded < noise_bytes
    assert default >= noise_bytes


# ------------------------------------------------------------------------------ 8. CLI
def test_cli_seed_gives_the_same_png_pixels_twice(tmp_path, cddpm_sd):
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in cddpm_sd.items()}, "noise_steps": 50}, ckpt)
    png = tmp_path / "in.png"
    Image.fromarray((synthetic_xray(1, 88, 120, seed=9)[0, 0].clip(0, 1) * 255).astype(np.uint8), mode="L").save(png)
    outs = []
    for seed in (7, 7, 8):
        img = denoise_image_diffusion(str(ckpt), str(png), device_type="cuda", img_size=64, inference_steps=K, variant="cddpm", seed=seed)
        out = tmp_path / f"out{len(outs)}.png"
        img.save(out)
        outs.append(np.asarray(Image.open(out)))
    assert outs[0].shape == (88, 120) and np.array_equal(outs[0], outs[1])
    assert not np.array_equal(outs[0], outs[2])
