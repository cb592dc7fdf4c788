"""compute="f16" on the GPU, through the C ABI: one fp16 MFMA per product, judged against the FP32 reference values with the
yardstick of tests/f16_emulation.py -- the reference under an emulation of CUDA autocast lies E away from the fp32 reference
(E_max, E_rms); the mode must stay within max|d| <= 2 E_max and rms(d) <= 1.5 E_rms.  E comes from the
fixtures recorded from the reference (tests/golden/make_golden_f16.py) or, where no fixture exists, live from the oracle under
the same emulation (tests/test_f16_mode_cpu.py ties the two).  The 1e-3 parity gate of the other modes does not apply here and
is not touched.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, timestep_list, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import golden
from tests.f16_emulation import AutocastEmulation, distance, gate

pytestmark = pytest.mark.gpu

RANGE_KW = dict(model_channels=32, channel_mult=(1, 2), num_res_blocks=2, attention_resolutions=(1,), time_emb_dim=32)
SMALL_KW = dict(model_channels=16, time_emb_dim=64)


def _model(cfg_kw, sd_np, variant="ddim", compute="f16", batch_invariant=False):
    m = UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant, **cfg_kw)
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd_np.items()}, strict=True)
    return m.to("cuda").eval()


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def full_sd():
    return make_state_dict(UNetConfig(), seed=42)


@pytest.fixture(scope="module")
def full_f16(full_sd):
    return _model({}, full_sd)


def _oracle_yardstick(sd, cfg, fn):
    """fn(state dict, topology) evaluated in fp32 and under the autocast emulation -> (fp32 values, E_max, E_rms)."""
    sdt, topo = orc.to_torch(sd), topology(cfg)
    with torch.no_grad():
        want = fn(sdt, topo).numpy()
        with AutocastEmulation(True):
            emu = fn(sdt, topo).numpy()
    return (want,) + distance(emu, want)


# ------------------------------------------------------------------------------ 1. the reference fixtures
def test_case_a_ddim_64_final_and_per_iteration(full_f16, full_sd):
    """Full ddim network, B = 2, 64 x 64, 50 iterations: x after the sampler, and eps / x of iterations 0, 24 and 49 (eps of
    iteration k: one forward on the mode's own x before that iteration).  Also: the mode is not f16x3 under another name --
    its result differs from the f16x3 result, and its profile lists one-plane kernels only."""
    g = golden.load("f16_mode_ddim_64")
    noisy = torch.from_numpy(synthetic_xray(2, 64, 64, seed=int(g["seed_image"]))).cuda()
    den = DiffusionDenoiser(full_f16, noise_steps=50)
    steps = timestep_list(50, 50)
    assert list(g["steps"]) == list(steps)
    out = den.denoise(noisy, inference_steps=50)
    assert torch.equal(den.denoise(noisy, inference_steps=50), out), "same call twice: same bits"
    gate(_np(out), g["x_fp32"], float(g["x_E_max"]), float(g["x_E_rms"]), "case a, x after 50 iterations")
    for k in (0, 24, 49):
        run = lambda n: full_f16.run_sampler(noisy, steps[:n], den.beta, den.alpha, den.alpha_hat, clamp_eps=True) if n else noisy
        x_before, x_after = run(k), run(k + 1)
        eps = full_f16(x_before, noisy, torch.full((2,), steps[k], dtype=torch.long))
        gate(_np(eps), g[f"eps_it{k}_fp32"], float(g[f"eps_it{k}_E_max"]), float(g[f"eps_it{k}_E_rms"]), f"case a, eps of iteration {k}")
        gate(_np(x_after), g[f"x_it{k}_fp32"], float(g[f"x_it{k}_E_max"]), float(g[f"x_it{k}_E_rms"]), f"case a, x after iteration {k}")
    assert torch.equal(run(50), out)

    x3 = DiffusionDenoiser(_model({}, full_sd, compute="f16x3"), noise_steps=50).denoise(noisy, inference_steps=50)
    d3 = distance(_np(out), _np(x3))
    print(f"case a: max|f16 - f16x3| = {d3[0]:.3e}; f16x3 vs the fp32 reference {distance(_np(x3), g['x_fp32'])[0]:.3e}")
    assert d3[0] > 0 and distance(_np(x3), g["x_fp32"])[0] < 1e-3

    full_f16.profile_begin()
    full_f16(noisy, noisy, torch.full((2,), 7, dtype=torch.long))
    prof = full_f16.profile_end()
    names = {p["name"].split("<")[0] for p in prof}
    print(sorted(names), sum(p["launches"] for p in prof), "launches")
    assert names == {"midd::in_conv1_kernel", "midd::conv_mfma_f16_kernel", "midd::conv1x1_f16_kernel", "midd::attention_f16_kernel",
                     "midd::resize_bilinear_kernel", "midd::out_conv_kernel"}
    assert sum(p["launches"] for p in prof) == 73


def test_case_b_cddpm_64_with_recorded_noise(full_sd):
    """Full cddpm network (its own module lists), B = 2, 64 x 64, 50 stochastic iterations replayed with the fixture's noise."""
    g = golden.load("f16_mode_cddpm_64")
    cfg = UNetConfig(variant="cddpm")
    model = _model({}, make_state_dict(cfg, seed=int(g["seed_weights"])), variant="cddpm")
    noisy = torch.from_numpy(synthetic_xray(2, 64, 64, seed=int(g["seed_image"]))).cuda()
    noise = torch.from_numpy(np.stack([g[f"step_noise_{i:02d}"] for i in range(50)])).cuda()
    out = DiffusionDenoiser(model, noise_steps=50).denoise(noisy, inference_steps=50, step_noise=noise)
    gate(_np(out), g["x_fp32"], float(g["x_E_max"]), float(g["x_E_rms"]), "case b, cddpm x after 50 iterations")


def test_case_c_ddim_128(full_f16):
    g = golden.load("f16_mode_ddim_128")
    noisy = torch.from_numpy(synthetic_xray(2, 128, 128, seed=int(g["seed_image"]))).cuda()
    out = DiffusionDenoiser(full_f16, noise_steps=50).denoise(noisy, inference_steps=50)
    gate(_np(out), g["x_fp32"], float(g["x_E_max"]), float(g["x_E_rms"]), "case c, 128 x 128, x after 50 iterations")


# ------------------------------------------------------------------------------ 2. single forwards, ragged shapes
@pytest.mark.parametrize("shape", [(256, 256), (200, 184), (40, 104)])
def test_forward_b8_vs_oracle(full_f16, full_sd, shape):
    """One forward of the default network at B = 8: 256 x 256 (the headline shape), 200 x 184 and 40 x 104 (ragged tiles at every
    level, N = H W / 64 keys not a multiple of 64).  fp32 values and E from the oracle, live, on rows 0 and 7 (CPU time)."""
    H, W = shape
    x = torch.from_numpy(synthetic_xray(8, H, W, seed=31, kind="uniform"))
    c = torch.from_numpy(synthetic_xray(8, H, W, seed=32))
    t = torch.tensor([49, 3, 17, 0, 25, 40, 9, 33])
    rows = [0, 7]
    want, e_max, e_rms = _oracle_yardstick(full_sd, UNetConfig(), lambda sdt, topo: orc.unet_forward(sdt, topo, x[rows], c[rows], t[rows]))
    got = full_f16(x.cuda(), c.cuda(), t.cuda())
    assert torch.isfinite(got).all()
    gate(_np(got)[rows], want, e_max, e_rms, f"forward B=8 {H}x{W}, rows 0 and 7 (max|eps| {np.abs(want).max():.2f})")
    one = full_f16(x[7:8].cuda(), c[7:8].cuda(), t[7:8].cuda())                  # the same sample in a batch of one: other tiles
    gate(_np(one), want[1:2], e_max, e_rms, f"forward B=1 {H}x{W}")


# ------------------------------------------------------------------------------ 3. small topologies
@pytest.mark.parametrize("kw,variant,shape", [(SMALL_KW, "ddim", (2, 32, 48)), (RANGE_KW, "ddim", (3, 104, 96)), (RANGE_KW, "cddpm", (4, 40, 56))])
def test_small_topologies_forward_and_sampler_vs_oracle(kw, variant, shape):
    """model_channels 16 and 32 (16 / 32 / 64-channel layers: the nt = 1, 2 tiles, two-wave workgroups, D = 32 attention) and the
    cddpm module lists: forward and a 6-iteration sampler (even batches >= 4 run as two sub-batch programs)."""
    B, H, W = shape
    cfg = UNetConfig(variant=variant, **kw)
    sd = make_state_dict(cfg, seed=77, perturb_norm=True)
    model = _model(kw, sd, variant=variant)
    x = torch.from_numpy(synthetic_xray(B, H, W, seed=1, kind="uniform"))
    c = torch.from_numpy(synthetic_xray(B, H, W, seed=2))
    t = torch.tensor([3, 40, 11, 27][:B])
    want, e_max, e_rms = _oracle_yardstick(sd, cfg, lambda sdt, topo: orc.unet_forward(sdt, topo, x, c, t))
    gate(_np(model(x.cuda(), c.cuda(), t.cuda())), want, e_max, e_rms, f"{variant} mc={kw['model_channels']} forward {shape}")
    if variant == "ddim":
        want, e_max, e_rms = _oracle_yardstick(sd, cfg, lambda sdt, topo: orc.denoise(sdt, topo, c, noise_steps=50, inference_steps=6))
        out = DiffusionDenoiser(model, noise_steps=50).denoise(c.cuda(), inference_steps=6)
        gate(_np(out), want, e_max, e_rms, f"{variant} mc={kw['model_channels']} sampler, 6 iterations {shape}")


# ------------------------------------------------------------------------------ 4. determinism, split, batch invariance
def test_split_and_unsplit_runs_agree_and_repeat(full_f16):
    """B = 4 runs as two sub-batch programs on two streams by default and as one program with MI_NO_SPLIT (other tiles, wide
    chunks): each inside the gate of the fixture, their difference inside it too, and each repeatable to the bit."""
    g = golden.load("f16_mode_ddim_64")
    two = synthetic_xray(2, 64, 64, seed=int(g["seed_image"]))
    noisy = torch.from_numpy(np.concatenate([two, two])).cuda()
    den = DiffusionDenoiser(full_f16, noise_steps=50)
    steps = timestep_list(50, 50)
    e_max, e_rms = float(g["x_E_max"]), float(g["x_E_rms"])
    split = full_f16.run_sampler(noisy, steps, den.beta, den.alpha, den.alpha_hat, clamp_eps=True)
    alone = full_f16.run_sampler(noisy, steps, den.beta, den.alpha, den.alpha_hat, clamp_eps=True, no_split=True)
    assert torch.equal(full_f16.run_sampler(noisy, steps, den.beta, den.alpha, den.alpha_hat, clamp_eps=True), split)
    assert torch.equal(full_f16.run_sampler(noisy, steps, den.beta, den.alpha, den.alpha_hat, clamp_eps=True, no_split=True), alone)
    assert torch.equal(split[:2], split[2:]), "same images, same per-program batch: same bits in either sub-batch"
    want = np.concatenate([g["x_fp32"], g["x_fp32"]])
    gate(_np(split), want, e_max, e_rms, "two sub-batch programs")
    gate(_np(alone), want, e_max, e_rms, "MI_NO_SPLIT")
    gate(_np(split), _np(alone), e_max, e_rms, "split vs MI_NO_SPLIT")


def test_batch_invariant_f16_is_bit_exact_across_batch_sizes(full_sd):
    """As tests/test_gpu_parity_r2.py::test_batch_invariant_mode_is_bit_exact_across_batch_sizes for the other modes."""
    m = _model({}, full_sd, batch_invariant=True)
    den = DiffusionDenoiser(m)
    for S, iters in ((64, 6), (256, 3)):
        x = torch.from_numpy(synthetic_xray(8, S, S, seed=77)).cuda()
        full = den.denoise(x, inference_steps=iters)
        for lo, hi in ((0, 1), (2, 5), (4, 8)):                       # batches of 1, 3 and 4 against the batch of 8
            part = den.denoise(x[lo:hi].contiguous(), inference_steps=iters)
            assert torch.equal(part, full[lo:hi]), f"{S}x{S}: rows {lo}:{hi} differ from the batch of 8 (max {(part - full[lo:hi]).abs().max().item():.3e})"
        t = torch.full((8,), 11, dtype=torch.long, device="cuda")
        e8 = m(x, x, t)
        assert torch.equal(m(x[2:3].contiguous(), x[2:3].contiguous(), t[2:3]), e8[2:3])
        assert torch.equal(m(x[3:6].contiguous(), x[3:6].contiguous(), t[3:6]), e8[3:6])
    g = golden.load("f16_mode_ddim_64")
    out = den.denoise(torch.from_numpy(synthetic_xray(2, 64, 64, seed=int(g["seed_image"]))).cuda(), inference_steps=50)
    gate(_np(out), g["x_fp32"], float(g["x_E_max"]), float(g["x_E_rms"]), "batch-invariant plan, case a")


# ------------------------------------------------------------------------------ 5. operand range
@pytest.mark.parametrize("gain", [1e-3, 3.0])
def test_attention_operand_range_in_range_passes_the_gate(gain):
    """The construction of tests/test_gpu_parity_r3.py::test_attention_operand_range_vs_oracle: the qkv projection scaled by
    `gain` (scores x gain^2, v x gain), one forward against the oracle with the live yardstick."""
    cfg = UNetConfig(**RANGE_KW)
    sd = make_state_dict(cfg, seed=78, perturb_norm=True)
    for k in sd:
        if ".qkv." in k:
            sd[k] = (sd[k] * gain).astype(np.float32)
    x = torch.from_numpy(synthetic_xray(2, 32, 32, seed=3, kind="uniform"))
    c = torch.from_numpy(synthetic_xray(2, 32, 32, seed=4))
    t = torch.tensor([11, 45])
    want, e_max, e_rms = _oracle_yardstick(sd, cfg, lambda sdt, topo: orc.unet_forward(sdt, topo, x, c, t))
    eps = _model(RANGE_KW, sd)(x.cuda(), c.cuda(), t.cuda())
    gate(_np(eps), want, e_max, e_rms, f"attention qkv gain {gain:g}")


def test_attention_operand_beyond_fp16_is_an_error_in_f16_mode():
    """Same rule as f16x3 (tests/test_gpu_parity_r3.py::test_attention_operand_beyond_fp16_is_an_error): q, k, v enter the
    attention as fp16(16 x value); |value| >= 4094 is reported through the status word, never returned as an image."""
    cfg = UNetConfig(**RANGE_KW)
    sd = make_state_dict(cfg, seed=78, perturb_norm=True)
    for k in sd:
        if ".qkv.bias" in k:
            sd[k] = (sd[k] + 6000.0).astype(np.float32)
    m = _model(RANGE_KW, sd)
    x = torch.from_numpy(synthetic_xray(2, 32, 32, seed=3, kind="uniform")).cuda()
    c = torch.from_numpy(synthetic_xray(2, 32, 32, seed=4)).cuda()
    with pytest.raises(native.MiddError) as ei:
        m(x, c, torch.tensor([11, 45]))
    assert ei.value.code == -5 and "range" in str(ei.value)
    with pytest.raises(native.MiddError):
        DiffusionDenoiser(m).denoise(c, inference_steps=2)


# ------------------------------------------------------------------------------ 7. a caller that forwards the argument
def test_hybrid_router_forwards_compute_f16(full_sd):
    """HybridDenoisingRouter(compute="f16") on the inputs of the hybrid_ddim_64 fixture: the diffusion branch alone
    (hq_denoised: sampler, then nan_to_num + clamp) against the oracle's sampler, yardstick live from the emulated oracle."""
    import os
    import torch.nn as nn
    from midd_amd.hybrid import HybridDenoisingRouter
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "hybrid_ddim_64.npz"))
    side = lambda cin: nn.Conv2d(cin, 1, 1)
    model = HybridDenoisingRouter(side(1), side(1), side(3), diffusion_params={"noise_steps": 50}, inference_diffusion_steps=8, compute="f16")
    assert model.diffusion_unet.compute == "f16"
    model.diffusion_unet.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in full_sd.items()}, strict=True)
    model = model.to("cuda").eval()
    noisy = torch.from_numpy(synthetic_xray(2, 64, 64, seed=int(g["seed_image"])))
    hq = model.hq_denoised(noisy.cuda())
    want, e_max, e_rms = _oracle_yardstick(full_sd, UNetConfig(), lambda sdt, topo: orc.denoise(sdt, topo, noisy, noise_steps=50, inference_steps=8))
    d32 = distance(want, g["hq_8"])[0]
    print(f"oracle fp32 vs the fixture's hq_8: {d32:.2e}")
    assert d32 < 1e-4
    gate(_np(hq), want, e_max, e_rms, "hybrid router, hq branch, inference_steps=8")
