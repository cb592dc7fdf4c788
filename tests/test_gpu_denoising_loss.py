"""GPU: the training objective as an evaluation (include/midd.h: THE FORWARD NOISE, THE NOISING, THE DENOISING LOSS).

The kernels alone, against tests/denoising_loss_reference.py bit for bit on shapes that take every path (partial patches, a plane
smaller than a patch, several channels, the 16-byte and the scalar path, tensors 4 bytes off a 16-byte boundary), then the chained
call through the network: equal to its pieces bit for bit, inside the bounds that the project's parity gate on eps implies against
the CPU oracle's forward, and independent of what shares the batch or the pass."""
import ctypes as C
import inspect
import json
import math
import re

import numpy as np
import pytest
import torch
from PIL import Image

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, topology
from midd_amd.cli import denoise_image_diffusion
from midd_amd.weights import make_state_dict, synthetic_xray
from midd_amd import image16
from oracle import ddim_oracle as orc
from tests import denoising_loss_reference as ref
from tests import test_gpu_step_noise as step_noise_tests

pytestmark = pytest.mark.gpu

SEED = 0xFEEDFACE12345678
SMALL = dict(model_channels=16, time_emb_dim=64)
DELTA = 1e-3              # the project's parity gate on eps (tests/test_gpu_parity.py: TOL_FINAL)
# the bound of the step-noise test on the same generator, read off that test so that the two cannot drift apart; applied to z itself
Z_BOUND = float(re.search(r"assert err <= ([0-9.eE+-]+)", inspect.getsource(step_noise_tests.test_values_match_the_float64_specification)).group(1))
assert Z_BOUND == 1e-5
ALPHA_HAT = orc.schedule(50)[2]
AH = ALPHA_HAT.numpy()


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _inputs(shape, seed):
    """clean in [0, 1] with flat regions (both edge magnitudes are sqrt(1e-8) there: the constant decides); eps_pred seeded, a good
    part of it beyond +-5 (the clamp matters, and p reaches both ends of [0, 1])."""
    rng = np.random.default_rng(seed)
    B, Cc, H, W = shape
    clean = rng.random(shape, dtype=np.float32)
    clean[..., : max(3, H // 2), : max(3, W // 3)] = 0.25
    clean[..., H - max(1, H // 4):, :] = 1.0
    pred = (3.0 * rng.standard_normal(shape)).astype(np.float32)
    assert np.count_nonzero(np.abs(pred) > 5) > 0
    return torch.from_numpy(clean).cuda(), torch.from_numpy(pred).cuda()


def _shifted(t):
    """The same values 4 bytes further from a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


CASES = [((2, 1, 37, 45), (13, 40)),           # partial patches on both axes, odd pitch, scalar path (37 * 45 is odd)
         ((1, 1, 8, 8), (25,)),                # smaller than a patch: every pixel next to the zero padding or one step from it
         ((1, 3, 32, 64), (3,)),               # channels are independent; 16-byte path
         ((3, 1, 64, 64), (0, 49, 7))]         # three timesteps, both ends of the schedule


# ------------------------------------------------------------------------------ 1. the kernels alone
@pytest.mark.parametrize("shape,t", CASES)
@pytest.mark.parametrize("clamp", [True, False])
def test_kernels_equal_the_restatement_bit_for_bit(shape, t, clamp):
    clean, pred = _inputs(shape, seed=sum(shape))
    kw = dict(seed=SEED, sample_offset=2, draw=3)
    x_t, eps = midd_amd.noise_images(clean, t, ALPHA_HAT, **kw)
    torch.cuda.synchronize()
    # the drawn values against the float64 specification: the step-noise test's bound, on z (there is no 0.5 factor here)
    z64 = ref.forward_noise(SEED, shape, sample_offset=2, draw=3)
    err = float(np.abs(eps.cpu().numpy().astype(np.float64) - z64).max())
    print(f"forward noise vs float64 specification: max|delta z| = {err:.3e}")
    assert err <= Z_BOUND
    # the noising, given that eps
    want_xt = ref.noise_images(clean.cpu().numpy(), eps.cpu().numpy(), t, AH)
    assert _same(x_t, want_xt)
    x_t2, eps2 = midd_amd.noise_images(clean, t, ALPHA_HAT, noise=eps)
    assert _same(x_t2, x_t) and eps2.data_ptr() == eps.data_ptr()
    # the loss: explicit form == restatement == seeded form
    want_out, (q, g, p) = ref.loss_terms(clean.cpu().numpy(), want_xt, eps.cpu().numpy(), pred.cpu().numpy(), t, AH, clamp, 0.2)
    out, maps = midd_amd.loss_terms(clean, pred, t, ALPHA_HAT, x_t=x_t, noise=eps, clamp_eps=clamp, edge_weight=0.2, return_maps=True)
    assert out.dtype == torch.float64 and out.shape == (shape[0], 3) and _same(out, want_out), (out.cpu().numpy(), want_out)
    assert _same(maps[0], q) and _same(maps[1], g) and _same(maps[2], p)
    assert (ref._sobel_magnitude(clean.cpu().numpy()) == np.sqrt(np.float32(1e-8))).any()      # flat regions: the constant decides
    assert (g > 1e-2).any() and (p == 0).any() and (p == 1).any()
    s_out, s_maps = midd_amd.loss_terms(clean, pred, t, ALPHA_HAT, clamp_eps=clamp, edge_weight=0.2, return_maps=True, **kw)
    assert _same(s_out, out) and _same(s_maps, maps)
    # again, and without the maps
    again, none = midd_amd.loss_terms(clean, pred, t, ALPHA_HAT, clamp_eps=clamp, edge_weight=0.2, **kw)
    assert none is None and _same(again, out)
    assert _same(midd_amd.loss_terms(clean, pred, t, ALPHA_HAT, x_t=x_t, noise=eps, clamp_eps=clamp, edge_weight=0.2)[0], out)
    assert _same(midd_amd.noise_images(clean, t, ALPHA_HAT, **kw)[0], x_t)


def _native_noise(clean, t, x_t, eps_in=None, eps_out=None, seeded=True):
    B, Cc, H, W = clean.shape
    tt = (C.c_int32 * B)(*t)
    native.check(native.lib().mi_noise_images(clean.data_ptr(), tt, AH.ctypes.data_as(C.POINTER(C.c_float)), 50,
                                              None if eps_in is None else eps_in.data_ptr(), 1 if seeded else 0, C.c_uint64(SEED), 2, 3, None, None,
                                              x_t.data_ptr(), None if eps_out is None else eps_out.data_ptr(), B, Cc, H, W,
                                              torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("shape,t", CASES)
def test_tensors_four_bytes_off_give_the_same_bits(shape, t):
    clean, pred = _inputs(shape, seed=sum(shape))
    kw = dict(seed=SEED, sample_offset=2, draw=3)
    x_t, eps = midd_amd.noise_images(clean, t, ALPHA_HAT, **kw)
    out, maps = midd_amd.loss_terms(clean, pred, t, ALPHA_HAT, x_t=x_t, noise=eps, return_maps=True)
    # every tensor shifted alike: 16-byte body with a scalar head and tail per sample
    c4, x4, e4 = _shifted(clean), _shifted(torch.zeros_like(x_t)), _shifted(torch.zeros_like(eps))
    _native_noise(c4, t, x4, eps_out=e4)
    assert _same(x4, x_t) and _same(e4, eps)
    x4b = _shifted(torch.zeros_like(x_t))
    _native_noise(c4, t, x4b, eps_in=e4, seeded=False)
    assert _same(x4b, x_t)
    # only the input shifted: no common boundary, element by element
    assert _same(midd_amd.noise_images(c4, t, ALPHA_HAT, **kw)[0], x_t)
    assert _same(midd_amd.noise_images(c4, t, ALPHA_HAT, noise=eps)[0], x_t)
    o4, m4 = midd_amd.loss_terms(c4, _shifted(pred), t, ALPHA_HAT, x_t=x4, noise=e4, return_maps=True)
    assert _same(o4, out) and _same(m4, maps)
    assert _same(midd_amd.loss_terms(c4, _shifted(pred), t, ALPHA_HAT, **kw)[0], out)


def test_per_sample_counter_words_select_rows_of_the_whole():
    shape, t = (4, 1, 16, 24), (5, 6, 7, 8)
    clean, _ = _inputs(shape, seed=1)
    whole = midd_amd.noise_images(clean, t, ALPHA_HAT, seed=SEED, draw=9)[1]
    pick = midd_amd.noise_images(clean[[3, 1]], (8, 6), ALPHA_HAT, seed=SEED, sample_index=[3, 1], draws=[9, 9])[1]
    assert _same(pick, whole[[3, 1]])
    assert _same(midd_amd.noise_images(clean[3:], (8,), ALPHA_HAT, seed=SEED, sample_offset=3, draw=9)[1], whole[3:])
    other = midd_amd.noise_images(clean, t, ALPHA_HAT, seed=SEED, draw=10)[1]
    assert not (other == whole).any()
    step = 2.0 * midd_amd.step_noise(SEED, 1, shape)[0]
    assert not (midd_amd.noise_images(clean, t, ALPHA_HAT, seed=SEED)[1] == step).any()


# ------------------------------------------------------------------------------ 2. through the network
_cache = {}


def _sd(variant):
    if ("sd", variant) not in _cache:
        _cache["sd", variant] = make_state_dict(UNetConfig(variant=variant, **SMALL), seed=42, perturb_norm=True)
    return _cache["sd", variant]


def _den(variant, compute, batch_invariant=False):
    key = (variant, compute, batch_invariant)
    if key not in _cache:
        m = UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant, **SMALL)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd(variant).items()}, strict=True)
        _cache[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _cache[key]


def _pair(B, S=64):
    clean = synthetic_xray(B, S, S, seed=77)
    rng = np.random.default_rng(5)
    noisy = np.clip(clean + 0.1 * rng.standard_normal(clean.shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(clean).cuda(), torch.from_numpy(noisy).cuda()


T2 = (49, 7)


def _oracle_loss(variant, clean, noisy, x_t, eps):
    """The restated loss over the CPU oracle's forward of the same x_t, once per variant."""
    if ("oracle", variant) not in _cache:
        with torch.no_grad():
            pred = orc.unet_forward(orc.to_torch(_sd(variant)), topology(UNetConfig(variant=variant, **SMALL)), x_t.cpu(), noisy.cpu(),
                                    torch.tensor(T2, dtype=torch.long))
        out, _ = ref.loss_terms(clean.cpu().numpy(), x_t.cpu().numpy(), eps.cpu().numpy(), pred.numpy(), T2, AH, variant == "ddim",
                                0.2 if variant == "ddim" else 0.0)
        _cache["oracle", variant] = (x_t.cpu().numpy().copy(), out)
    return _cache["oracle", variant]


@pytest.mark.parametrize("compute", ["f16x3", "f32"])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_denoising_loss_equals_its_pieces_and_meets_the_oracle(variant, compute):
    den = _den(variant, compute)
    clean, noisy = _pair(2)
    res = den.denoising_loss(clean, noisy, T2, seed=SEED, return_maps=True)
    assert res.seed == SEED and res.t.tolist() == list(T2) and res.loss.dtype == torch.float64 and res.loss.shape == (2,)
    # the pieces one after another
    x_t, eps = den.noise_images(clean, T2, seed=SEED)
    pred = den.model(x_t, noisy, torch.tensor(T2))
    clamp, weight = variant == "ddim", 0.2 if variant == "ddim" else 0.0
    out, maps = midd_amd.loss_terms(clean, pred, T2, den.alpha_hat, x_t=x_t, noise=eps, clamp_eps=clamp, edge_weight=weight, return_maps=True)
    assert _same(res.mse, out[:, 0]) and _same(res.edge, out[:, 1]) and _same(res.loss, out[:, 2])
    assert _same(res.maps.q, maps[0]) and _same(res.maps.g, maps[1]) and _same(res.maps.p, maps[2])
    assert _same(midd_amd.loss_terms(clean, pred, T2, den.alpha_hat, seed=SEED, clamp_eps=clamp, edge_weight=weight)[0], out)
    if variant == "cddpm":
        assert _same(res.loss, res.mse)                   # its objective is the plain MSE; the edge term is still reported
        assert float(res.edge.min()) > 0
    # the same scalars without the maps, and with the caller's noise tensor
    plain = den.denoising_loss(clean, noisy, T2, seed=SEED)
    assert plain.maps is None and _same(plain.loss, res.loss) and _same(plain.mse, res.mse) and _same(plain.edge, res.edge)
    given = den.denoising_loss(clean, noisy, T2, noise=eps)
    assert given.seed is None and _same(given.loss, res.loss) and _same(given.edge, res.edge)
    # against the restated loss over the oracle's forward: |d eps| <= DELTA per pixel gives
    #   |d mse| <= 2 DELTA sqrt(mse) + DELTA^2        (Cauchy-Schwarz on the mean of (d + e)^2 - d^2)
    #   |d edge| <= 8 sqrt(2) (s / a) DELTA           (|dp| <= (s / a) DELTA; each Sobel kernel's weights sum to 8 in absolute value;
    #                                                  the magnitude of (ex, ey) and both clamps are 1-Lipschitz)
    xt_then, want = _oracle_loss(variant, clean, noisy, x_t, eps)
    assert np.array_equal(xt_then, x_t.cpu().numpy())
    a, s = ref.coefficients(T2, AH)
    got = out.cpu().numpy()
    for b in range(2):
        bound_mse = 2 * DELTA * math.sqrt(want[b, 0]) + DELTA ** 2
        bound_edge = 8 * math.sqrt(2) * float(s[b]) / float(a[b]) * DELTA
        d_mse, d_edge = abs(got[b, 0] - want[b, 0]), abs(got[b, 1] - want[b, 1])
        print(f"{variant} {compute} t={T2[b]}: mse {got[b, 0]:.6f} |d| {d_mse:.3e} (bound {bound_mse:.3e})   "
              f"edge {got[b, 1]:.6f} |d| {d_edge:.3e} (bound {bound_edge:.3e})")
        assert d_mse <= bound_mse and d_edge <= bound_edge
        assert abs(got[b, 2] - want[b, 2]) <= bound_mse + weight * bound_edge


@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_an_entry_does_not_depend_on_what_shares_its_batch(variant):
    den = _den(variant, "f16x3", batch_invariant=True)
    clean, noisy = _pair(3)
    t3 = (49, 7, 20)
    whole = den.denoising_loss(clean, noisy, t3, seed=SEED, sample_offset=4, draw=1)
    for b in range(3):
        one = den.denoising_loss(clean[b:b + 1], noisy[b:b + 1], t3[b:b + 1], seed=SEED, sample_offset=4 + b, draw=1)
        assert _same(one.loss, whole.loss[b:b + 1]) and _same(one.mse, whole.mse[b:b + 1]) and _same(one.edge, whole.edge[b:b + 1])
    assert not _same(den.denoising_loss(clean[1:2], noisy[1:2], t3[1:2], seed=SEED, sample_offset=4, draw=1).loss, whole.loss[1:2])


def test_loss_profile_does_not_depend_on_the_pass_size():
    den = _den("ddim", "f16x3", batch_invariant=True)
    clean, noisy = _pair(2)
    steps = (0, 7, 20, 33, 49)
    a = den.loss_profile(clean, noisy, timesteps=steps, seed=SEED, max_batch=4)        # passes of 4, 4 and 2 pairs
    b = den.loss_profile(clean, noisy, timesteps=steps, seed=SEED, max_batch=16)       # one pass of 10
    assert a.t == steps and a.loss.shape == (5, 2) and a.loss.dtype == torch.float64
    assert _same(a.loss, b.loss) and _same(a.mse, b.mse) and _same(a.edge, b.edge)
    # pair (b, k) is image b alone at (sample_offset + b, draw k)
    one = den.denoising_loss(clean[1:2], noisy[1:2], (33,), seed=SEED, sample_offset=1, draw=3)
    assert _same(one.loss.cpu(), a.loss[3, 1:2]) and _same(one.edge.cpu(), a.edge[3, 1:2])
    assert torch.isfinite(a.loss).all() and float(a.mse.min()) > 0
    full = den.loss_profile(clean[:1], noisy[:1], seed=SEED)
    assert full.t == tuple(range(50)) and full.loss.shape == (50, 1) and _same(full.loss[0], a.loss[0, :1])      # (t = 0 is draw 0 in both)


@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_a_nan_in_the_prediction_is_a_nan_for_that_sample_only(variant):
    den = _den(variant, "f16x3")
    clean, noisy = _pair(2)
    x_t, eps = den.noise_images(clean, T2, seed=SEED)
    pred = den.model(x_t, noisy, torch.tensor(T2))
    clamp = variant == "ddim"
    good, _ = midd_amd.loss_terms(clean, pred, T2, den.alpha_hat, x_t=x_t, noise=eps, clamp_eps=clamp)
    pred[1, 0, 5, 9] = float("nan")
    for kw in (dict(x_t=x_t, noise=eps), dict(seed=SEED)):
        out, maps = midd_amd.loss_terms(clean, pred, T2, den.alpha_hat, clamp_eps=clamp, return_maps=True, **kw)
        assert torch.isnan(out[1]).all() and _same(out[0], good[0])
        assert int(torch.isnan(maps[0]).sum()) == 1 and int(torch.isnan(maps[2]).sum()) == 1 and int(torch.isnan(maps[1]).sum()) == 8
        assert not torch.isnan(maps[:, 0]).any()


def test_cli_evaluation_prints_and_writes_the_profile(tmp_path, capsys):
    sd = make_state_dict(UNetConfig(), seed=42)
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "noise_steps": 50}, ckpt)
    clean = synthetic_xray(1, 88, 120, seed=9)[0, 0].clip(0, 1)
    noisy = np.clip(clean + 0.1 * np.random.default_rng(3).standard_normal(clean.shape), 0, 1)
    for name, a in (("clean", clean), ("noisy", noisy)):
        Image.fromarray((a * 255).astype(np.uint8), mode="L").save(tmp_path / f"{name}.png")
    out = tmp_path / "loss.json"
    kw = dict(device_type="cuda", img_size=64, inference_steps=3, variant="ddim")
    img = denoise_image_diffusion(str(ckpt), str(tmp_path / "noisy.png"), seed=11, clean=str(tmp_path / "clean.png"), loss_out=str(out), **kw)
    text = capsys.readouterr().out
    assert "Denoising loss of the checkpoint" in text and "PSNR" in text and "SSIM" in text
    res = json.loads(out.read_text())
    assert res["t"] == list(range(50)) and len(res["loss"]) == 50 and all(math.isfinite(v) and v > 0 for v in res["loss"])
    assert res["variant"] == "ddim" and math.isfinite(res["psnr"]) and -1 <= res["ssim"] <= 1
    np.testing.assert_allclose(res["loss"], np.asarray(res["mse"]) + 0.2 * np.asarray(res["edge"]), rtol=1e-12)
    # the sampler run and the returned image are those of the call without --clean
    plain = denoise_image_diffusion(str(ckpt), str(tmp_path / "noisy.png"), **kw)
    assert np.array_equal(np.asarray(img), np.asarray(plain))


@pytest.mark.parametrize("window", [None, (1.0, 99.0)])
def test_cli_evaluation_on_16_bit_files_uses_the_16_bit_recipe(tmp_path, window):
    """--bit-depth 16, plain and windowed: the profile the CLI writes is the profile of the pair loaded by the host recipe of
    image16.py (bit-identical to the device's by the prepost tests) -- the clean image under the NOISY image's window."""
    sd = make_state_dict(UNetConfig(), seed=42)
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "noise_steps": 50}, ckpt)
    clean = synthetic_xray(1, 88, 120, seed=9)[0, 0].clip(0, 1)
    noisy = np.clip(clean + 0.1 * np.random.default_rng(3).standard_normal(clean.shape), 0, 1)
    raw = {}
    for name, a in (("clean", clean), ("noisy", noisy)):
        raw[name] = (a * 4095.0 + 300.0).astype(np.uint16)                 # a 12-bit detector range inside a 16-bit file
        image16.image_from_u16(raw[name]).save(tmp_path / f"{name}.png")
    out = tmp_path / "loss.json"
    kw = {} if window is None else {"window": window}
    denoise_image_diffusion(str(ckpt), str(tmp_path / "noisy.png"), device_type="cuda", img_size=64, inference_steps=3, variant="ddim", seed=11,
                            bit_depth=16, clean=str(tmp_path / "clean.png"), loss_out=str(out), **kw)
    res = json.loads(out.read_text())
    if window is None:
        load = image16.unit_float
    else:
        levels = image16.window_levels(raw["noisy"], window)
        load = lambda a: image16.unit_float_window(a, levels)
    pair = [torch.from_numpy(image16.resize_f(load(raw[name]), (64, 64)))[None, None].cuda() for name in ("clean", "noisy")]
    m = UNetDiffusion()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    want = DiffusionDenoiser(m.cuda().eval(), noise_steps=50).loss_profile(pair[0], pair[1], seed=11)
    assert res["loss"] == want.loss[:, 0].tolist() and res["mse"] == want.mse[:, 0].tolist() and res["edge"] == want.edge[:, 0].tolist()
    assert math.isfinite(res["psnr"]) and -1 <= res["ssim"] <= 1
