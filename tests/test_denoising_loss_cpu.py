"""CPU: the specifications behind the denoising-loss calls (include/midd.h: THE FORWARD NOISE, THE NOISING, THE DENOISING LOSS) as
tests/denoising_loss_reference.py restates them -- against the reference's own code and torch eager (`reference`-marked; each has a
twin that reads tests/golden/denoising_loss_ref.npz, recorded from the reference by tests/golden/make_loss_golden.py) -- the counter
words of the forward noise, and the argument rules of the native calls and of the Python and CLI surface, all before any GPU work."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native
from midd_amd.cli import denoise_image_diffusion, main as cli_main
from tests import denoising_loss_reference as ref
from tests import step_noise_reference as sn
from tests.golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
CLAMP = {"ddim": True, "cddpm": False}
WEIGHT = {"ddim": 0.2, "cddpm": 0.0}


@pytest.fixture(scope="module")
def fx():
    return load("denoising_loss_ref")


# ------------------------------------------------------------------------------ 0. what fails without the feature
def test_the_surface_exists():
    for name in ("noise_images", "sample_timesteps", "denoising_loss", "loss_profile"):
        assert callable(getattr(DiffusionDenoiser, name)), name
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    for sym in ("mi_noise_images", "mi_loss_terms", "mi_loss_workspace_bytes", "mi_denoising_loss", "mi_denoising_loss_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert getattr(native.lib(), sym) is not None
    for title in ("THE FORWARD NOISE", "THE NOISING", "THE DENOISING LOSS"):
        assert title in header


def test_sample_timesteps_is_the_reference_draw():
    den = DiffusionDenoiser(UNetDiffusion(model_channels=16, time_emb_dim=64), noise_steps=50)
    g = torch.Generator().manual_seed(3)
    t = den.sample_timesteps(64, generator=g)
    assert t.shape == (64,) and t.dtype == torch.int64 and int(t.min()) >= 1 and int(t.max()) <= 49
    assert torch.equal(t, torch.randint(low=1, high=50, size=(64,), generator=torch.Generator().manual_seed(3)))
    torch.manual_seed(11)
    a = den.sample_timesteps(5)
    torch.manual_seed(11)
    assert torch.equal(a, torch.randint(low=1, high=50, size=(5,)))      # DDIMModel.py:266, the global generator


# ------------------------------------------------------------------------------ 1. the restatement against the reference
@pytest.mark.reference
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_restated_noising_is_the_reference_noise_images_bit_for_bit(reference_module, variant):
    refmod = getattr(reference_module, variant)
    den = refmod.DiffusionDenoiser(None, noise_steps=50)
    den.alpha_hat = den.alpha_hat.cpu()
    torch.manual_seed(5)
    clean = torch.rand(4, 1, 19, 23)
    t = torch.tensor([0, 49, 7, 31])
    x_t, eps = den.noise_images(clean, t)
    got = ref.noise_images(clean.numpy(), eps.numpy(), t.numpy(), den.alpha_hat.numpy())
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), x_t.numpy().view(np.uint32))


def test_restated_noising_equals_the_recorded_reference_output(fx):
    got = ref.noise_images(fx["clean"], fx["eps"], fx["t"], fx["alpha_hat"])
    assert np.array_equal(got.view(np.uint32), fx["x_t"].view(np.uint32))


def _torch_p(x_t, eps_pred, t, alpha_hat, clamp):
    """The reference's expression (DDIMModel.py:358-362) in torch eager on the CPU."""
    x_t, pred, ah = torch.from_numpy(x_t), torch.from_numpy(eps_pred), torch.from_numpy(alpha_hat)[torch.from_numpy(t)][:, None, None, None]
    e = torch.clamp(pred, -5, 5) if clamp else pred
    return torch.clamp((x_t - torch.sqrt(1 - ah) * e) / torch.sqrt(ah), 0, 1).numpy()


@pytest.mark.reference
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_restated_predicted_image_is_the_torch_eager_expression_bit_for_bit(reference_module, fx, variant):
    den = getattr(reference_module, variant).DiffusionDenoiser(None, noise_steps=50)
    ah = den.alpha_hat.cpu().numpy()
    assert np.array_equal(ah, fx["alpha_hat"])
    rng = np.random.default_rng(8)
    pred = (fx[f"eps_pred_{variant}"] * rng.choice([1.0, 6.0], size=fx["clean"].shape)).astype(np.float32)      # some beyond +-5
    want = _torch_p(fx["x_t"], pred, fx["t"], ah, CLAMP[variant])
    _, _, p = ref.pixel_maps(fx["clean"], fx["x_t"], fx["eps"], pred, fx["t"], ah, CLAMP[variant])
    assert np.array_equal(p.view(np.uint32), want.view(np.uint32))
    assert 0 < np.count_nonzero(p == 0) and 0 < np.count_nonzero((p > 0) & (p < 1))


@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_restated_predicted_image_equals_the_recorded_one(fx, variant):
    _, _, p = ref.pixel_maps(fx["clean"], fx["x_t"], fx["eps"], fx[f"eps_pred_{variant}"], fx["t"], fx["alpha_hat"], CLAMP[variant])
    assert np.array_equal(p.view(np.uint32), fx[f"p_{variant}"].view(np.uint32))


def _scalars_within_twice_the_references_distance(fx, variant, s32, s64):
    """|restated - float64| <= 2 * |reference fp32 - float64|, relative: two different fp32 evaluations of one quantity are each one
    such distance from the truth.  (loss of cddpm is its mse: edge_weight 0.)"""
    out, _ = ref.loss_terms(fx["clean"], fx["x_t"], fx["eps"], fx[f"eps_pred_{variant}"], fx["t"], fx["alpha_hat"], CLAMP[variant], WEIGHT[variant])
    ours = np.abs(out - s64) / np.abs(s64)
    theirs = np.abs(s32 - s64) / np.abs(s64)
    for b in range(out.shape[0]):
        for k, name in enumerate(("mse", "edge", "loss")):
            print(f"{variant} sample {b} {name}: restated {out[b, k]:.12g} float64 {s64[b, k]:.12g} distance {ours[b, k]:.3e} (reference fp32: {theirs[b, k]:.3e})")
    assert np.all(theirs > 0), "a reference scalar that equals its float64 value gives no yardstick"
    assert np.all(ours <= 2.0 * theirs), (ours, theirs)


@pytest.mark.reference
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_restated_scalars_against_the_reference_evaluated_now(reference_module, fx, variant):
    from tests.golden import make_loss_golden as gen
    from midd_amd.config import UNetConfig as Cfg
    refmod = getattr(reference_module, variant)
    model = gen.build(refmod, Cfg(variant=variant, **gen.SMALL), seed=int(fx["seed_weights"]), perturb=True)
    den = refmod.DiffusionDenoiser(model, noise_steps=50)
    den.alpha_hat = den.alpha_hat.cpu()
    clean, noisy, eps, t = (torch.from_numpy(fx[k]) for k in ("clean", "noisy", "eps", "t"))
    x_t, pred, p, s32 = gen.objective(model, den, clean, noisy, t, eps, variant, torch.float32)
    den.alpha_hat = den.alpha_hat.double()
    _, _, _, s64 = gen.objective(model, den, clean, noisy, t, eps, variant, torch.float64, pred=torch.from_numpy(pred))
    assert np.array_equal(x_t, fx["x_t"])                                                     # the fixture is what the reference gives
    np.testing.assert_allclose(pred, fx[f"eps_pred_{variant}"], rtol=0, atol=1e-5)            # (a thread count may regroup a conv's sums)
    np.testing.assert_allclose(s64, fx[f"scalars64_{variant}"], rtol=1e-5)
    np.testing.assert_allclose(s32, fx[f"scalars32_{variant}"], rtol=1e-5)
    _scalars_within_twice_the_references_distance(fx, variant, fx[f"scalars32_{variant}"], fx[f"scalars64_{variant}"])


@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_restated_scalars_against_the_recorded_reference(fx, variant):
    _scalars_within_twice_the_references_distance(fx, variant, fx[f"scalars32_{variant}"], fx[f"scalars64_{variant}"])


def test_ordered_sum_is_the_headers_order():
    """The order, spelled out pixel by pixel on a shape with partial patches, against the vectorised restatement."""
    rng = np.random.default_rng(2)
    v = (rng.random((1, 2, 37, 45)) * 10.0 ** rng.integers(-6, 3, (1, 2, 37, 45))).astype(np.float32)
    total = 0.0
    for c in range(2):
        for ty in range(2):
            for tx in range(2):
                lanes = []
                for j in range(256):
                    s = 0.0
                    for k in range(4):
                        y, x = ty * 32 + j // 32 + 8 * k, tx * 32 + j % 32
                        if y < 37 and x < 45:
                            s += float(v[0, c, y, x])
                    lanes.append(s)
                n = 256
                while n > 1:
                    n //= 2
                    lanes = [lanes[j] + lanes[j + n] for j in range(n)]
                total += lanes[0]
    assert ref.ordered_sum(v)[0] == total


def test_a_nan_prediction_stays_a_nan_for_its_sample_only(fx):
    pred = fx["eps_pred_ddim"].copy()
    pred[1, 0, 5, 9] = np.nan
    out, (q, g, p) = ref.loss_terms(fx["clean"], fx["x_t"], fx["eps"], pred, fx["t"], fx["alpha_hat"], True, 0.2)
    assert np.isfinite(out[0]).all() and np.isnan(out[1]).all()
    assert np.isnan(q[1, 0, 5, 9]) and np.isnan(p[1, 0, 5, 9]) and np.count_nonzero(np.isnan(q)) == 1
    hit = np.isnan(g[1, 0, 4:7, 8:11])                   # the eight neighbours: the centre tap of both kernels is zero
    assert hit.sum() == 8 and not hit[1, 1] and np.count_nonzero(np.isnan(g)) == 8


# ------------------------------------------------------------------------------ 2. counter separation
def test_forward_noise_shares_no_counter_with_the_step_noise():
    shape = (2, 1, 9, 11)
    z = ref.forward_noise(SEED, shape)
    step = 2.0 * sn.step_noise(SEED, 1, shape)[0]                       # iteration 0 of the sampler: c2 = 0
    assert not np.any(z == step) and abs(np.corrcoef(z.ravel(), step.ravel())[0, 1]) < 0.3
    # the generator itself is the step noise's: c2 = 0x80000000 | draw is the only difference
    e = np.arange(99, dtype=np.uint64)
    assert np.array_equal(z[1].ravel(), sn.normal(SEED, 1, 0x80000000, e))
    assert not np.any(ref.forward_noise(SEED, shape, draw=1) == z)       # draw changes the value
    assert np.array_equal(ref.forward_noise(SEED, shape, draw=5), ref.forward_noise(SEED, shape, draws=[5, 5]))
    assert np.abs(z).max() <= 5.77


def test_sample_offset_shifts_the_rows():
    whole = ref.forward_noise(SEED, (4, 2, 5, 7))
    assert np.array_equal(ref.forward_noise(SEED, (1, 2, 5, 7), sample_offset=3)[0], whole[3])
    assert np.array_equal(ref.forward_noise(SEED, (2, 2, 5, 7), sample_index=[3, 1]), whole[[3, 1]])
    assert not np.array_equal(ref.forward_noise(SEED, (1, 2, 5, 7))[0], whole[3])


# ------------------------------------------------------------------------------ 3. argument rules of the native calls (no GPU work)
B_, C_, H_, W_ = 2, 1, 8, 8
_buf = np.zeros(B_ * C_ * H_ * W_ * 3 + 64, np.float32)
PTR = _buf.ctypes.data                                                     # a non-null, 16-byte aligned "device" pointer: never read
_ah = np.linspace(0.99, 0.5, 50).astype(np.float32)
AH = _ah.ctypes.data_as(C.POINTER(C.c_float))


def _t(*vals):
    return (C.c_int32 * len(vals))(*vals)


def _i64(*vals):
    return (C.c_int64 * len(vals))(*vals)


def _noise(t=_t(1, 2), eps=None, seeded=1, offset=0, draw=0, si=None, dr=None, clean=PTR, x_t=PTR, eps_out=None, shape=(B_, C_, H_, W_), steps=50, ah=AH):
    return native.lib().mi_noise_images(clean, t, ah, steps, eps, seeded, C.c_uint64(SEED), offset, draw, si, dr, x_t, eps_out, *shape, None)


def _terms(t=_t(1, 2), x_t=None, eps=None, seeded=1, offset=0, draw=0, si=None, dr=None, pred=PTR, out=PTR, ws=PTR, ws_bytes=1 << 12,
           shape=(B_, C_, H_, W_), weight=0.2):
    return native.lib().mi_loss_terms(PTR, x_t, eps, pred, t, AH, 50, seeded, C.c_uint64(SEED), offset, draw, si, dr, native.MI_CLAMP_EPS, weight,
                                      out, None, *shape, ws, ws_bytes, None)


@pytest.fixture(scope="module")
def plan():
    cfg = UNetConfig(model_channels=16, time_emb_dim=64)
    s = native.UNetCfg()
    s.in_channels, s.model_channels, s.num_levels = cfg.in_channels, cfg.model_channels, len(cfg.channel_mult)
    for i, m in enumerate(cfg.channel_mult):
        s.channel_mult[i] = m
    s.num_res_blocks, s.num_attention_levels = cfg.num_res_blocks, len(cfg.attention_resolutions)
    for i, a in enumerate(cfg.attention_resolutions):
        s.attention_levels[i] = a
    s.time_emb_dim, s.variant = cfg.time_emb_dim, native.MI_VARIANT[cfg.variant]
    h = C.c_void_p()
    native.check(native.lib().mi_unet_plan_create(C.byref(s), C.byref(h)))
    yield h
    native.lib().mi_plan_destroy(h)


def _whole(plan, t=_t(1, 2), eps=None, seeded=1, offset=0, draw=0, si=None, dr=None, clean=PTR, cond=PTR, out=PTR, B=B_, H=H_, W=W_):
    return native.lib().mi_denoising_loss(plan, clean, cond, t, AH, 50, eps, seeded, C.c_uint64(SEED), offset, draw, si, dr, 0, 0.2, out, None,
                                          B, H, W, PTR, 1 << 20, None)


def _refused(rc, word):
    msg = native.lib().mi_last_error().decode()
    assert rc == -1 and word in msg, (rc, msg)


def test_native_calls_refuse_bad_arguments_before_any_gpu_work(plan):
    for call in (_noise, _terms, lambda **kw: _whole(plan, **kw)):
        _refused(call(t=_t(1, 50)), "timestep 50 of sample 1 outside [0, 50)")
        _refused(call(t=_t(-1, 2)), "timestep -1 of sample 0")
        _refused(call(draw=2 ** 31), "draw must be in [0, 2^31)")
        _refused(call(draw=-1), "draw must be in [0, 2^31)")
        _refused(call(dr=_i64(0, 2 ** 31)), "draw must be in [0, 2^31), got 2147483648 for sample 1")
        _refused(call(offset=-1), "sample_offset must be >= 0")
        _refused(call(si=_i64(4, -2)), "sample_index must be >= 0")
        _refused(call(eps=PTR), "both a seed and eps")
        _refused(call(seeded=0), "neither a seed nor eps")
        _refused(call(t=None), "null argument")
    _refused(_noise(seeded=0, eps=PTR, si=_i64(0, 1)), "without a seed")
    _refused(_noise(clean=None), "null argument")
    _refused(_noise(x_t=None), "null argument")
    _refused(_noise(ah=None), "null argument")
    _refused(_noise(seeded=0, eps=PTR, eps_out=PTR), "eps_out with eps")
    _refused(_noise(shape=(1, 1, 65536, 65536), t=_t(1)), "C*H*W must stay below 2^32")
    _refused(_noise(shape=(0, 1, 8, 8)), "must be positive")
    for call in (_noise, _terms):                  # (H + 31 must stay inside an int: refused by name, not as a workspace that is too small)
        _refused(call(shape=(1, 1, 2 ** 31 - 1, 1), t=_t(1)), "H and W must be at most 2^30")
        _refused(call(shape=(1, 1, 1, 2 ** 30 + 1), t=_t(1)), "H and W must be at most 2^30")
    _refused(_noise(clean=PTR + 2), "4-byte aligned")
    _refused(_noise(steps=0), "noise_steps must be positive")
    _refused(_terms(shape=(1, 1, 65536, 65536), t=_t(1)), "C*H*W must stay below 2^32")
    _refused(_terms(pred=None), "null argument")
    _refused(_terms(out=None), "null argument")
    _refused(_terms(ws=None), "null argument")
    _refused(_terms(x_t=PTR), "both a seed and x_t")
    _refused(_terms(seeded=0, eps=PTR), "the explicit form reads x_t")
    _refused(_terms(weight=float("nan")), "edge_weight is NaN")
    _refused(_terms(out=PTR + 4), "8-byte aligned")
    assert _terms(ws_bytes=8) == -4 and b"workspace too small" in native.lib().mi_last_error()
    _refused(_whole(None), "null plan")
    _refused(_whole(plan, cond=None), "null argument")
    _refused(_whole(plan, out=None), "null argument")
    # past the argument rules the whole call asks for the plan's state (no weights were loaded): not a crash, and still no GPU work
    assert _whole(plan) == -2 and b"mi_unet_finalize" in native.lib().mi_last_error()


def test_workspace_queries():
    lib = native.lib()
    assert lib.mi_loss_workspace_bytes(8, 1, 256, 256) == 8 * 1 * 64 * 2 * 8                    # [B][C][patches][2] doubles
    assert lib.mi_loss_workspace_bytes(2, 1, 37, 45) == 256                                     # 2 * 4 patches: 128 bytes, rounded up to 256
    assert lib.mi_loss_workspace_bytes(1, 3, 32, 64) == 256 and lib.mi_loss_workspace_bytes(1, 1, 8, 8) == 256
    assert lib.mi_loss_workspace_bytes(0, 1, 8, 8) == 0 and lib.mi_loss_workspace_bytes(1, 1, 65536, 65536) == 0
    assert lib.mi_loss_workspace_bytes(1, 1, 2 ** 31 - 1, 1) == 0 and b"2^30" in lib.mi_last_error()
    assert lib.mi_loss_workspace_bytes(1, 1, 2 ** 30, 1) == 2 ** 25 * 16                          # the largest side: 2^25 patches
    assert lib.mi_denoising_loss_workspace_bytes(None, 1, 64, 64) == 0 and b"null plan" in lib.mi_last_error()


# ------------------------------------------------------------------------------ 4. argument rules of the Python surface and the CLI
def test_python_surface_refuses_before_the_device_check():
    den = DiffusionDenoiser(UNetDiffusion(model_channels=16, time_emb_dim=64), noise_steps=50)
    x = torch.rand(2, 1, 16, 16)
    with pytest.raises(ValueError, match="either seed .* or noise"):
        den.noise_images(x, [1, 2], seed=1, noise=torch.zeros_like(x))
    with pytest.raises(ValueError, match=r"t must be in \[0, 50\)"):
        den.noise_images(x, [1, 50], seed=1)
    with pytest.raises(ValueError, match="t must have 2 entries"):
        den.noise_images(x, [1, 2, 3], seed=1)
    with pytest.raises(ValueError, match="draw must be in"):
        den.noise_images(x, [1, 2], seed=1, draw=2 ** 31)
    with pytest.raises(ValueError, match="sample_offset must be in"):
        den.noise_images(x, [1, 2], seed=1, sample_offset=-1)
    with pytest.raises(ValueError, match="noise must be a"):
        den.noise_images(x, [1, 2], noise=torch.zeros(2, 1, 16, 15))
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        den.noise_images(torch.rand(16, 16), [1], seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        den.noise_images(x, [1, 2], seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        den.noise_images(x, [1, 2])                                   # the reference's own signature: torch.randn_like, then the device
    with pytest.raises(ValueError, match="either seed .* or noise"):
        den.denoising_loss(x, x, [1, 2], seed=1, noise=torch.zeros_like(x))
    with pytest.raises(ValueError, match="edge_weight must not be NaN"):
        den.denoising_loss(x, x, [1, 2], seed=1, edge_weight=float("nan"))
    with pytest.raises(ValueError, match="timesteps must be in"):
        den.loss_profile(x, x, timesteps=[0, 50], seed=1)
    with pytest.raises(ValueError, match="max_batch must be in"):
        den.loss_profile(x, x, seed=1, max_batch=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        den.denoising_loss(x, x, [1, 2], seed=1)


@pytest.mark.parametrize("flag,kw", [("--tile", {"tile": 64}), ("--samples", {"samples": 4}), ("--views", {"tile": None, "views": "auto"}),
                                     ("--self-ensemble", {"self_ensemble": "auto"}), ("--members", {"members": 2})])
def test_cli_evaluation_refuses_the_flags_that_make_no_sense_with_it(flag, kw):
    with pytest.raises(ValueError, match=re.escape(f"--clean (evaluation) cannot be combined with {flag}")):
        denoise_image_diffusion(None, "noisy.png", device_type="cpu", clean="clean.png", **kw)
    argv = ["--image", "noisy.png", "--clean", "clean.png", flag] + ([] if flag in ("--views", "--self-ensemble") else ["64"])
    with pytest.raises(SystemExit):
        cli_main(argv)


def test_cli_evaluation_refuses_a_cpu_device_before_anything_runs():
    with pytest.raises(RuntimeError, match="runs only on a ROCm GPU"):      # (neither file exists: nothing was opened, nothing sampled)
        denoise_image_diffusion(None, "no_such_noisy.png", device_type="cpu", clean="no_such_clean.png")


def test_two_denoisers_with_different_schedules_keep_their_own_tables():
    """The host copy of alpha_hat belongs to the call: a second denoiser, or a replaced table, is never answered from an earlier one."""
    from midd_amd.sampler import loss_table_args
    a = DiffusionDenoiser(UNetDiffusion(model_channels=16, time_emb_dim=64), noise_steps=50)
    ta = loss_table_args([3], a.alpha_hat, 1)[0][0].copy()
    del a
    b = DiffusionDenoiser(UNetDiffusion(model_channels=16, time_emb_dim=64), noise_steps=50, beta_end=0.05)
    tb = loss_table_args([3], b.alpha_hat, 1)[0][0]
    assert np.array_equal(tb, b.alpha_hat.numpy()) and not np.array_equal(tb, ta)
    b.alpha_hat = b.alpha_hat * 0.5
    assert np.array_equal(loss_table_args([3], b.alpha_hat, 1)[0][0], b.alpha_hat.numpy())
    # the copy a denoiser keeps follows its own table: another tensor, and a write in place
    first = b._alpha_hat_host()
    assert b._alpha_hat_host() is first and np.array_equal(first, b.alpha_hat.numpy())
    b.alpha_hat.mul_(0.5)
    assert np.array_equal(b._alpha_hat_host(), b.alpha_hat.numpy()) and not np.array_equal(first, b.alpha_hat.numpy())
    b.alpha_hat = b.alpha_hat.clone() + 0.01
    assert np.array_equal(b._alpha_hat_host(), b.alpha_hat.numpy())
    c = DiffusionDenoiser(UNetDiffusion(model_channels=16, time_emb_dim=64), noise_steps=50)
    assert np.array_equal(c._alpha_hat_host(), c.alpha_hat.numpy()) and not np.array_equal(c._alpha_hat_host(), b._alpha_hat_host())


def test_cli_loss_out_needs_clean(capsys):
    with pytest.raises(ValueError, match="--loss-out needs --clean"):
        denoise_image_diffusion(None, "noisy.png", device_type="cpu", loss_out="x.json")
    with pytest.raises(SystemExit):
        cli_main(["--image", "noisy.png", "--loss-out", "x.json"])
    assert "--loss-out needs --clean" in capsys.readouterr().err
