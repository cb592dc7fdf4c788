"""GPU: the DDIM(eta) update rule fused into the out-conv epilogue (include/midd.h: THE DDIM UPDATE; out_conv_ddim_kernel and
out_conv_ddim_seeded_kernel).

The rule is a specification, so the device is held to its numpy restatement (tests/ddim_update_reference.py) bit for bit, given
the network's own eps from ``forward``; the seeded form to its replay through the noise tensor; the whole loop to the restated
loop over the CPU oracle within the project's parity gate; and the batched calls to the plain call."""
import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, timestep_list, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import ddim_update_reference as ref
from tests import tiled_reference as tiles_ref

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # north_star: |delta| < 1e-3 fp32 per pixel (tests/test_gpu_parity.py)
SEED = 0x1234567890ABCDEF
K = 5                     # inference_steps of the seeded cases: the list 40, 30, 20, 10, 0
NOISE_STEPS = 50

_sds, _models = {}, {}


def _sd(variant):
    if variant not in _sds:
        _sds[variant] = make_state_dict(UNetConfig(variant=variant), seed=42)
    return _sds[variant]


def _model(variant, compute="f16x3", batch_invariant=False):
    key = (variant, compute, batch_invariant)
    if key not in _models:
        m = UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd(variant).items()}, strict=True)
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=NOISE_STEPS)
    return _models[key]


def _images(B, H=64, W=64, seed=77):
    return torch.from_numpy(synthetic_xray(B, H, W, seed=seed)).cuda()


def _stretched(B, H, W):
    """synthetic_xray with its contrast doubled about 0.5 and cut to [0, 1]: a quarter of the pixels sit at 0 or 1, so that the
    predicted image leaves the range on 3.6 % .. 40 % of them in every case below (CPU restatement over the oracle, both variants,
    both lists; the plain image gives 0.5 % on the one-entry list whatever its seed)."""
    x = np.clip((synthetic_xray(B, H, W, seed=77) - 0.5) * 2.0 + 0.5, 0.0, 1.0).astype(np.float32)
    return torch.from_numpy(x).cuda()


def _fma_f32(a, b, c):
    """fp32 fused multiply-add a * b + c, exactly (finite values far from float64's limits, as here).  The product of two fp32
    values is exact in float64.  The sum is rounded to float64 TO ODD: where it is inexact (its two-sum error is not zero) and the
    nearest float64 has an even mantissa, the neighbour on the error's side is taken.  A value rounded to odd at 53 bits rounds to
    24 bits as the exact value does (53 >= 24 + 2), so there is no double rounding."""
    p, c = np.float64(a) * b.astype(np.float64), c.astype(np.float64)
    s = p + c
    v = s - p
    err = (p - (s - v)) + (c - v)                                            # two-sum: p + c == s + err exactly
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0.0) & even, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _reference_restated(x, eps, t, den, clamp_eps):
    """The reference's update as out_conv_kernel evaluates it (profiles/step_noise_isa.txt): x - c2 * eps is ONE fused
    multiply-add (hipcc contracts it), the product with c1 and the clamp are rounded on their own."""
    F = np.float32
    alpha, alpha_hat = den.alpha.cpu().numpy(), den.alpha_hat.cpu().numpy()
    c1 = F(1.0) / np.sqrt(F(alpha[t]))
    c2 = (F(1.0) - F(alpha[t])) / np.sqrt(F(1.0) - F(alpha_hat[t]))
    e = np.fmin(np.fmax(eps, F(-5.0)), F(5.0)) if clamp_eps else eps
    return np.fmin(np.fmax(c1 * _fma_f32(-c2, e, x), F(0.0)), F(1.0))


# ------------------------------------------------------------------------------ 1. the update, bit for bit
@pytest.mark.parametrize("shape", [(3, 40, 24), (1, 64, 64), (4, 40, 24)])
@pytest.mark.parametrize("clip_x0", [True, False])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_update_equals_the_numpy_restatement_bit_for_bit(variant, eta, clip_x0, shape):
    """The lists [48, 24] and [24] with MI_NO_SPLIT on a batch-invariant plan.  eps comes from ``forward`` at the same batch, so
    the two sides differ in the update alone: x1 from eps0, eps1 = model(x1, cond, 24), x2 from eps1.  First the control: the same
    restatement of the REFERENCE rule gives the existing call's bits, i.e. ``forward`` and the loop share their eps.
    40 x 24: a multiple of 8 that is no multiple of the 16-pixel out-conv tile on either axis (edge workgroups); 64 x 64: 16
    workgroups per sample; B = 4 is the smallest batch the default call would split."""
    B, H, W = shape
    den = _model(variant, batch_invariant=True)
    clamp_eps = variant == "ddim"
    cond = _stretched(B, H, W)
    x_np = cond.cpu().numpy()
    alpha_hat = den.alpha_hat.cpu().numpy()
    tabs = (den.beta, den.alpha, den.alpha_hat)
    gen = torch.Generator().manual_seed(11)
    noise = (0.5 * torch.randn((2, B, 1, H, W), generator=gen)).cuda()

    def model_eps(x, t):
        xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        return den.model(xt, cond, torch.full((B,), t, dtype=torch.long)).cpu().numpy()

    eps48, eps24 = model_eps(x_np, 48), model_eps(x_np, 24)
    # control: the reference rule, restated the same way
    for t, eps in ((48, eps48), (24, eps24)):
        got = den.model.run_sampler(cond, [t], *tabs, clamp_eps=clamp_eps, no_split=True).cpu().numpy()
        assert np.array_equal(got, _reference_restated(x_np, eps, t, den, clamp_eps)), f"control, t = {t}: forward and the loop do not share bits"

    kw = dict(clamp_eps=clamp_eps, no_split=True, update="ddim", eta=eta, clip_x0=clip_x0)
    # [24]: one iteration, the last one
    rows = ref.coefficients([24], alpha_hat, eta)
    want, mask = ref.update(x_np, eps24, rows[0], clamp_eps, clip_x0, last=True, noise=noise[0].cpu().numpy())
    got = den.model.run_sampler(cond, [24], *tabs, step_noise=noise[:1].contiguous(), **kw).cpu().numpy()
    masks = [float(mask.mean())]
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    assert want.min() >= 0.0 and want.max() <= 1.0
    # [48, 24]: an unclamped intermediate x, then the last iteration
    rows = ref.coefficients([48, 24], alpha_hat, eta)
    x1, mask = ref.update(x_np, eps48, rows[0], clamp_eps, clip_x0, last=False, noise=noise[0].cpu().numpy())
    masks.append(float(mask.mean()))
    assert x1.max() > 1.0                                 # the intermediate state does leave [0, 1]: no clamp under this rule
    want, mask = ref.update(x1, model_eps(x1, 24), rows[1], clamp_eps, clip_x0, last=True, noise=noise[1].cpu().numpy())
    got = den.model.run_sampler(cond, [48, 24], *tabs, step_noise=noise, **kw).cpu().numpy()
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    print(f"{variant} eta {eta} clip {clip_x0} {shape}: clip changed x0 on {masks[0]:.3f} ([24]) and {masks[1]:.3f} ([48, 24]) of the pixels")
    if clip_x0:
        assert all(0.01 <= m <= 0.99 for m in masks), masks
    else:
        assert masks == [0.0, 0.0]
    if eta == 1.0:                                        # the noise term is really there (s > 0 on the first row only)
        quiet = den.model.run_sampler(cond, [48, 24], *tabs, **kw).cpu().numpy()
        assert not np.array_equal(quiet, got)


# ------------------------------------------------------------------------------ 2. seeded == its replay
@pytest.mark.parametrize("no_split", [False, True])
@pytest.mark.parametrize("compute,B", [("f16x3", 1), ("f16x3", 3), ("f16x3", 4), ("f32", 1), ("f32", 3), ("f32", 4), ("f16", 4)])
def test_seeded_run_equals_its_replay_bit_for_bit(compute, B, no_split):
    """B = 4: two programs of 2 on two streams unless MI_NO_SPLIT (the second one's samples start at global index 2); 3, 1: one."""
    den = _model("cddpm", compute)
    x = _images(B)
    steps = timestep_list(NOISE_STEPS, K)
    args = (x, steps, den.beta, den.alpha, den.alpha_hat)
    kw = dict(clamp_eps=False, no_split=no_split, update="ddim", eta=1.0)
    seeded = den.model.run_sampler(*args, seed=SEED, **kw)
    replay = den.model.run_sampler(*args, step_noise=midd_amd.step_noise(SEED, len(steps), x.shape), **kw)
    assert torch.isfinite(seeded).all() and torch.equal(seeded, replay)
    assert float(seeded.min()) >= 0.0 and float(seeded.max()) <= 1.0
    if not no_split:
        assert torch.equal(den.denoise(x, K, update="ddim", eta=1.0, seed=SEED), seeded)


@pytest.mark.parametrize("variant", ["cddpm", "ddim"])
def test_same_seed_same_bits_other_seed_other_bits(variant):
    den = _model(variant)
    x = _images(3)
    first = den.denoise(x, K, update="ddim", eta=1.0, seed=SEED)
    assert torch.equal(den.denoise(x, K, update="ddim", eta=1.0, seed=SEED), first)
    assert not torch.equal(den.denoise(x, K, update="ddim", eta=1.0, seed=SEED + 1), first)
    assert not torch.equal(den.denoise(x, K, update="ddim", eta=0.5, seed=SEED), first)
    # eta = 0 is deterministic: neither a seed nor a noise tensor shows
    quiet = den.denoise(x, K, update="ddim")
    assert torch.equal(den.denoise(x, K, update="ddim", seed=SEED), quiet)
    assert torch.equal(den.denoise(x, K, update="ddim", seed=SEED + 1), quiet)
    assert torch.equal(den.denoise(x, K, update="ddim", step_noise=midd_amd.step_noise(SEED, K, x.shape)), quiet)
    assert not torch.equal(quiet, first)
    # without a source at eta > 0 the noise is torch's: two calls differ
    assert not torch.equal(den.denoise(x, K, update="ddim", eta=1.0), den.denoise(x, K, update="ddim", eta=1.0))


# ------------------------------------------------------------------------------ 3. against the oracle
_oracle = {}


def _oracle_loop(x, clip_x0=True):
    """The restated loop over the CPU oracle's forward, on the served list (9 of 50), once."""
    if "ddim" not in _oracle:
        cfg = UNetConfig(variant="ddim")
        sd, topo = orc.to_torch(_sd("ddim")), topology(cfg)
        cond = x.cpu()
        _, _, alpha_hat = ref.schedule(NOISE_STEPS)

        def eps(xn, t):
            return orc.unet_forward(sd, topo, torch.from_numpy(xn), cond, torch.full((xn.shape[0],), t, dtype=torch.long)).numpy()

        steps = timestep_list(NOISE_STEPS, 8)
        assert len(steps) == 9
        _oracle["ddim"] = ref.loop(cond.numpy(), steps, alpha_hat, 0.0, eps, clamp_eps=True)
        _oracle["reference"] = orc.denoise(sd, topo, cond, NOISE_STEPS, 8).numpy()
    return _oracle


@pytest.mark.parametrize("compute", ["f16x3", "f32"])
def test_whole_loop_matches_the_restated_loop_over_the_oracle(compute):
    """denoise(x, 8, update="ddim") at 64 x 64, B = 2 against tests/ddim_update_reference.loop running on the oracle's forward.
    The gate is the project's parity gate; the reference rule on the same inputs is measured next to it."""
    den = _model("ddim", compute)
    x = _images(2)
    want = _oracle_loop(x)
    got = den.denoise(x, 8, update="ddim").cpu().numpy()
    got_ref = den.denoise(x, 8).cpu().numpy()
    err, err_ref = float(np.abs(got - want["ddim"]).max()), float(np.abs(got_ref - want["reference"]).max())
    print(f"{compute}: update=ddim vs restated loop over the oracle max|delta| = {err:.3e}; reference rule vs oracle {err_ref:.3e}")
    assert np.isfinite(got).all() and err < TOL_FINAL
    assert float(np.abs(want["ddim"] - want["reference"]).max()) > 10 * TOL_FINAL      # the two rules are different samplers


# ------------------------------------------------------------------------------ 4. the batched calls
def test_one_tile_is_the_plain_call():
    den = _model("cddpm")
    x = _images(2)
    kw = dict(update="ddim", eta=1.0, seed=SEED)
    res = den.denoise_tiled(x, K, tile=64, overlap=16, return_tiles=True, **kw)
    plain = den.denoise(x, K, **kw)
    assert res.origins_y == (0,) and res.origins_x == (0,) and res.seed == SEED
    assert torch.equal(res.image, plain) and torch.equal(res.tiles[:, 0], plain)
    quiet = den.denoise_tiled(x, K, tile=64, overlap=16, update="ddim", seed=SEED)      # eta = 0: the seed is ignored
    assert quiet.seed is None and torch.equal(quiet.image, den.denoise(x, K, update="ddim"))


@pytest.mark.parametrize("variant", ["cddpm", "ddim"])
def test_ensemble_member_zero_is_the_plain_seeded_call(variant):
    """Also: the DDIM variant has an ensemble under this rule once eta > 0, and none at eta = 0."""
    den = _model(variant, batch_invariant=True)
    x = _images(2, 40, 24)
    kw = dict(update="ddim", eta=1.0, seed=SEED)
    ens = den.denoise_ensemble(x, K, members=3, return_samples=True, **kw)
    assert ens.samples.shape == (2, 3, 1, 40, 24) and ens.seed == SEED and torch.isfinite(ens.mean).all()
    assert torch.equal(ens.samples[:, 0], den.denoise(x, K, **kw))
    assert torch.equal(ens.samples[:, 2], den.denoise(x, K, member=2, **kw))
    assert float(ens.std.max()) > 0.0
    with pytest.raises(ValueError, match="deterministic"):
        den.denoise_ensemble(x, K, members=3, update="ddim", seed=SEED)
    if variant == "ddim":
        with pytest.raises(ValueError, match="deterministic"):
            den.denoise_ensemble(x, K, members=3, seed=SEED)


def test_tiled_call_equals_the_restated_blend_of_per_tile_calls():
    """72 x 56 as 40 x 40 tiles with overlap 8: origins (0, 32) x (0, 16).  Every tile is the plain call on its crop with the crop
    of the image's noise field (batch-invariant plan), and the image is the float64 blend of those."""
    H, W, T, O = 72, 56, 40, 8
    den = _model("cddpm", batch_invariant=True)
    x = _images(2, H, W)
    plan = midd_amd.tile_plan(H, W, T, O)
    assert (plan.origins_y, plan.origins_x) == ((0, 32), (0, 16))
    res = den.denoise_tiled(x, K, tile=T, overlap=O, update="ddim", eta=1.0, seed=SEED, return_tiles=True)
    field = midd_amd.step_noise(SEED, K, x.shape)
    crops = midd_amd.tile_extract(x, T, O).reshape(8, 1, T, T)
    noise = torch.stack([field[:, b, :, y0:y0 + T, x0:x0 + T] for b in range(2) for y0 in plan.origins_y for x0 in plan.origins_x], dim=1)
    alone = den.denoise(crops, K, update="ddim", eta=1.0, step_noise=noise.contiguous())
    assert torch.equal(res.tiles.reshape(8, 1, T, T), alone)
    assert np.array_equal(res.image.cpu().numpy(), tiles_ref.blend(alone.reshape(2, 4, 1, T, T).cpu().numpy(), H, W, (O, O)))


# ------------------------------------------------------------------------------ 5. the default is the reference's rule
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_update_reference_is_the_default_bit_for_bit(variant):
    den = _model(variant)
    x = _images(4)
    kw = dict(seed=SEED) if variant == "cddpm" else {}
    assert torch.equal(den.denoise(x, K, **kw), den.denoise(x, K, update="reference", **kw))
    a, b = den.denoise_tiled(x, K, tile=64, **kw), den.denoise_tiled(x, K, tile=64, update="reference", **kw)
    assert torch.equal(a.image, b.image)
    assert not torch.equal(den.denoise(x, K, update="ddim", **kw), den.denoise(x, K, **kw))
    if variant == "cddpm":
        e0, e1 = den.denoise_ensemble(x[:1], K, members=2, **kw), den.denoise_ensemble(x[:1], K, members=2, update="reference", **kw)
        assert torch.equal(e0.mean, e1.mean) and torch.equal(e0.std, e1.std)
