"""GPU: every sampler call on networks with more than one image channel (`in_channels` 2..4).

With one channel the channel index is 0 wherever it enters an address or a noise counter word -- `oc * plane` in the seeded
updates (the plane of the WHOLE image for a tile), the per-iteration slice `i * B*C*H*W` of a noise tensor, the C*H*W strides of the
ensemble, tile and view stores, the idle-slot return of the slots kernel -- so no one-channel case can tell a right index from a
wrong one, and the run-time-channel compiles `out_conv_*_kernel<0>` are reached by `forward` alone.  Here every call of the
sampler runs on

  NET3         the default topology with in_channels = 3: in_conv_kernel at Cout = 48 (3 channel groups, 85 pixel lanes: thread 255
               idles through the statistics) and out_conv_*<0> at C = 48;
  NET2 / NET4  a two-level 32-wide network, cheap for the CPU oracle; 4 channels is the accumulator bound of the out-conv kernel.

Shapes: (4, 40, 24) -- the smallest batch the default call splits into two sub-batch programs, 40 x 24 a multiple of 8 that is no
multiple of the 16-pixel out-conv tile on either axis; (3, 40, 24) one program; 40 x 40 where the views transpose; lists of at most
5 entries of a 50-step schedule.  Channels differ: images are `synthetic_xray` with another seed per channel, noise tensors are
drawn over all channels from one generator.

Contracts: bit identity (`torch.equal` / `np.array_equal`) wherever the project states one, the parity gate TOL_FINAL = 1e-3 of
tests/test_gpu_parity.py against the CPU oracle, and for compute="f16" that mode's own rule (tests/f16_emulation.py)."""
import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, timestep_list, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import ddim_update_reference as dref
from tests import ensemble_reference as eref
from tests import quantile_reference as qref
from tests import self_ensemble_reference as sref
from tests import tiled_reference as tref
from tests.f16_emulation import AutocastEmulation, distance, gate
from tests.test_gpu_ddim_update import _reference_restated

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # north_star: |delta| < 1e-3 fp32 per pixel (tests/test_gpu_parity.py)
SEED = 0x1234567890ABCDEF
K = 5                     # inference_steps: the list 40, 30, 20, 10, 0
NOISE_STEPS = 50
OFFSET = 3                # sample_offset of the tiled cases
LEVELS = (0.05, 0.5, 0.95)
H, W = 40, 24
TWO_LEVEL = dict(model_channels=32, channel_mult=(1, 2), num_res_blocks=2, attention_resolutions=(1,), time_emb_dim=32)
NETS = {"NET2": dict(in_channels=2, **TWO_LEVEL), "NET3": dict(in_channels=3), "NET4": dict(in_channels=4, **TWO_LEVEL)}
TILED = (56, 72, 32, 8)   # image H, W, tile, overlap: 2 x 3 tiles, origins (0, 24) x (0, 20, 40)

_sds, _models, _oracle = {}, {}, {}


def _channels(net):
    return NETS[net]["in_channels"]


def _cfg(net, variant):
    return UNetConfig(variant=variant, **NETS[net])


def _sd(net, variant):
    if (net, variant) not in _sds:
        _sds[net, variant] = make_state_dict(_cfg(net, variant), seed=42)
    return _sds[net, variant]


def _den(net, variant, compute="f16x3", batch_invariant=False):
    key = (net, variant, compute, batch_invariant)
    if key not in _models:
        m = UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant, **NETS[net])
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd(net, variant).items()}, strict=True)
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=NOISE_STEPS)
    return _models[key]


def images_np(C, B, h=H, w=W, seed=77):
    """[B, C, h, w]: another synthetic image per channel (tests/test_gpu_parity.py: test_other_topologies_forward_vs_oracle)."""
    return np.concatenate([synthetic_xray(B, h, w, seed=seed + 31 * c) for c in range(C)], axis=1)


def stretched_np(C, B, h=H, w=W):
    """The contrast-stretched image of tests/test_gpu_ddim_update.py, per channel."""
    return np.clip((images_np(C, B, h, w) - 0.5) * 2.0 + 0.5, 0.0, 1.0).astype(np.float32)


def tensor_noise(n, shape, seed=11):
    """[n, B, C, H, W], 0.5-scaled, all channels from one generator."""
    return 0.5 * torch.randn((n,) + tuple(shape), generator=torch.Generator().manual_seed(seed))


def _images(net, B, h=H, w=W, seed=77):
    return torch.from_numpy(images_np(_channels(net), B, h, w, seed)).cuda()


def _sampler(den, x, steps, **kw):
    return den.model.run_sampler(x, steps, den.beta, den.alpha, den.alpha_hat, clamp_eps=den.model.variant != "cddpm", **kw)


def _run_slots(den, cond, x, rows, **kw):
    return den.model.run_slots(cond, x, rows, den.beta, den.alpha, den.alpha_hat, clamp_eps=den.model.variant != "cddpm", **kw)


def _view_t(x, g):
    u = x.transpose(-1, -2) if g & 4 else x
    if g & 2:
        u = u.flip(-2)
    if g & 1:
        u = u.flip(-1)
    return u.contiguous()


def _unview_t(y, g):
    u = y
    if g & 1:
        u = u.flip(-1)
    if g & 2:
        u = u.flip(-2)
    if g & 4:
        u = u.transpose(-1, -2)
    return u.contiguous()


def _oracle_denoise(net, variant, x, noise=None, emulate=False, steps=K):
    sd_t, topo = orc.to_torch(_sd(net, variant)), topology(_cfg(net, variant))
    kw = {} if noise is None else dict(step_noise=list(noise))
    if emulate:
        with AutocastEmulation(True):
            return orc.denoise(sd_t, topo, x, NOISE_STEPS, steps, **kw).float().numpy()
    return orc.denoise(sd_t, topo, x, NOISE_STEPS, steps, **kw).numpy()


# ------------------------------------------------------------------------------ 1. the reference update, tensor noise, vs the oracle
def _case1_oracle(net, variant, emulate):
    """B = 4 once per (network, variant, arithmetic); the B = 3 case is its first three rows (samples are independent)."""
    key = ("case1", net, variant, emulate)
    if key not in _oracle:
        x = torch.from_numpy(images_np(_channels(net), 4))
        noise = tensor_noise(len(timestep_list(NOISE_STEPS, K)), x.shape) if variant == "cddpm" else None
        _oracle[key] = (x, noise, _oracle_denoise(net, variant, x, noise, emulate))
    return _oracle[key]


@pytest.mark.parametrize("compute", ["f16x3", "f32", "f16"])
@pytest.mark.parametrize("B", [4, 3])
@pytest.mark.parametrize("net", ["NET2", "NET3"])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_reference_update_with_tensor_noise_matches_the_oracle(variant, net, B, compute):
    """out_conv_kernel<0> with a.x != null (and, cddpm, a.noise): iteration i of sub-batch program h reads its noise at
    i * B*C*H*W + h * (B/2)*C*H*W, so a slice that forgets C shows at i >= 1 (B = 3) and h = 1 (B = 4: two programs of 2)."""
    x, noise, want = _case1_oracle(net, variant, False)
    den = _den(net, variant, compute)
    kw = {} if noise is None else dict(step_noise=noise[:, :B].contiguous().cuda())
    got = den.denoise(x[:B].cuda(), K, **kw).cpu().numpy()
    err = distance(got, want[:B])[0]
    print(f"case 1 {variant} {net} B={B} {compute}: max|hip - oracle| = {err:.3e}")
    assert np.isfinite(got).all()
    if compute == "f16":
        emu = _case1_oracle(net, variant, True)[2]
        gate(got, want[:B], *distance(emu[:B], want[:B]), f"case 1 {variant} {net} B={B}")
    else:
        assert err < TOL_FINAL


# ------------------------------------------------------------------------------ 2. seeded == its replay
@pytest.mark.parametrize("no_split", [False, True])
@pytest.mark.parametrize("compute,B", [("f16x3", 1), ("f16x3", 3), ("f16x3", 4), ("f32", 1), ("f32", 3), ("f32", 4), ("f16", 4)])
@pytest.mark.parametrize("net", ["NET2", "NET3", "NET4"])
def test_seeded_run_equals_its_replay_bit_for_bit(net, compute, B, no_split):
    """out_conv_seeded_kernel<0>: the fused draw's element index oc * H*W + y * W + x against midd_amd.step_noise, which
    tests/test_gpu_step_noise.py holds to the float64 specification at C = 2."""
    den = _den(net, "cddpm", compute)
    x = _images(net, B)
    steps = timestep_list(NOISE_STEPS, K)
    seeded = _sampler(den, x, steps, no_split=no_split, seed=SEED)
    replay = _sampler(den, x, steps, no_split=no_split, step_noise=midd_amd.step_noise(SEED, len(steps), x.shape))
    assert torch.isfinite(seeded).all() and torch.equal(seeded, replay), float((seeded - replay).abs().max())
    assert not torch.equal(seeded, _sampler(den, x, steps, no_split=no_split, seed=SEED + 1))
    if not no_split:
        assert torch.equal(den.denoise(x, K, seed=SEED), seeded)


@pytest.mark.parametrize("net", ["NET2", "NET3", "NET4"])
def test_a_block_of_the_batch_with_its_offset_equals_the_block_of_the_whole(net):
    den = _den(net, "cddpm", batch_invariant=True)
    x = _images(net, 4)
    whole = den.denoise(x, K, seed=SEED)
    assert torch.equal(den.denoise(x[1:3], K, seed=SEED, sample_offset=1), whole[1:3])
    assert not torch.equal(den.denoise(x[1:3], K, seed=SEED), whole[1:3])


# ------------------------------------------------------------------------------ 3. the reference update, restated bit for bit
@pytest.mark.parametrize("t", [48, 24])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("net", ["NET3", "NET4"])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_reference_update_equals_its_restatement_bit_for_bit(variant, net, B, t):
    """The control of tests/test_gpu_ddim_update.py on out_conv_kernel<0>: eps from `forward` (the same kernel with a.x == null),
    then c1 * fma(-c2, eps, x) and the clamp -- the contraction hipcc makes in out_conv_kernel<1> (profiles/step_noise_isa.txt)."""
    den = _den(net, variant, batch_invariant=True)
    clamp_eps = variant == "ddim"
    cond = torch.from_numpy(stretched_np(_channels(net), B)).cuda()
    eps = den.model(cond, cond, torch.full((B,), t, dtype=torch.long)).cpu().numpy()
    got = _sampler(den, cond, [t], no_split=True).cpu().numpy()
    want = _reference_restated(cond.cpu().numpy(), eps, t, den, clamp_eps)
    assert got.shape == (B, _channels(net), H, W)
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    assert 0.0 < float((got != cond.cpu().numpy()).mean())


# ------------------------------------------------------------------------------ 4. the DDIM(eta) update
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("clip_x0", [True, False])
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("net", ["NET3", "NET4"])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_ddim_update_equals_the_numpy_restatement_bit_for_bit(variant, net, eta, clip_x0, B):
    """tests/test_gpu_ddim_update.py: test_update_equals_the_numpy_restatement_bit_for_bit on out_conv_ddim_kernel<0>, the noise
    shaped (2, B, C, H, W).  The share of pixels whose predicted image the clip changes was computed beforehand on the CPU with the
    restatement over the oracle for these very inputs: 0.16 .. 0.38 over every network, variant, eta, batch and list used here
    (at least 0.07 in every single channel), so the cap 0.01 .. 0.99 below is met by the reference alone with a wide margin."""
    C = _channels(net)
    den = _den(net, variant, batch_invariant=True)
    clamp_eps = variant == "ddim"
    x_np = stretched_np(C, B)
    cond = torch.from_numpy(x_np).cuda()
    alpha_hat = den.alpha_hat.cpu().numpy()
    noise = tensor_noise(2, (B, C, H, W)).cuda()

    def model_eps(x, t):
        xt = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        return den.model(xt, cond, torch.full((B,), t, dtype=torch.long)).cpu().numpy()

    eps48, eps24 = model_eps(x_np, 48), model_eps(x_np, 24)
    kw = dict(no_split=True, update="ddim", eta=eta, clip_x0=clip_x0)
    rows = dref.coefficients([24], alpha_hat, eta)
    want, mask = dref.update(x_np, eps24, rows[0], clamp_eps, clip_x0, last=True, noise=noise[0].cpu().numpy())
    got = _sampler(den, cond, [24], step_noise=noise[:1].contiguous(), **kw).cpu().numpy()
    masks = [float(mask.mean())]
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    rows = dref.coefficients([48, 24], alpha_hat, eta)
    x1, mask = dref.update(x_np, eps48, rows[0], clamp_eps, clip_x0, last=False, noise=noise[0].cpu().numpy())
    masks.append(float(mask.mean()))
    assert x1.max() > 1.0
    want, mask = dref.update(x1, model_eps(x1, 24), rows[1], clamp_eps, clip_x0, last=True, noise=noise[1].cpu().numpy())
    got = _sampler(den, cond, [48, 24], step_noise=noise, **kw).cpu().numpy()
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    print(f"case 4 {variant} {net} eta {eta} clip {clip_x0} B={B}: clip changed x0 on {masks[0]:.3f} ([24]) and {masks[1]:.3f} ([48, 24]) of the pixels")
    if clip_x0:
        assert all(0.01 <= m <= 0.99 for m in masks), masks
    else:
        assert masks == [0.0, 0.0]
    if eta == 1.0:                                        # the noise term is really there, and every channel's own
        assert not np.array_equal(_sampler(den, cond, [48, 24], **kw).cpu().numpy(), got)
        rolled = noise.roll(1, dims=2).contiguous()
        assert not np.array_equal(_sampler(den, cond, [48, 24], step_noise=rolled, **kw).cpu().numpy(), got)


@pytest.mark.parametrize("no_split", [False, True])
@pytest.mark.parametrize("B", [3, 4])
@pytest.mark.parametrize("net", ["NET3", "NET4"])
def test_seeded_ddim_update_equals_its_replay_bit_for_bit(net, B, no_split):
    """out_conv_ddim_seeded_kernel<0>."""
    den = _den(net, "cddpm")
    x = _images(net, B)
    steps = timestep_list(NOISE_STEPS, K)
    kw = dict(no_split=no_split, update="ddim", eta=1.0)
    seeded = _sampler(den, x, steps, seed=SEED, **kw)
    replay = _sampler(den, x, steps, step_noise=midd_amd.step_noise(SEED, len(steps), x.shape), **kw)
    assert torch.isfinite(seeded).all() and torch.equal(seeded, replay), float((seeded - replay).abs().max())
    assert float(seeded.min()) >= 0.0 and float(seeded.max()) <= 1.0


# ------------------------------------------------------------------------------ 5. slots
@pytest.mark.parametrize("B", [1, 3, 4])
@pytest.mark.parametrize("net", ["NET2", "NET4"])
@pytest.mark.parametrize("mode", ["ddim", "seeded", "replay"])
def test_uniform_slot_table_equals_denoise_bit_for_bit(mode, net, B):
    """out_conv_slots_kernel<0> against out_conv_kernel<0> / out_conv_seeded_kernel<0>: the plain form (DDIM), the seeded form and the
    replay through a (n_rows, B, C, H, W) tensor (cddpm)."""
    den = _den(net, "ddim" if mode == "ddim" else "cddpm")
    img = _images(net, B)
    t_list = timestep_list(NOISE_STEPS, K)
    rows = [[t] * B for t in t_list]
    kw = {}
    if mode == "seeded":
        kw = dict(seed=SEED)
    elif mode == "replay":
        kw = dict(step_noise=midd_amd.step_noise(SEED ^ 5, len(t_list), img.shape))
        assert kw["step_noise"].shape == (len(t_list), B, _channels(net), H, W)
    want = den.denoise(img, K, **kw)
    x = img.clone()
    got = _run_slots(den, img, x, rows, **kw)
    assert got is x and torch.isfinite(got).all() and not torch.equal(got, img)
    assert torch.equal(got, want), float((got - want).abs().max())


RAGGED = (5, 2, 3, 1)


@pytest.mark.parametrize("net", ["NET2", "NET4"])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_ragged_equals_the_single_image_runs_bit_for_bit(variant, net):
    den = _den(net, variant, batch_invariant=True)
    img = _images(net, len(RAGGED))
    got = den.denoise_ragged(img, RAGGED, seed=SEED, sample_offset=2)
    assert got.shape == img.shape and torch.isfinite(got).all()
    for b, k in enumerate(RAGGED):
        want = den.denoise(img[b:b + 1], k, seed=SEED, sample_offset=2 + b)
        assert torch.equal(got[b:b + 1], want), (b, k, float((got[b:b + 1] - want).abs().max()))


@pytest.mark.parametrize("net", ["NET2", "NET4"])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_an_idle_slot_keeps_the_bits_of_all_its_channels(variant, net):
    den = _den(net, variant, batch_invariant=True)
    C = _channels(net)
    img = _images(net, 4, seed=21)
    t_list = timestep_list(NOISE_STEPS, 3)
    rows = [[t, -1, t, -1] for t in t_list]
    x = img.clone()
    ramp = torch.linspace(0.0, 1.0, H * W, device="cuda").reshape(H, W)
    for c in range(C):                                        # another pattern per channel
        x[1, c] = (ramp * (c + 1)) % 1.0
        x[3, c] = 0.125 * (c + 1)
    before = x.clone()
    _run_slots(den, img, x, rows, seed=SEED if variant == "cddpm" else None)
    assert torch.equal(x[1], before[1]) and torch.equal(x[3], before[3])
    for b in (0, 2):
        want = den.denoise(img[b:b + 1], 3, seed=SEED, sample_offset=b)
        assert torch.equal(x[b:b + 1], want), b


def test_ragged_stays_within_the_parity_gate_of_the_oracle():
    """NET2, cddpm, the default (not batch-invariant) plan; the oracle is fed the exported seeded noise of every image's own index."""
    net, variant = "NET2", "cddpm"
    den = _den(net, variant)
    img = _images(net, len(RAGGED))
    got = den.denoise_ragged(img, RAGGED, seed=SEED).cpu().numpy()
    worst = 0.0
    for b, k in enumerate(RAGGED):
        n = len(timestep_list(NOISE_STEPS, k))
        noise = midd_amd.step_noise(SEED, n, (1,) + tuple(img.shape[1:]), sample_offset=b).cpu()
        want = _oracle_denoise(net, variant, img[b:b + 1].cpu(), noise, steps=k)
        err = distance(got[b:b + 1], want)[0]
        print(f"case 5 ragged {variant} {net} image {b} steps {k}: max|hip - oracle| = {err:.3e}")
        worst = max(worst, err)
    assert worst < TOL_FINAL


# ------------------------------------------------------------------------------ 6. ensemble
@pytest.mark.parametrize("max_batch", [2, 16])
def test_ensemble_members_and_maps(max_batch):
    """B * members = 6 virtual samples, image-major: passes of 2 cut image 0's members after the second and image 1's after the
    first.  The condition broadcast, the member stores and the reduce all stride by C*H*W."""
    net, B, M = "NET2", 2, 3
    C = _channels(net)
    den = _den(net, "cddpm", batch_invariant=True)
    x = _images(net, B)
    res = den.denoise_ensemble(x, K, members=M, seed=SEED, max_batch=max_batch, return_samples=True, quantiles=LEVELS)
    assert res.samples.shape == (B, M, C, H, W) and res.mean.shape == res.std.shape == x.shape and res.quantiles.shape == (B, len(LEVELS), C, H, W)
    assert torch.isfinite(res.samples).all()
    n_iters = len(timestep_list(NOISE_STEPS, K))
    for m in range(M):
        assert torch.equal(res.samples[:, m], den.denoise(x, K, seed=SEED, member=m)), m
        # ... and its replay through the exported noise of that member: the draw's channel index against midd_amd.step_noise
        replay = den.denoise(x, K, step_noise=midd_amd.step_noise(SEED, n_iters, x.shape, member=m))
        assert torch.equal(res.samples[:, m], replay), (m, float((res.samples[:, m] - replay).abs().max()))
    assert not torch.equal(res.samples[:, 0], res.samples[:, 1])
    mean, std = midd_amd.ensemble_reduce(res.samples)
    assert torch.equal(res.mean, mean) and torch.equal(res.std, std)
    assert torch.equal(res.quantiles, midd_amd.ensemble_quantiles(res.samples, LEVELS))
    samples = res.samples.cpu().numpy()
    want_mean, want_std = eref.reduce(samples)
    assert np.array_equal(res.mean.cpu().numpy(), want_mean)
    assert np.array_equal(res.std.cpu().numpy(), want_std), float(np.abs(res.std.cpu().numpy() - want_std).max())
    assert np.array_equal(res.quantiles.cpu().numpy().view(np.uint32), qref.quantiles(samples, LEVELS).view(np.uint32))


# ------------------------------------------------------------------------------ 7. tiled
def _tile_crops(x):
    Hi, Wi, T, O = TILED
    return midd_amd.tile_extract(x, T, O).reshape(-1, x.shape[1], T, T)


def _noise_crops(x, n_iters, member=0):
    """[n_iters, B * tiles, C, T, T]: a tile's noise at channel c is the image's at (c * H_img + y0 + y) * W_img + x0 + x."""
    Hi, Wi, T, O = TILED
    plan = midd_amd.tile_plan(Hi, Wi, T, O)
    field = midd_amd.step_noise(SEED, n_iters, x.shape, sample_offset=OFFSET, member=member)
    crops = [field[:, b, :, y0:y0 + T, x0:x0 + T] for b in range(x.shape[0]) for y0 in plan.origins_y for x0 in plan.origins_x]
    return torch.stack(crops, dim=1).contiguous()


@pytest.mark.parametrize("max_batch", [3, 16])
@pytest.mark.parametrize("net", ["NET2", "NET3"])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_tiles_are_functions_of_their_crops_and_blend_to_the_image(variant, net, max_batch):
    Hi, Wi, T, O = TILED
    C = _channels(net)
    den = _den(net, variant, batch_invariant=True)
    x = _images(net, 2, Hi, Wi)
    plan = midd_amd.tile_plan(Hi, Wi, T, O)
    assert (plan.origins_y, plan.origins_x) == ((0, 24), (0, 20, 40))
    kw = dict(seed=SEED, sample_offset=OFFSET) if variant == "cddpm" else {}
    res = den.denoise_tiled(x, K, tile=T, overlap=O, max_batch=max_batch, return_tiles=True, **kw)
    assert res.tiles.shape == (2, 6, C, T, T) and res.image.shape == x.shape and torch.isfinite(res.image).all()
    crops = _tile_crops(x)
    assert np.array_equal(crops.cpu().numpy(), tref.extract(x.cpu().numpy(), (T, T), (O, O)).reshape(12, C, T, T))
    n_iters = len(timestep_list(NOISE_STEPS, K))
    alone = den.denoise(crops, K, **({"step_noise": _noise_crops(x, n_iters)} if variant == "cddpm" else {}))
    for v in range(12):
        assert torch.equal(res.tiles.reshape(12, C, T, T)[v], alone[v]), (v, float((res.tiles.reshape(12, C, T, T)[v] - alone[v]).abs().max()))
    assert torch.equal(res.image, midd_amd.tile_blend(res.tiles, Hi, Wi, O))
    assert np.array_equal(res.image.cpu().numpy(), tref.blend(res.tiles.cpu().numpy(), Hi, Wi, (O, O)))


@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_tiled_call_matches_the_oracle_run_tile_by_tile(variant):
    Hi, Wi, T, O = TILED
    net = "NET2"
    den = _den(net, variant)
    x = _images(net, 2, Hi, Wi)
    kw = dict(seed=SEED, sample_offset=OFFSET) if variant == "cddpm" else {}
    res = den.denoise_tiled(x, K, tile=T, overlap=O, return_tiles=True, **kw)
    crops = torch.from_numpy(tref.extract(x.cpu().numpy(), (T, T), (O, O)).reshape(12, 2, T, T))
    noise = _noise_crops(x, len(timestep_list(NOISE_STEPS, K))).cpu() if variant == "cddpm" else None
    want_tiles = _oracle_denoise(net, variant, crops, noise).reshape(2, 6, 2, T, T)
    err_tiles = distance(res.tiles.cpu().numpy(), want_tiles)[0]
    err_image = distance(res.image.cpu().numpy(), tref.blend(want_tiles, Hi, Wi, (O, O)))[0]
    print(f"case 7 {variant} {net}: tiles max|hip - oracle| = {err_tiles:.3e}, blended image {err_image:.3e}")
    assert err_tiles < TOL_FINAL and err_image < TOL_FINAL


# ------------------------------------------------------------------------------ 8. tiled ensemble
def test_tiled_ensemble_members_and_maps():
    Hi, Wi, T, O = TILED
    net, M = "NET2", 2
    C = _channels(net)
    den = _den(net, "cddpm", batch_invariant=True)
    x = _images(net, 1, Hi, Wi)
    kw = dict(tile=T, overlap=O, seed=SEED, sample_offset=OFFSET, return_tiles=True)
    res = den.denoise_tiled_ensemble(x, K, members=M, return_samples=True, **kw)
    assert res.tiles.shape == (M, 1, 6, C, T, T) and res.samples.shape == (1, M, C, Hi, Wi) and res.mean.shape == res.std.shape == x.shape
    one = den.denoise_tiled(x, K, **kw)
    assert torch.equal(res.tiles[0], one.tiles) and torch.equal(res.samples[:, 0], one.image)
    n_iters = len(timestep_list(NOISE_STEPS, K))
    alone = den.denoise(_tile_crops(x), K, step_noise=_noise_crops(x, n_iters, member=1))
    assert torch.equal(res.tiles[1].reshape(6, C, T, T), alone)
    assert not torch.equal(res.tiles[0], res.tiles[1])
    mean, std, samples = midd_amd.tile_blend_reduce(res.tiles, Hi, Wi, O, return_samples=True)
    assert torch.equal(res.mean, mean) and torch.equal(res.std, std) and torch.equal(res.samples, samples)


# ------------------------------------------------------------------------------ 9. self-ensemble
@pytest.mark.parametrize("shape,views", [((2, 40, 24), "flips"), ((1, 40, 40), "d4")])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_a_self_ensemble_member_is_denoise_of_the_view_turned_back(variant, shape, views):
    net = "NET2"
    C = _channels(net)
    B, h, w = shape
    den = _den(net, variant, batch_invariant=True)
    x = _images(net, B, h, w)
    kw = dict(seed=SEED, sample_offset=4, member_offset=3) if variant == "cddpm" else {}
    res = den.denoise_self_ensemble(x, K, views=views, max_batch=3, return_samples=True, **kw)
    codes = sref.FLIPS if views == "flips" else sref.D4
    assert res.views == codes and res.samples.shape == (B, len(codes), C, h, w) and res.mean.shape == res.std.shape == x.shape
    for b in range(B):
        for k, g in enumerate(codes):
            one = dict(seed=SEED, sample_offset=4 + b, member=3 + k) if variant == "cddpm" else {}
            alone = den.denoise(_view_t(x[b:b + 1], g), K, **one)
            assert torch.equal(res.samples[b, k], _unview_t(alone, g)[0]), (b, k, g)
    assert not torch.equal(res.samples[:, 0], res.samples[:, 1])
    want_mean, want_std = eref.reduce(res.samples.cpu().numpy())
    assert np.array_equal(res.mean.cpu().numpy(), want_mean)
    assert np.array_equal(res.std.cpu().numpy(), want_std), float(np.abs(res.std.cpu().numpy() - want_std).max())


def test_ddim_self_ensemble_matches_the_oracle():
    net = "NET2"
    den = _den(net, "ddim")
    x = _images(net, 2)
    res = den.denoise_self_ensemble(x, K, views="flips", return_samples=True)
    xn = x.cpu().numpy()
    outs = np.stack([_oracle_denoise(net, "ddim", torch.from_numpy(np.stack([sref.view(xn[b], g) for b in range(2)]))) for g in sref.FLIPS], axis=1)
    want_mean, _, want_members = sref.reduce(outs, sref.FLIPS)
    err_m = distance(res.samples.cpu().numpy(), want_members)[0]
    err_mean = distance(res.mean.cpu().numpy(), want_mean)[0]
    print(f"case 9 ddim {net} flips: members max|hip - oracle| = {err_m:.3e}, mean {err_mean:.3e}")
    assert err_m < TOL_FINAL and err_mean < TOL_FINAL


# ------------------------------------------------------------------------------ 10. the status word
def test_a_nan_in_one_channel_of_one_image_is_reported():
    net = "NET3"
    den = _den(net, "ddim", batch_invariant=True)
    x = _images(net, 3)
    clean = den.denoise(x, K)
    bad = x.clone()
    bad[1, 2, 7, 5] = float("nan")                            # image 1, channel 2 only
    with pytest.raises(native.MiddError) as ei:
        den.denoise(bad, K)
    assert ei.value.code == -5 and "non-finite" in str(ei.value)
    den.model.check_status = False
    try:
        out = den.denoise(bad, K)
        torch.cuda.synchronize()
    finally:
        den.model.check_status = True
    assert torch.equal(out[0], clean[0]) and torch.equal(out[2], clean[2])
    assert torch.equal(den.denoise(x, K), clean)              # the next call starts from a cleared word
