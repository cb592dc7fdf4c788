"""GPU: the geometric self-ensemble (include/midd.h: THE GEOMETRY, mi_dihedral_views, mi_dihedral_reduce, mi_dihedral_quantiles,
mi_denoise_self_ensemble; DiffusionDenoiser.denoise_self_ensemble).

The fill is a copy and the reduce's arithmetic is fixed, so the three kernels are compared bit for bit (as int32) with the numpy
restatement (tests/self_ensemble_reference.py) on the smallest shapes that reach each path: below one 32 x 32 tile, odd sizes
(dword path, partial tiles on both axes), 16-byte path with full and partial tiles, non-square lists, unaligned bases.  A view is
one more sample of the unchanged sampler: with a batch-invariant plan member k is `unview(denoise(view(x)))` bit for bit, for
both variants and whatever the pass size, and the whole call agrees with the oracle run on every numpy view."""
import ctypes as C

import numpy as np
import pytest
import torch
from PIL import Image

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, timestep_list, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import self_ensemble_reference as sref

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # north_star: |delta| < 1e-3 fp32 per pixel (tests/test_gpu_parity.py)
TOL_STD = 1.5e-3          # unbiased std over K values moves by at most sqrt(K / (K - 1)) <= 1.42 x the largest member error (tests/test_gpu_ensemble.py)
SEED = 0x1234567890ABCDEF
K_STEPS = 5               # inference_steps of the sampler cases
LEVELS = (0.0, 0.05, 0.5, 0.95, 1.0)
QNAN = 0x7FC00000

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
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models[key]


def _images(B, H=64, W=64, seed=77):
    return torch.from_numpy(synthetic_xray(B, H, W, seed=seed)).cuda()


def _seed_kw(variant):
    return dict(seed=SEED) if variant == "cddpm" else {}


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int32)


def _same_bits(got, want, what):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    assert np.array_equal(g, w), (what, int((g != w).sum()), "elements differ")


def _view_t(x, g):
    """view() of the specification on a torch tensor [..., H, W] (the caller's spelling today)."""
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


# ------------------------------------------------------------------------------ 1. the kernels alone
def _check_kernels(shape, codes, unaligned=False, seed=0):
    B, Cc, H, W = shape
    G = len(codes)
    rng = np.random.default_rng(seed + H * W)
    x = rng.random(shape, dtype=np.float32)
    vo = rng.random((B, G, Cc, H, W), dtype=np.float32)
    mid = (slice(H // 4, H - H // 4), slice(W // 4, W - W // 4))             # a centred block: every view maps it onto itself
    vo[(0, slice(None), 0) + mid] = np.float32(0.25)                         # ... constant over the members there: mean 0.25, std 0

    def dev(a):
        """On the device; `unaligned`: the base address is 4 bytes past a 16-byte boundary."""
        if not unaligned:
            return torch.from_numpy(a).cuda()
        flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = torch.from_numpy(a.reshape(-1)).cuda()
        t = flat[1:].view(a.shape)
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        return t
    _same_bits(midd_amd.dihedral_views(dev(x), codes), sref.views(x, codes), "views")
    mean, std, samples = midd_amd.dihedral_reduce(dev(vo), codes)
    want_mean, want_std, want_samples = sref.reduce(vo, codes)
    _same_bits(samples, want_samples, "samples")
    _same_bits(mean, want_mean, "mean")
    if G >= 2:
        ulps = int(np.abs(_bits(std).astype(np.int64) - _bits(want_std).astype(np.int64)).max())
        print(f"dihedral_reduce {shape} {codes}: std max distance to the float64 restatement = {ulps} ulp")
        _same_bits(std, want_std, "std")
        assert not _bits(std)[(0, 0) + mid].any() and (_bits(mean)[(0, 0) + mid] == np.float32(0.25).view(np.int32)).all()
        assert _bits(std).any(axis=(-1, -2)).all()
    else:
        assert std is None
    # ... which is unview per view followed by mi_ensemble_reduce, and the same bits without the samples
    m2, s2 = midd_amd.ensemble_reduce(samples)
    assert torch.equal(m2, mean) and (std is None or torch.equal(s2, std))
    quiet = midd_amd.dihedral_reduce(dev(vo), codes, return_samples=False)
    assert quiet[2] is None and torch.equal(quiet[0], mean) and (std is None or torch.equal(quiet[1], std))
    q = midd_amd.dihedral_quantiles(dev(vo), codes, LEVELS)
    _same_bits(q, sref.quantiles(vo, codes, LEVELS), "quantiles")
    assert torch.equal(q, midd_amd.ensemble_quantiles(samples, LEVELS))


@pytest.mark.parametrize("shape,codes", [
    ((2, 1, 8, 8), sref.D4),                     # smaller than one tile
    ((1, 3, 33, 33), sref.D4),                   # odd size: dword path, a partial tile on both axes, several channels
    ((2, 1, 72, 72), sref.D4),                   # 16-byte path, two full 32-pixel tiles and a partial one per axis
    ((3, 1, 5, 7), sref.FLIPS),                  # dword path, non-square
    ((2, 2, 40, 104), sref.FLIPS),               # 16-byte path, non-square, partial tiles
    ((1, 1, 64, 64), (0, 5, 6, 3)),              # list order
    ((1, 1, 64, 64), (3, 6, 5, 0)),
    ((2, 1, 40, 40), (6,)),                      # one view: no std
])
def test_kernels_match_the_restatement_bit_for_bit(shape, codes):
    _check_kernels(shape, codes)


@pytest.mark.parametrize("shape,codes", [((2, 1, 72, 72), sref.D4), ((2, 2, 40, 104), sref.FLIPS)])
def test_an_unaligned_base_gives_the_same_bits(shape, codes):
    """The same checks against the same restatement with every input 4 bytes past a 16-byte boundary: the dword path at a shape
    whose aligned run takes the 16-byte path."""
    _check_kernels(shape, codes, unaligned=True)


def test_list_order_permutes_the_members_and_orders_the_sums():
    rng = np.random.default_rng(5)
    vo = rng.random((1, 4, 1, 64, 64), dtype=np.float32)
    a, b = (0, 5, 6, 3), (3, 6, 5, 0)
    ra = midd_amd.dihedral_reduce(torch.from_numpy(vo).cuda(), a)
    rb = midd_amd.dihedral_reduce(torch.from_numpy(np.ascontiguousarray(vo[:, ::-1])).cuda(), b)      # the same view outputs, listed backwards
    assert torch.equal(ra[2], rb[2].flip(1))                                 # the members permute with the list
    for r, v, codes in ((ra, vo, a), (rb, np.ascontiguousarray(vo[:, ::-1]), b)):      # each against the restatement, not against each other
        want = sref.reduce(v, codes)
        _same_bits(r[0], want[0], "mean")
        _same_bits(r[1], want[1], "std")
    assert float((ra[0] - rb[0]).abs().max()) <= 2.0 ** -23                  # the sum order is the list order: equal to the last bits only


def test_views_windows():
    lib = native.lib()
    B, Cc, H, W, codes = 2, 2, 40, 40, sref.D4
    x = np.random.default_rng(9).random((B, Cc, H, W), dtype=np.float32)
    want = sref.views(x, codes).reshape(B * 8, Cc, H, W)
    src = torch.from_numpy(x).cuda()
    arr = (C.c_int32 * 8)(*codes)
    stream = torch.cuda.current_stream().cuda_stream
    for v0, n in [(5, 6), (3, 1), (0, 16), (15, 1), (8, 8)]:                 # windows that start and end inside an image's views
        dst = torch.full((n, Cc, H, W), -7.0, device="cuda")
        assert lib.mi_dihedral_views(src.data_ptr(), B, Cc, H, W, arr, 8, v0, n, dst.data_ptr(), stream) == 0, lib.mi_last_error()
        _same_bits(dst, want[v0:v0 + n], (v0, n))
    dst = torch.full((1, Cc, H, W), -7.0, device="cuda")
    assert lib.mi_dihedral_views(src.data_ptr(), B, Cc, H, W, arr, 8, 4, 0, dst.data_ptr(), stream) == 0      # n = 0: MI_OK, nothing written
    torch.cuda.synchronize()
    assert float(dst.min()) == -7.0 and float(dst.max()) == -7.0
    assert lib.mi_dihedral_views(src.data_ptr(), B, Cc, H, W, arr, 8, 11, 6, dst.data_ptr(), stream) == -1


def test_special_values():
    rng = np.random.default_rng(13)
    codes = sref.D4
    vo = rng.random((1, 8, 1, 33, 33), dtype=np.float32)
    specials = np.array([-0.0, 0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), 1e-45, -1e-45], np.float32)
    vo[0, :, 0, 4, :6] = specials                                            # signed zeros, the clamp values, denormals
    vo[0, 3, 0, 20, 11] = np.float32("nan")                                  # one NaN member, in view 3's frame
    mean, std, samples = midd_amd.dihedral_reduce(torch.from_numpy(vo).cuda(), codes)
    want = sref.members(vo, codes)
    _same_bits(samples, want, "samples")                                     # every bit pattern passes through
    for s in specials:
        assert (_bits(samples) == s.view(np.int32)).sum() == 8
    nan_at = np.argwhere(np.isnan(want[0, 3, 0]))
    assert nan_at.shape == (1, 2)
    y, x = nan_at[0]                                                         # where unview puts it: (32 - 20, 32 - 11)
    assert (y, x) == (12, 21)
    m = mean.cpu().numpy()
    assert np.isnan(m[0, 0, y, x]) and np.isnan(m).sum() == 1 and np.isnan(std.cpu().numpy()).sum() == 1
    q = midd_amd.dihedral_quantiles(torch.from_numpy(vo).cuda(), codes, LEVELS)
    assert (_bits(q)[0, :, 0, y, x] == QNAN).all() and np.isnan(q.cpu().numpy()).sum() == len(LEVELS)
    _same_bits(q, sref.quantiles(vo, codes, LEVELS), "quantiles")


# ------------------------------------------------------------------------------ 2. a member is the sampler's run of the turned image
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_a_member_is_denoise_of_the_view_turned_back(variant):
    """B * 8 = 16 virtual samples: one pass of 16, and passes of 5 whose boundaries fall inside an image's views."""
    den = _model(variant, batch_invariant=True)
    B = 2
    x = _images(B)
    res = den.denoise_self_ensemble(x, inference_steps=K_STEPS, max_batch=16, return_samples=True, **_seed_kw(variant))
    assert res.views == sref.D4 and res.samples.shape == (B, 8, 1, 64, 64) and res.mean.shape == x.shape and res.std.shape == x.shape
    assert res.seed == (SEED if variant == "cddpm" else None) and torch.isfinite(res.samples).all()
    for b in range(B):
        for k, g in enumerate(res.views):
            kw = dict(seed=SEED, sample_offset=b, member=k) if variant == "cddpm" else {}
            alone = den.denoise(_view_t(x[b:b + 1], g), inference_steps=K_STEPS, **kw)
            assert torch.equal(res.samples[b, k], _unview_t(alone, g)[0]), (variant, b, k, g)
    assert not torch.equal(res.samples[0, 0], res.samples[0, 5])
    small = den.denoise_self_ensemble(x, inference_steps=K_STEPS, max_batch=5, return_samples=True, **_seed_kw(variant))
    assert torch.equal(small.samples, res.samples) and torch.equal(small.mean, res.mean) and torch.equal(small.std, res.std)
    # without the samples the statistics are the same bits
    quiet = den.denoise_self_ensemble(x, inference_steps=K_STEPS, max_batch=5, **_seed_kw(variant))
    assert quiet.samples is None and torch.equal(quiet.mean, res.mean) and torch.equal(quiet.std, res.std)
    if variant == "cddpm":      # member_offset shifts the member words: a list of two views draws as members 3 and 4
        two = den.denoise_self_ensemble(x, inference_steps=K_STEPS, views=(6, 1), seed=SEED, sample_offset=4, member_offset=3, return_samples=True)
        for k, g in enumerate((6, 1)):
            alone = den.denoise(_view_t(x[1:2], g), inference_steps=K_STEPS, seed=SEED, sample_offset=5, member=3 + k)
            assert torch.equal(two.samples[1, k], _unview_t(alone, g)[0]), (k, g)


@pytest.mark.parametrize("compute", ["f16x3", "f32", "f16"])
def test_the_identity_view_alone_is_denoise(compute):
    for variant in ("ddim", "cddpm"):
        den = _model(variant, compute)
        x = _images(4)
        res = den.denoise_self_ensemble(x, inference_steps=K_STEPS, views=(0,), return_samples=True, **_seed_kw(variant))
        plain = den.denoise(x, inference_steps=K_STEPS, **_seed_kw(variant))
        assert res.std is None and res.views == (0,)
        assert torch.equal(res.samples[:, 0], plain) and torch.equal(res.mean, plain), (variant, compute)


# ------------------------------------------------------------------------------ 3. against the oracle
def _oracle_self_ensemble(variant, x, codes, noise_of=None):
    """oracle/ddim_oracle.py on every numpy view of every image, unview, numpy reduce -> (mean, std, members)."""
    sd_t, topo = orc.to_torch(_sd(variant)), topology(UNetConfig(variant=variant))
    xn = x.cpu().numpy()
    B = xn.shape[0]
    outs = np.empty((B, len(codes)) + sref.view(xn[0], codes[0]).shape, np.float32)
    for k, g in enumerate(codes):
        turned = torch.from_numpy(np.stack([sref.view(xn[b], g) for b in range(B)]))
        noise = None if noise_of is None else noise_of(k, turned.shape)
        outs[:, k] = orc.denoise(sd_t, topo, turned, 50, K_STEPS, step_noise=noise).numpy()
    return sref.reduce(outs, codes)


def _gate(res, want, what):
    want_mean, want_std, want_members = want
    err_m = float(np.abs(res.samples.cpu().numpy().astype(np.float64) - want_members).max())
    err_mean = float(np.abs(res.mean.cpu().numpy().astype(np.float64) - want_mean).max())
    err_std = float(np.abs(res.std.cpu().numpy().astype(np.float64) - want_std).max())
    print(f"{what} vs oracle: members max|delta| = {err_m:.3e}, mean {err_mean:.3e}, std {err_std:.3e}")
    assert err_m < TOL_FINAL and err_mean < TOL_FINAL
    assert err_std < TOL_STD


def test_ddim_square_matches_the_oracle():
    den = _model("ddim")
    x = _images(2)
    res = den.denoise_self_ensemble(x, inference_steps=K_STEPS, return_samples=True)
    _gate(res, _oracle_self_ensemble("ddim", x, sref.D4), "ddim 2 x 64x64, 8 views")


def test_ddim_non_square_matches_the_oracle():
    den = _model("ddim")
    x = _images(1, 40, 104)
    res = den.denoise_self_ensemble(x, inference_steps=K_STEPS, views="auto", return_samples=True)
    assert res.views == sref.FLIPS
    _gate(res, _oracle_self_ensemble("ddim", x, sref.FLIPS), "ddim 1 x 40x104, flips")


def test_cddpm_matches_the_oracle_given_the_exported_noise():
    den = _model("cddpm")
    x = _images(1)
    n_iters = len(timestep_list(50, K_STEPS))
    res = den.denoise_self_ensemble(x, inference_steps=K_STEPS, seed=SEED, return_samples=True)

    def noise_of(k, shape):      # view k draws as member k, at the pixel's place in the view's frame
        return list(midd_amd.step_noise(SEED, n_iters, tuple(shape), member=k).cpu())
    _gate(res, _oracle_self_ensemble("cddpm", x, sref.D4, noise_of), "cddpm 1 x 64x64, 8 views")


# ------------------------------------------------------------------------------ 4. the returned statistics, quantiles, determinism
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_statistics_and_quantiles_are_those_of_the_returned_members(variant):
    den = _model(variant)
    x = _images(2)
    kw = dict(inference_steps=K_STEPS, return_samples=True, **_seed_kw(variant))
    res = den.denoise_self_ensemble(x, **kw)
    mean, std = midd_amd.ensemble_reduce(res.samples)
    assert torch.equal(res.mean, mean) and torch.equal(res.std, std)
    want_mean, want_std = sref.eref.reduce(res.samples.cpu().numpy())
    _same_bits(res.mean, want_mean, "mean")
    _same_bits(res.std, want_std, "std")
    withq = den.denoise_self_ensemble(x, quantiles=LEVELS, **kw)
    assert isinstance(withq, midd_amd.SelfEnsembleQuantileResult) and withq.levels == LEVELS and withq.quantiles.shape == (2, len(LEVELS), 1, 64, 64)
    assert torch.equal(withq.quantiles, midd_amd.ensemble_quantiles(res.samples, LEVELS))
    _same_bits(withq.quantiles, sref.qref.quantiles(res.samples.cpu().numpy(), LEVELS), "quantiles")
    assert torch.equal(withq.mean, res.mean) and torch.equal(withq.std, res.std) and torch.equal(withq.samples, res.samples)
    only = den.denoise_self_ensemble(x, inference_steps=K_STEPS, quantiles=(0.5,), **_seed_kw(variant))      # no samples tensor at all
    assert only.samples is None and torch.equal(only.quantiles[:, 0], withq.quantiles[:, 2]) and torch.equal(only.mean, res.mean)
    # the same call twice gives the same bits, on another stream too
    again = den.denoise_self_ensemble(x, **kw)
    assert torch.equal(again.samples, res.samples) and torch.equal(again.mean, res.mean) and torch.equal(again.std, res.std)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = den.denoise_self_ensemble(x, quantiles=LEVELS, **kw)
    side.synchronize()
    assert torch.equal(on_side.samples, res.samples) and torch.equal(on_side.std, res.std) and torch.equal(on_side.quantiles, withq.quantiles)
    if variant == "cddpm":
        drawn = den.denoise_self_ensemble(x, inference_steps=K_STEPS, return_samples=True)      # seed=None: drawn, and returned
        assert isinstance(drawn.seed, int) and 0 <= drawn.seed < 1 << 64
        repeat = den.denoise_self_ensemble(x, inference_steps=K_STEPS, return_samples=True, seed=drawn.seed)
        assert torch.equal(repeat.samples, drawn.samples) and not torch.equal(drawn.samples, res.samples)


# ------------------------------------------------------------------------------ 5. the status word accumulates over the passes
def test_a_nan_in_the_first_pass_is_still_reported_after_the_last():
    den = _model("ddim")
    m = den.model
    x = _images(3)
    bad = x.clone()
    bad[0, 0, 5, 7] = float("nan")                                            # image 0: virtual samples 0 .. 3 = the first pass of 4
    kw = dict(inference_steps=K_STEPS, views="flips", max_batch=4)
    assert torch.isfinite(den.denoise_self_ensemble(x, **kw).mean).all()       # clean input: no flag
    with pytest.raises(native.MiddError) as ei:
        den.denoise_self_ensemble(bad, **kw)
    assert ei.value.code == -5
    m.check_status = False
    try:
        res = den.denoise_self_ensemble(bad, **kw)
        torch.cuda.synchronize()
    finally:
        m.check_status = True
    assert torch.isfinite(res.mean[1:]).all() and torch.isfinite(res.std[1:]).all(), "the other images must not see image 0's NaN"
    assert torch.isfinite(den.denoise_self_ensemble(x, **kw).mean).all()       # the next call clears the word


# ------------------------------------------------------------------------------ 6. memory
def test_self_ensemble_call_allocates_its_workspace_and_outputs_only():
    den = _model("ddim")
    B, G, S = 1, 8, 256
    x = _images(B, S, S)
    img_bytes = B * S * S * 4
    ws_bytes = den.model.self_ensemble_workspace_bytes(B, G, S, S)
    assert ws_bytes == den.model.ensemble_workspace_bytes(B, G, S, S)
    assert ws_bytes >= den.model.workspace_bytes(8, S, S) + G * img_bytes + B * G * img_bytes      # the pass, its views, the view outputs
    assert den.model.self_ensemble_workspace_bytes(B, G, S, S, samples_external=True) == ws_bytes      # they stay in the workspace
    den.model._ensemble_ws = None                                              # the call below allocates its workspace
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = den.denoise_self_ensemble(x, inference_steps=K_STEPS)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    outputs = 2 * img_bytes
    print(f"peak rise across one self-ensemble call: {rise / 1e6:.1f} MB (workspace {ws_bytes / 1e6:.1f} MB, outputs {outputs / 1e6:.1f} MB)")
    assert torch.isfinite(res.mean).all() and res.samples is None
    assert rise <= ws_bytes + outputs + 4 * 2 ** 20
    # the sampler workspaces of earlier calls are still resident: the self-ensemble did not evict them
    cached = len(den.model._workspaces)
    den.denoise_self_ensemble(x[:, :, :64, :64].contiguous(), inference_steps=2, views="flips")
    assert len(den.model._workspaces) == cached


# ------------------------------------------------------------------------------ 7. CLI
def test_cli_self_ensemble_gives_the_same_png_and_std_map_twice(tmp_path, capsys):
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in _sd("ddim").items()}, "noise_steps": 50}, ckpt)
    png = tmp_path / "in.png"
    Image.fromarray((synthetic_xray(1, 88, 120, seed=9)[0, 0].clip(0, 1) * 255).astype(np.uint8), mode="L").save(png)
    from midd_amd import cli
    base = ["--image", str(png), "--checkpoint", str(ckpt), "--variant", "ddim", "--img-size", "64", "--inference-steps", str(K_STEPS)]
    outs, stds = [], []
    for i in range(2):
        out, std = tmp_path / f"out{i}.png", tmp_path / f"std{i}.npy"
        cli.main(base + ["--out", str(out), "--self-ensemble", "--std-out", str(std)])
        outs.append(np.asarray(Image.open(out)))
        stds.append(np.load(std))
    assert "Self-ensemble of 8 views" in capsys.readouterr().out
    assert outs[0].shape == (88, 120) and np.array_equal(outs[0], outs[1])
    assert stds[0].shape == (64, 64) and stds[0].dtype == np.float32 and np.array_equal(stds[0], stds[1])
    assert np.isfinite(stds[0]).all() and stds[0].max() > 0
    qpath = tmp_path / "q.npy"
    cli.main(base + ["--out", str(tmp_path / "q.png"), "--self-ensemble", "flips", "--quantiles", "0.05,0.5,0.95", "--quantiles-out", str(qpath)])
    q = np.load(qpath)
    assert q.shape == (3, 64, 64) and (q[0] <= q[1]).all() and (q[1] <= q[2]).all()
    # the mean over the views is not the single run
    single = cli.denoise_image_diffusion(str(ckpt), str(png), device_type="cuda", img_size=64, inference_steps=K_STEPS, variant="ddim")
    assert not np.array_equal(np.asarray(single), outs[0])
    capsys.readouterr()
    for argv, word in [(["--self-ensemble", "--samples", "4"], "--self-ensemble cannot be combined with --samples"),
                       (["--self-ensemble", "--tile", "64"], "--self-ensemble cannot be combined with --tile")]:
        with pytest.raises(SystemExit):
            cli.main(base + argv)
        assert word in capsys.readouterr().err, argv
