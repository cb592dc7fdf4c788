"""GPU: fused tiled denoising (include/midd.h: THE CONSENSUS, mi_tile_consensus, mi_denoise_tiled_fused;
midd_amd.tile_consensus, DiffusionDenoiser.denoise_tiled_fused).

The consensus has fixed arithmetic, so it is compared bit for bit (int32 views: a NaN counts) with the numpy restatement
(tests/tiled_fused_reference.py) and with the device composition tile_extract(tile_blend(.)), on every load path.  The call is
specified as a composition of public calls -- one row of run_slots_rule per (step, pass), one tile_consensus per step -- and must
equal it bit for bit; against the float64-free CPU oracle it is held to the project's 1e-3 parity gate."""
import numpy as np
import pytest
import torch
from PIL import Image

import midd_amd
from midd_amd import DiffusionDenoiser, SamplerRule, UNetConfig, UNetDiffusion, native, timestep_list, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import ddim_update_reference as ddim_ref
from tests import tiled_fused_reference as fref
from tests import tiled_reference as ref

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # north_star: |delta| < 1e-3 fp32 per pixel (tests/test_gpu_parity.py); the consensus is a convex combination
SEED = 0x1234567890ABCDEF
OFFSET = 3                # sample_offset of the seeded cases
K_STEPS = 5               # inference_steps of the sampler cases
H, W, TILE, OVERLAP = 88, 104, 64, 16          # the shape of tests/test_gpu_tiled.py: 2 x 2 tiles, origins (0, 24) x (0, 40), B = 2: 8 tiles

_sds, _models, _runs, _oracle = {}, {}, {}, {}


def _sd(variant):
    if variant not in _sds:
        _sds[variant] = make_state_dict(UNetConfig(variant=variant), seed=42)
    return _sds[variant]


def _model(variant, compute="f16x3", batch_invariant=True):
    key = (variant, compute, batch_invariant)
    if key not in _models:
        m = UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd(variant).items()}, strict=True)
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models[key]


def _image(h=H, w=W, B=2):
    return torch.from_numpy(synthetic_xray(B, h, w, seed=77)).cuda()


def _bits(t):
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


# (variant, rule keywords, seeded): the sampler cases of the call
CASES = {
    "ddim-reference": ("ddim", {}, False),
    "cddpm-reference": ("cddpm", {}, True),
    "ddim-eta": ("ddim", dict(update="ddim", eta=0.5), True),
    "ddim-dpmpp2m": ("ddim", dict(update="dpmpp2m"), False),
}


def _seed_kw(seeded):
    return dict(seed=SEED, sample_offset=OFFSET) if seeded else {}


def _fused(case, compute="f16x3", max_batch=8, batch_invariant=True):
    """The 88 x 104 case, run once per key and shared."""
    key = (case, compute, max_batch, batch_invariant)
    if key not in _runs:
        variant, rule, seeded = CASES[case]
        _runs[key] = _model(variant, compute, batch_invariant).denoise_tiled_fused(
            _image(), inference_steps=K_STEPS, tile=TILE, overlap=OVERLAP, max_batch=max_batch, return_tiles=True, **_seed_kw(seeded), **rule)
    return _runs[key]


# ------------------------------------------------------------------------------ 1. the consensus kernel
# (H, W, tile, overlap).  25 x 27: W odd, the dword kernel, 3 x 3 tiles with triple cover on both axes.  41 x 52 (origins 0, 9, 18, 28)
# and 40 x 36 (tile 16 x 24, origins 0, 12): the 16-byte kernel whose threads fall back to dwords wherever a covering tile sits at an
# odd place.  45 x 59: W odd again.  56 x 56 (origins 0, 12, 24): 16 bytes everywhere, 3 x 3 cover.
CONSENSUS_GEOMETRIES = [(25, 27, (16, 16), (8, 8)), (41, 52, (24, 24), (12, 12)), (45, 59, (32, 32), (8, 8)), (40, 36, (16, 24), (8, 5)),
                        (56, 56, (32, 32), (16, 16))]


def _planted_tiles(h, w, tile, overlap, C):
    """Gaussian tiles [2, K, C, th, tw] with NaN, +Inf, -Inf and -0.0 planted inside an overlap and inside a single-cover region
    (tile 0 of image 0, channel 0; eight different pixels, so no Inf meets its opposite)."""
    K = len(ref.origins(h, tile[0], overlap[0])) * len(ref.origins(w, tile[1], overlap[1]))
    rng = np.random.default_rng(h * 100 + w + C)
    tiles = rng.standard_normal((2, K, C) + tile).astype(np.float32)
    shared = fref.cover_mask(1, 1, h, w, tile, overlap)[0, 0, 0]
    specials = np.array([np.nan, np.inf, -np.inf, -0.0], np.float32)
    for where in (np.argwhere(shared), np.argwhere(~shared)):
        assert len(where) >= 4
        for (ry, rx), v in zip(where[:: max(1, len(where) // 4)][:4], specials):
            tiles[0, 0, 0, ry, rx] = v
    return tiles


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("geom", CONSENSUS_GEOMETRIES)
def test_consensus_equals_the_restatement_and_the_device_composition_bit_for_bit(geom, C):
    h, w, tile, overlap = geom
    tiles = _planted_tiles(h, w, tile, overlap, C)
    want_tiles, want_image = fref.consensus(tiles, h, w, overlap, return_image=True)
    dev = torch.from_numpy(tiles).cuda()
    got = midd_amd.tile_consensus(dev, h, w, overlap)                           # on a copy, no image
    assert got.data_ptr() != dev.data_ptr() and _same_bits(dev, tiles)          # the input is untouched
    assert got.shape == dev.shape and _same_bits(got, want_tiles)
    got2, image = midd_amd.tile_consensus(dev, h, w, overlap, return_image=True)
    assert _same_bits(got2, want_tiles) and image.shape == (2, C, h, w) and _same_bits(image, want_image)
    blended = midd_amd.tile_blend(dev, h, w, overlap)                           # the pair of launches the kernel replaces
    assert _same_bits(image, blended) and _same_bits(got, midd_amd.tile_extract(blended, tile, overlap))
    # a tiles pointer one element off 16-byte alignment: the dword kernel, in place, with and without the image
    for with_image in (False, True):
        pad = torch.zeros(tiles.size + 1, device="cuda")
        shifted = pad[1:].view(dev.shape)
        shifted.copy_(dev)
        assert shifted.data_ptr() % 16 == 4
        out = midd_amd.tile_consensus(shifted, h, w, overlap, inplace=True, return_image=with_image)
        res = out[0] if with_image else out
        assert res.data_ptr() == shifted.data_ptr() and _same_bits(shifted, want_tiles) and float(pad[0]) == 0.0
        if with_image:
            assert _same_bits(out[1], want_image)
    # run twice, it equals once run
    again = midd_amd.tile_consensus(got.clone(), h, w, overlap, inplace=True)
    assert _same_bits(again, got)
    # the specials really sat where the test says: the NaN under an overlap reached every tile over its pixel
    assert np.isnan(want_tiles).sum() >= 3 and np.isinf(want_tiles).sum() >= 6


def test_consensus_of_abutting_tiles_and_of_one_tile_is_the_identity():
    x = torch.randn(2, 3, 128, 128, device="cuda")
    tiles = midd_amd.tile_extract(x, 64, 0)
    assert tiles.shape == (2, 4, 3, 64, 64)
    noise = torch.randn_like(tiles)                                             # tiles that agree nowhere: nothing is shared, nothing changes
    out, image = midd_amd.tile_consensus(noise, 128, 128, 0, return_image=True)
    assert _same_bits(out, noise) and _same_bits(midd_amd.tile_extract(image, 64, 0), noise)
    one = torch.randn(2, 1, 1, 40, 56, device="cuda")                            # one tile that is the image
    out, image = midd_amd.tile_consensus(one, 40, 56, 8, return_image=True)
    assert _same_bits(out, one) and _same_bits(image, one[:, 0])


# ------------------------------------------------------------------------------ 2. the call is its composition
def _compose(den, x, variant, rule_kw, seeded, max_batch, inference_steps=K_STEPS, tile=TILE, overlap=OVERLAP):
    """include/midd.h: the specification of mi_denoise_tiled_fused, out of the public calls -- one row of run_slots_rule per
    (step, pass) at the native call's pass size, one tile_consensus per step.  -> (image, tiles)."""
    model = den.model
    t_list = list(timestep_list(50, inference_steps))
    B, Cc, h, w = x.shape
    plan = midd_amd.tile_plan(h, w, tile, overlap)
    (th, tw), K = plan.tile, len(plan.origins_y) * len(plan.origins_x)
    cond = midd_amd.tile_extract(x, tile, overlap).reshape(B * K, Cc, th, tw).contiguous()
    xs = cond.clone()
    rule = SamplerRule(**rule_kw) if rule_kw else None
    hist = torch.empty_like(xs) if rule is not None and rule.update == "dpmpp2m" else None
    V = B * K
    p = min(max_batch, V)
    image = None
    for i, t in enumerate(t_list):
        for v0 in range(0, V, p):
            vs = list(range(v0, min(v0 + p, V)))
            kw = dict(iter_base=[i] * len(vs), sample_index=[OFFSET * seeded + v // K for v in vs])
            if seeded:
                kw.update(seed=SEED, frame=[(w, h * w, plan.origins_y[(v % K) // len(plan.origins_x)] * w + plan.origins_x[(v % K) % len(plan.origins_x)])
                                            for v in vs])
            if rule is not None:
                kw.update(rule=rule, t_before=[t_list[i - 1] if i > 0 else -1] * len(vs),
                          t_after=[t_list[i + 1] if i + 1 < len(t_list) else -1] * len(vs))
            if hist is not None:
                kw.update(x0=hist[v0:v0 + len(vs)])
            model.run_slots_rule(cond[v0:v0 + len(vs)], xs[v0:v0 + len(vs)], [[t] * len(vs)], den.beta, den.alpha, den.alpha_hat,
                                 clamp_eps=variant == "ddim", **kw)
        last = i == len(t_list) - 1
        out = midd_amd.tile_consensus(xs.view(B, K, Cc, th, tw), h, w, overlap, inplace=True, return_image=last)
        if last:
            image = out[1]
    return image, xs.view(B, K, Cc, th, tw)


@pytest.mark.parametrize("max_batch", [3, 8])
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_call_equals_its_composition_bit_for_bit(case, max_batch):
    """8 tiles in passes of 3, 3, 2 and in one pass of 8 (which splits into two programs of 4), batch_invariant off: the pass
    size shows in the bits, and the composition at the same pass size must show the same."""
    variant, rule_kw, seeded = CASES[case]
    den = _model(variant, batch_invariant=False)
    res = _fused(case, max_batch=max_batch, batch_invariant=False)
    assert res.origins_y == (0, 24) and res.origins_x == (0, 40) and res.tiles.shape == (2, 4, 1, TILE, TILE)
    assert res.seed == (SEED if seeded else None) and torch.isfinite(res.image).all()
    image, tiles = _compose(den, _image(), variant, rule_kw, seeded, max_batch)
    assert _same_bits(res.tiles, tiles), case
    assert _same_bits(res.image, image), case


def test_a_triple_cover_case_equals_its_composition():
    """64 x 120, tile 64, overlap 32: one row of three tiles at origins 0, 28, 56 -- columns 56 .. 63 lie under all three."""
    den = _model("cddpm", batch_invariant=False)
    x = _image(64, 120, B=1)
    res = den.denoise_tiled_fused(x, inference_steps=3, tile=64, overlap=32, max_batch=2, return_tiles=True, seed=SEED, sample_offset=OFFSET)
    assert res.origins_y == (0,) and res.origins_x == (0, 28, 56) and ref.cover_counts(120, 64, 32).max() == 3
    image, tiles = _compose(den, x, "cddpm", {}, True, 2, inference_steps=3, tile=64, overlap=32)
    assert _same_bits(res.tiles, tiles) and _same_bits(res.image, image)
    assert _same_bits(res.tiles, midd_amd.tile_extract(res.image, 64, 32))


# ------------------------------------------------------------------------------ 3. properties of the result
@pytest.mark.parametrize("case", ["ddim-reference", "cddpm-reference"])
def test_with_a_batch_invariant_plan_the_pass_size_does_not_show(case):
    base = _fused(case, max_batch=8)
    for mb in (1, 3):
        r = _fused(case, max_batch=mb)
        assert _same_bits(r.tiles, base.tiles) and _same_bits(r.image, base.image), (case, mb)
    variant, rule_kw, seeded = CASES[case]
    quiet = _model(variant).denoise_tiled_fused(_image(), inference_steps=K_STEPS, tile=TILE, overlap=OVERLAP, max_batch=3, **_seed_kw(seeded))
    assert quiet.tiles is None and _same_bits(quiet.image, base.image)          # the tile states live in the workspace


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_tile_is_the_plain_call(case):
    variant, rule_kw, seeded = CASES[case]
    den = _model(variant, batch_invariant=False)
    x = _image(64, 64)
    res = den.denoise_tiled_fused(x, inference_steps=K_STEPS, tile=64, overlap=16, return_tiles=True, **_seed_kw(seeded), **rule_kw)
    plain = den.denoise(x, inference_steps=K_STEPS, **_seed_kw(seeded), **rule_kw)
    assert res.origins_y == (0,) and res.origins_x == (0,) and res.tiles.shape == (2, 1, 1, 64, 64)
    assert torch.equal(res.image, plain) and torch.equal(res.tiles[:, 0], plain)
    assert res.seed == (SEED if seeded else None)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_tiles_agree_and_the_result_differs_from_the_unfused_call(case):
    variant, rule_kw, seeded = CASES[case]
    res = _fused(case)
    assert _same_bits(res.tiles, midd_amd.tile_extract(res.image, TILE, OVERLAP))          # tiles == extract(image): nothing left to hide
    unfused = _model(variant).denoise_tiled(_image(), inference_steps=K_STEPS, tile=TILE, overlap=OVERLAP, return_tiles=True,
                                            **_seed_kw(seeded), **rule_kw)
    assert not torch.equal(unfused.image, res.image)
    shared = torch.from_numpy(fref.cover_mask(2, 1, H, W, (TILE, TILE), (OVERLAP, OVERLAP))).cuda()
    gap = (unfused.tiles - midd_amd.tile_extract(unfused.image, TILE, OVERLAP)).abs()[shared]
    print(f"{case}: the unfused tiles differ from their own blend by up to {float(gap.max()):.3e} on shared pixels; the fused ones by 0")
    assert float(gap.max()) > 0.0


def test_the_same_call_gives_the_same_bits_and_a_drawn_seed_reproduces_the_run():
    den = _model("cddpm")
    x = _image()
    kw = dict(inference_steps=K_STEPS, tile=TILE, overlap=OVERLAP, max_batch=8, return_tiles=True)
    again = den.denoise_tiled_fused(x, seed=SEED, sample_offset=OFFSET, **kw)
    base = _fused("cddpm-reference")
    assert _same_bits(again.image, base.image) and _same_bits(again.tiles, base.tiles)
    other = den.denoise_tiled_fused(x, seed=SEED + 1, sample_offset=OFFSET, **kw)
    assert not torch.equal(other.image, base.image)
    drawn = den.denoise_tiled_fused(x[:1], inference_steps=2, tile=TILE, overlap=OVERLAP)      # seed=None: drawn, and returned
    assert isinstance(drawn.seed, int) and 0 <= drawn.seed < 1 << 64
    assert _same_bits(den.denoise_tiled_fused(x[:1], inference_steps=2, tile=TILE, overlap=OVERLAP, seed=drawn.seed).image, drawn.image)
    ddim = _model("ddim")
    assert ddim.denoise_tiled_fused(x[:1], inference_steps=2, tile=TILE, overlap=OVERLAP).seed is None
    with pytest.raises(native.MiddError, match="tile <= image"):
        ddim.denoise_tiled_fused(x, inference_steps=2, tile=96, overlap=16)


def test_a_nan_pixel_is_reported():
    den = _model("ddim")
    x = _image()
    bad = x.clone()
    bad[0, 0, 3, 5] = float("nan")
    kw = dict(inference_steps=K_STEPS, tile=TILE, overlap=OVERLAP, max_batch=2)
    assert torch.isfinite(den.denoise_tiled_fused(x, **kw).image).all()        # clean input: no flag
    with pytest.raises(native.MiddError) as ei:
        den.denoise_tiled_fused(bad, **kw)
    assert ei.value.code == -5
    assert torch.isfinite(den.denoise_tiled_fused(x, **kw).image).all()        # the next call clears the word


# ------------------------------------------------------------------------------ 4. against the oracle
def _noise_crops(x, plan):
    """[n_iters, B, K, C, th, tw]: every tile's crop of the image's seeded noise field."""
    n_iters = len(timestep_list(50, K_STEPS))
    field = midd_amd.step_noise(SEED, n_iters, x.shape, sample_offset=OFFSET).cpu().numpy()
    return ref.extract(field.reshape((n_iters * x.shape[0],) + tuple(x.shape[1:])), (TILE, TILE), (OVERLAP, OVERLAP)).reshape(
        (n_iters, x.shape[0], -1, x.shape[1], TILE, TILE))


def _oracle_fused(variant, update):
    """The restated step-outer loop over the CPU oracle's forward, numpy consensus after every step.  Once per (variant, update)."""
    key = (variant, update)
    if key not in _oracle:
        x = _image()
        sd, topo = orc.to_torch(_sd(variant)), topology(UNetConfig(variant=variant))
        plan = midd_amd.tile_plan(H, W, TILE, OVERLAP)

        def eps(xn, cond, t):
            return orc.unet_forward(sd, topo, torch.from_numpy(xn), torch.from_numpy(cond), torch.full((xn.shape[0],), t, dtype=torch.long)).numpy()

        noise = _noise_crops(x, plan) if variant == "cddpm" else None
        _oracle[key] = fref.fused_loop(x.cpu().numpy(), list(timestep_list(50, K_STEPS)), ddim_ref.schedule(50), eps, (TILE, TILE),
                                       (OVERLAP, OVERLAP), clamp_eps=variant == "ddim", update=update, step_noise=noise)
    return _oracle[key]


@pytest.mark.parametrize("variant,update,compute", [("ddim", "reference", "f16x3"), ("ddim", "reference", "f32"),
                                                    ("cddpm", "reference", "f16x3"), ("cddpm", "reference", "f32"), ("ddim", "ddim", "f16x3")])
def test_fused_call_matches_the_restated_loop_over_the_oracle(variant, update, compute):
    want_image, want_tiles = _oracle_fused(variant, update)
    if update == "ddim":
        res = _model(variant, compute).denoise_tiled_fused(_image(), inference_steps=K_STEPS, tile=TILE, overlap=OVERLAP, return_tiles=True,
                                                           update="ddim")
    else:
        res = _fused(f"{variant}-reference", compute)
    err_tiles = float(np.abs(res.tiles.cpu().numpy() - want_tiles).max())
    err_image = float(np.abs(res.image.cpu().numpy() - want_image).max())
    print(f"{variant} update={update} {compute}: tiles max|delta| = {err_tiles:.3e}, image max|delta| = {err_image:.3e}")
    assert err_tiles < TOL_FINAL
    assert err_image < TOL_FINAL


# ------------------------------------------------------------------------------ 5. CLI
def test_cli_tile_fuse_step_writes_the_image_of_the_api_call(tmp_path):
    from midd_amd import cli
    sd = _sd("cddpm")
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "noise_steps": 50}, ckpt)
    png, out = tmp_path / "in.png", tmp_path / "out.png"
    u8 = (synthetic_xray(1, 90, 70, seed=9)[0, 0].clip(0, 1) * 255).astype(np.uint8)
    Image.fromarray(u8, mode="L").save(png)
    cli.main(["--image", str(png), "--out", str(out), "--checkpoint", str(ckpt), "--inference-steps", str(K_STEPS),
              "--tile", "64", "--overlap", "16", "--tile-fuse", "step", "--seed", "7"])
    got = np.asarray(Image.open(out))
    assert got.shape == (90, 70) and got.dtype == np.uint8
    x = torch.from_numpy(u8.astype(np.float32) / 255.0)[None, None].cuda()
    den = _model("cddpm", batch_invariant=False)
    res = den.denoise_tiled_fused(x, inference_steps=K_STEPS, tile=64, overlap=16, seed=7)
    assert res.origins_y == (0, 26) and res.origins_x == (0, 6)
    assert np.array_equal(got, (res.image[0, 0].cpu().numpy() * 255).astype(np.uint8))
    end = den.denoise_tiled(x, inference_steps=K_STEPS, tile=64, overlap=16, seed=7)
    assert not torch.equal(end.image, res.image)
