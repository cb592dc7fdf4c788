"""GPU: the tiled self-ensemble (include/midd.h: TILED SELF-ENSEMBLE; mi_tile_blend_unview_reduce, mi_tile_blend_unview_quantiles,
mi_denoise_tiled_self_ensemble; DiffusionDenoiser.denoise_tiled_self_ensemble).

The final launch's arithmetic is fixed -- the blend per view IN THE VIEW'S FRAME, the un-view, then the ensemble reduce / quantiles
-- so it is compared bit for bit with the numpy restatement (tests/tiled_self_ensemble_reference.py) and with the existing public
kernels run one after the other, on the smallest shapes that reach each path: the dword and the 16-byte path, partial 32 x 32
patches, origins that are not mirror-symmetric, one tile per view, a non-square tile (the instantiation without LDS).  The whole
call is held to what it IS: member k is `unview(denoise_tiled(view(x)))` -- on a reduced topology, 16 x 16 tiles, three steps."""
import ctypes as C

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, timestep_list, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import tiled_reference as tref
from tests import tiled_self_ensemble_reference as ref

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # the project's sampler gate (tests/test_gpu_parity.py); blend and mean are convex combinations
SMALL = dict(model_channels=16, time_emb_dim=64)
SEED, OFFSET, MEMBER_OFFSET = 0x1234567890ABCDEF, 3, 2
K_STEPS, TILE, OVERLAP, MAX_BATCH = 3, 16, 4, 4
LEVELS = (0.0, 0.25, 0.5, 1.0)
D4, FLIPS = ref.D4, ref.FLIPS

_sds, _models = {}, {}


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).view(np.uint32)


def _same(got, want, what):
    assert tuple(got.shape) == tuple(want.shape), (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), what


def tview(x, g):
    u = x.transpose(-1, -2) if g & 4 else x
    if g & 2:
        u = u.flip(-2)
    if g & 1:
        u = u.flip(-1)
    return u.contiguous()


def tunview(v, g):
    u = v
    if g & 1:
        u = u.flip(-1)
    if g & 2:
        u = u.flip(-2)
    if g & 4:
        u = u.transpose(-1, -2)
    return u.contiguous()


# ------------------------------------------------------------------------------ 1. the reduce and quantile launches alone
CASES = {   # name: (B, C, H, W, (th, tw), (oy, ox), views)
    "dword-41x27": (2, 1, 41, 27, (16, 16), (4, 4), D4),        # dword stores, partial patches, origins 0, 8, 16, 25 (not mirror-symmetric)
    "vec-48x32": (1, 2, 48, 32, (16, 16), (8, 8), D4),          # 16-byte loads and stores, overlap = T / 2: pixels under 2 x 2 tiles everywhere
    "one-tile-16x16": (1, 1, 16, 16, (16, 16), (4, 4), D4),     # one tile per view
    "flips-40x56": (1, 1, 40, 56, (16, 24), (4, 8), FLIPS),     # a non-square tile: no transposing view, the instantiation without LDS
}
_case_data = {}


def _case(name):
    """Random tiles of the case with mixed magnitudes, their device copy and the restatement's results; made once and shared."""
    if name not in _case_data:
        B, Cc, H, W, T, O, codes = CASES[name]
        K = len(tref.origins(H, T[0], O[0])) * len(tref.origins(W, T[1], O[1]))
        rng = np.random.default_rng(sum(map(ord, name)))
        tiles = rng.standard_normal((len(codes), B, K, Cc, T[0], T[1])).astype(np.float32)
        tiles[-1, B - 1, :, 0, 5:9, :] *= np.float32(1e4)
        want = ref.reduce(tiles, H, W, O, codes) + (ref.quantiles(tiles, H, W, O, codes, LEVELS),)
        _case_data[name] = (tiles, torch.from_numpy(tiles).cuda(), want)
    return _case_data[name]


def _composition(dev, H, W, O, codes):
    """The existing public pieces, one after the other: tile_blend per view in ITS frame, a torch un-view, stacked."""
    out = []
    for k, g in enumerate(codes):
        Hv, Wv, _, ov = ref.frame(H, W, tuple(dev.shape[4:]), O, g)
        out.append(tunview(midd_amd.tile_blend(dev[k], Hv, Wv, ov), g))
    return torch.stack(out, dim=1).contiguous()


@pytest.mark.parametrize("name", list(CASES))
def test_launches_equal_the_restatement_and_the_existing_kernels_bit_for_bit(name):
    B, Cc, H, W, T, O, codes = CASES[name]
    tiles, dev, (want_mean, want_std, want_samples, want_q) = _case(name)
    mean, std, samples = midd_amd.tile_blend_unview_reduce(dev, H, W, O, codes, return_samples=True)
    assert mean.shape == (B, Cc, H, W) and samples.shape == (B, len(codes), Cc, H, W) and mean.dtype == torch.float32
    _same(samples, want_samples, "samples")
    _same(mean, want_mean, "mean")
    _same(std, want_std, "std")
    q = midd_amd.tile_blend_unview_quantiles(dev, H, W, O, codes, LEVELS)
    _same(q, want_q, "quantiles")
    # the composition of existing public pieces, on the device
    stacked = _composition(dev, H, W, O, codes)
    two_mean, two_std = midd_amd.ensemble_reduce(stacked)
    assert torch.equal(samples, stacked) and torch.equal(mean, two_mean) and torch.equal(std, two_std)
    assert torch.equal(q, midd_amd.ensemble_quantiles(stacked, LEVELS))
    # the same bits without the samples
    quiet_mean, quiet_std, none = midd_amd.tile_blend_unview_reduce(dev, H, W, O, codes)
    assert none is None and torch.equal(quiet_mean, mean) and torch.equal(quiet_std, std)
    # the same bits from tiles that are not 16-byte aligned (the dword loads)
    shifted = torch.empty(dev.numel() + 1, device="cuda")[1:].view(dev.shape).copy_(dev)
    assert shifted.data_ptr() % 16 == 4
    m2, s2, sam2 = midd_amd.tile_blend_unview_reduce(shifted, H, W, O, codes, return_samples=True)
    assert torch.equal(m2, mean) and torch.equal(s2, std) and torch.equal(sam2, samples)
    assert torch.equal(midd_amd.tile_blend_unview_quantiles(shifted, H, W, O, codes, LEVELS), q)


@pytest.mark.parametrize("name,codes", [("dword-41x27", (6, 0, 3)), ("vec-48x32", (6, 0, 3)), ("vec-48x32", (5, 4)), ("dword-41x27", (7,)),
                                        ("flips-40x56", (2, 1)), ("flips-40x56", (3,)), ("one-tile-16x16", (4, 1, 7, 2))])
def test_a_list_gives_its_members_in_list_order_and_a_single_view_the_mean_only(name, codes):
    B, Cc, H, W, T, O, full = CASES[name]
    tiles, dev, _ = _case(name)
    pick = [full.index(g) for g in codes]
    sub, dsub = np.ascontiguousarray(tiles[pick]), dev[pick].contiguous()
    want_mean, want_std, want_samples = ref.reduce(sub, H, W, O, codes)
    mean, std, samples = midd_amd.tile_blend_unview_reduce(dsub, H, W, O, codes, return_samples=True)
    _same(samples, want_samples, "samples")
    _same(mean, want_mean, "mean")
    for k, g in enumerate(codes):                                              # member k is view codes[k]: the full list's member of that code
        assert torch.equal(samples[:, k], _composition(dev, H, W, O, full)[:, full.index(g)]), (k, g)
    _same(midd_amd.tile_blend_unview_quantiles(dsub, H, W, O, codes, LEVELS), ref.quantiles(sub, H, W, O, codes, LEVELS), "quantiles")
    if len(codes) > 1:
        _same(std, want_std, "std")
        return
    assert std is None and want_std is None and torch.equal(mean, samples[:, 0])
    v = (C.c_int32 * 1)(*codes)                                                 # std_out with one view is refused, before any GPU work
    out = torch.empty_like(mean)
    rc = native.lib().mi_tile_blend_unview_reduce(dsub.data_ptr(), B, Cc, H, W, T[0], T[1], O[0], O[1], v, 1, mean.data_ptr(), out.data_ptr(), None, None)
    assert rc == -1 and b"std_out needs at least two views" in native.lib().mi_last_error()


def test_a_non_square_tile_refuses_a_transposing_code():
    B, Cc, H, W, T, O, _ = CASES["flips-40x56"]
    _, dev, _ = _case("flips-40x56")
    with pytest.raises(ValueError, match="square tile and overlap"):
        midd_amd.tile_blend_unview_reduce(dev, H, W, O, (0, 1, 2, 5))
    v = (C.c_int32 * 4)(0, 1, 2, 5)
    out = torch.empty((B, Cc, H, W), device="cuda")
    rc = native.lib().mi_tile_blend_unview_reduce(dev.data_ptr(), B, Cc, H, W, T[0], T[1], O[0], O[1], v, 4, out.data_ptr(), None, None, None)
    assert rc == -1 and b"th == tw and oy == ox" in native.lib().mi_last_error()
    assert midd_amd.view_codes_tiled(H, W, T, O) == FLIPS


@pytest.mark.parametrize("name", ["dword-41x27", "flips-40x56"])
def test_a_nan_tile_element_makes_the_pixels_it_covers_nan_at_every_level(name):
    B, Cc, H, W, T, O, codes = CASES[name]
    tiles = _case(name)[0].copy()
    k, tile, ry, rx = len(codes) - 1, 1, 3, 14                                  # one element of one tile of the last view
    tiles[k, 0, tile, 0, ry, rx] = np.nan
    q = midd_amd.tile_blend_unview_quantiles(torch.from_numpy(tiles).cuda(), H, W, O, codes, LEVELS)
    _same(q, ref.quantiles(tiles, H, W, O, codes, LEVELS), "quantiles")
    g = codes[k]
    Hv, Wv, tv, ov = ref.frame(H, W, T, O, g)
    ys, xs = tref.origins(Hv, tv[0], ov[0]), tref.origins(Wv, tv[1], ov[1])
    hit = np.zeros((Hv, Wv), bool)
    hit[ys[tile // len(xs)] + ry, xs[tile % len(xs)] + rx] = True
    hit = ref.unview(hit, g)                                                     # the pixel of the image that element lies over
    got = np.isnan(q.cpu().numpy())
    assert hit.sum() == 1 and got[0, :, 0][:, hit].all() and got.sum() == len(LEVELS) and not got[1:].any()


# ------------------------------------------------------------------------------ 2. the whole call
def _sd(variant):
    if variant not in _sds:
        _sds[variant] = make_state_dict(UNetConfig(variant=variant, **SMALL), seed=5, perturb_norm=True)
    return _sds[variant]


def _model(variant="ddim", compute="f16x3", batch_invariant=False):
    key = (variant, compute, batch_invariant)
    if key not in _models:
        m = UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant, **SMALL)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd(variant).items()}, strict=True)
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models[key]


IMAGES = {"40x24": (1, 40, 24), "41x27": (2, 41, 27)}      # 3 x 2 = 6 tiles (passes of 4 + 2); 4 x 2 = 8 tiles, origins 0, 8, 16, 25


def _image(name):
    B, H, W = IMAGES[name]
    return torch.from_numpy(synthetic_xray(B, H, W, seed=9)).cuda()


KW = dict(inference_steps=K_STEPS, tile=TILE, overlap=OVERLAP, max_batch=MAX_BATCH)


@pytest.mark.parametrize("compute", ["f16x3", "f32"])
@pytest.mark.parametrize("name", list(IMAGES))
def test_ddim_members_are_the_tiled_runs_of_the_views_turned_back(name, compute):
    """Any plan: the passes of a view are mi_denoise_tiled's on the viewed batch, so this needs no batch-invariant plan."""
    den, x = _model("ddim", compute), _image(name)
    B, H, W = IMAGES[name]
    res = den.denoise_tiled_self_ensemble(x, views="d4", return_samples=True, return_tiles=True, **KW)
    assert res.views == D4 and res.seed is None and res.samples.shape == (B, 8, 1, H, W) and res.mean.shape == res.std.shape == x.shape
    assert res.tiles.shape[:3] == (8, B, len(res.origins_y) * len(res.origins_x)) and torch.isfinite(res.tiles).all()
    assert (res.origins_y, res.origins_x) == (tuple(tref.origins(H, TILE, OVERLAP)), tuple(tref.origins(W, TILE, OVERLAP)))
    for k, g in enumerate(D4):
        one = den.denoise_tiled(tview(x, g), return_tiles=True, **KW)
        assert torch.equal(res.tiles[k], one.tiles), (k, g)
        assert torch.equal(res.samples[:, k], tunview(one.image, g)), (k, g)
    mean, std = midd_amd.ensemble_reduce(res.samples)
    assert torch.equal(res.mean, mean) and torch.equal(res.std, std) and float(res.std.max()) > 0
    want_mean, want_std, want_samples = ref.reduce(res.tiles.cpu().numpy(), H, W, (OVERLAP, OVERLAP), D4)
    _same(res.samples, want_samples, "samples")
    _same(res.mean, want_mean, "mean")
    _same(res.std, want_std, "std")
    # the call twice gives the same bits; without the tensors the tiles live in the workspace and the members nowhere
    quiet = den.denoise_tiled_self_ensemble(x, views="d4", **KW)
    assert quiet.samples is None and quiet.tiles is None and torch.equal(quiet.mean, res.mean) and torch.equal(quiet.std, res.std)
    withq = den.denoise_tiled_self_ensemble(x, views="d4", quantiles=LEVELS, **KW)
    assert withq.tiles is None and torch.equal(withq.mean, res.mean) and torch.equal(withq.quantiles, midd_amd.ensemble_quantiles(res.samples, LEVELS))


def test_auto_is_d4_for_a_non_square_image_and_a_list_keeps_its_order():
    den, x = _model("ddim"), _image("40x24")
    full = den.denoise_tiled_self_ensemble(x, return_samples=True, **KW)                     # views="auto"
    assert full.views == D4
    part = den.denoise_tiled_self_ensemble(x, views=[6, 0, 3], return_samples=True, **KW)
    assert part.views == (6, 0, 3)
    for k, g in enumerate((6, 0, 3)):
        assert torch.equal(part.samples[:, k], full.samples[:, g]), g
    one = den.denoise_tiled_self_ensemble(x, views=[0], return_tiles=True, **KW)              # views = [0] IS denoise_tiled
    plain = den.denoise_tiled(x, return_tiles=True, **KW)
    assert one.std is None and torch.equal(one.mean, plain.image) and torch.equal(one.tiles[0], plain.tiles)


@pytest.mark.parametrize("name", list(IMAGES))
def test_cddpm_members_are_the_single_member_tiled_ensembles_of_the_views(name):
    den, x = _model("cddpm"), _image(name)
    kw = dict(seed=SEED, sample_offset=OFFSET, **KW)
    res = den.denoise_tiled_self_ensemble(x, views="d4", member_offset=MEMBER_OFFSET, return_samples=True, return_tiles=True, **kw)
    assert res.seed == SEED and torch.isfinite(res.mean).all()
    for k, g in enumerate(D4):
        one = den.denoise_tiled_ensemble(tview(x, g), members=1, member_offset=MEMBER_OFFSET + k, return_samples=True, return_tiles=True, **kw)
        assert torch.equal(res.tiles[k], one.tiles[0]), (k, g)
        assert torch.equal(res.samples[:, k], tunview(one.samples[:, 0], g)), (k, g)
    mean, std = midd_amd.ensemble_reduce(res.samples)
    assert torch.equal(res.mean, mean) and torch.equal(res.std, std)
    first = den.denoise_tiled_self_ensemble(x, views=[0], return_tiles=True, **kw)            # member_offset 0, the identity: the seeded tiled run
    plain = den.denoise_tiled(x, return_tiles=True, **kw)
    assert torch.equal(first.mean, plain.image) and torch.equal(first.tiles[0], plain.tiles)
    again = den.denoise_tiled_self_ensemble(x, views="d4", member_offset=MEMBER_OFFSET, **kw)
    assert torch.equal(again.mean, res.mean) and torch.equal(again.std, res.std)


def test_with_a_batch_invariant_plan_every_tile_is_the_denoised_crop_of_the_view_whatever_the_pass_size():
    den, x = _model("cddpm", batch_invariant=True), _image("41x27")
    B, H, W = IMAGES["41x27"]
    codes = (0, 5, 3, 6)
    n_iters = len(timestep_list(50, K_STEPS))
    runs = [den.denoise_tiled_self_ensemble(x, inference_steps=K_STEPS, views=codes, tile=TILE, overlap=OVERLAP, max_batch=mb, seed=SEED,
                                            sample_offset=OFFSET, member_offset=MEMBER_OFFSET, return_tiles=True) for mb in (MAX_BATCH, 3)]
    assert torch.equal(runs[0].tiles, runs[1].tiles) and torch.equal(runs[0].mean, runs[1].mean) and torch.equal(runs[0].std, runs[1].std)
    for k, g in enumerate(codes):
        v = tview(x, g)
        plan = midd_amd.tile_plan(v.shape[2], v.shape[3], TILE, OVERLAP)
        field = midd_amd.step_noise(SEED, n_iters, v.shape, sample_offset=OFFSET, member=MEMBER_OFFSET + k)
        where = [(b, y0, x0) for b in range(B) for y0 in plan.origins_y for x0 in plan.origins_x]
        crops = midd_amd.tile_extract(v, TILE, OVERLAP).reshape(len(where), 1, TILE, TILE)
        noise = torch.stack([field[:, b, :, y0:y0 + TILE, x0:x0 + TILE] for b, y0, x0 in where], dim=1).contiguous()
        alone = den.denoise(crops, inference_steps=K_STEPS, step_noise=noise)
        assert torch.equal(runs[0].tiles[k].reshape(alone.shape), alone), (k, g)


@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_update_ddim(variant):
    den, x = _model(variant), _image("40x24")
    codes = (0, 6, 3)
    res = den.denoise_tiled_self_ensemble(x, views=codes, return_samples=True, update="ddim", **KW)                  # eta = 0: deterministic
    assert res.seed is None
    for k, g in enumerate(codes):
        one = den.denoise_tiled(tview(x, g), update="ddim", **KW)
        assert torch.equal(res.samples[:, k], tunview(one.image, g)), (k, g)
    assert not torch.equal(res.mean, den.denoise_tiled_self_ensemble(x, views=codes, **KW, **({"seed": SEED} if variant == "cddpm" else {})).mean)
    kw = dict(update="ddim", eta=0.7, seed=SEED, sample_offset=OFFSET, **KW)                                         # eta > 0: seeded, both variants
    first = den.denoise_tiled_self_ensemble(x, views=[0], **kw)
    assert first.seed == SEED and torch.equal(first.mean, den.denoise_tiled(x, **kw).image)
    a = den.denoise_tiled_self_ensemble(x, views="d4", **kw)
    b = den.denoise_tiled_self_ensemble(x, views="d4", **kw)
    assert torch.equal(a.mean, b.mean) and torch.equal(a.std, b.std) and torch.isfinite(a.mean).all()
    assert not torch.equal(a.mean, den.denoise_tiled_self_ensemble(x, views="d4", **{**kw, "eta": 0.0}).mean)
    with pytest.raises(ValueError, match="dpmpp2m"):
        den.denoise_tiled_self_ensemble(x, update="dpmpp2m", **KW)


# ------------------------------------------------------------------------------ 3. against the oracle
@pytest.mark.parametrize("compute", ["f16x3", "f32"])
def test_ddim_mean_matches_the_composition_over_the_oracles_forward(compute):
    """The restated composition with the CPU oracle as the sampler: every view's crops through the oracle, blended in the view's
    frame, turned back, reduced -- all in numpy.  The mean is a convex combination (blend, then mean) of tile pixels, so it keeps the
    project's 1e-3 sampler gate (the measured distances: DESIGN.md section 6b)."""
    B, H, W = IMAGES["40x24"]
    x = _image("40x24")
    cfg = UNetConfig(variant="ddim", **SMALL)
    tiles = []
    for g in D4:
        crops = ref.view_tiles(x.cpu().numpy(), (TILE, TILE), (OVERLAP, OVERLAP), [g])[0]
        out = orc.denoise(orc.to_torch(_sd("ddim")), topology(cfg), torch.from_numpy(crops.reshape(-1, 1, TILE, TILE)), 50, K_STEPS)
        tiles.append(out.numpy().reshape(crops.shape))
    want_mean, want_std, _ = ref.reduce(np.stack(tiles).astype(np.float32), H, W, (OVERLAP, OVERLAP), D4)
    res = _model("ddim", compute).denoise_tiled_self_ensemble(x, views="d4", **KW)
    err_mean = float(np.abs(res.mean.cpu().numpy() - want_mean).max())
    err_std = float(np.abs(res.std.cpu().numpy() - want_std).max())
    print(f"ddim {compute}: mean max|delta| = {err_mean:.3e} (gate {TOL_FINAL:.0e}), std max|delta| = {err_std:.3e}, std max = {float(res.std.max()):.3e}")
    assert err_mean < TOL_FINAL


# ------------------------------------------------------------------------------ 4. the CLI
def test_cli_views_and_members_with_tile(tmp_path, capsys):
    from PIL import Image
    from midd_amd import cli
    png = tmp_path / "in.png"
    Image.fromarray((synthetic_xray(1, 72, 88, seed=9)[0, 0].clip(0, 1) * 255).astype(np.uint8), mode="L").save(png)
    ckpts = {}
    for variant in ("ddim", "cddpm"):                                          # the CLI builds the reference's default topology
        ckpts[variant] = str(tmp_path / f"{variant}.pth")
        sd = make_state_dict(UNetConfig(variant=variant), seed=42)
        torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "noise_steps": 50}, ckpts[variant])
    base = ["--image", str(png), "--inference-steps", "2", "--tile", "64", "--overlap", "16"]
    out, std, qp = tmp_path / "out.png", tmp_path / "std.npy", tmp_path / "q.npy"
    cli.main(base + ["--variant", "ddim", "--checkpoint", ckpts["ddim"], "--views", "--out", str(out), "--std-out", str(std), "--quantiles", "0.05,0.5,0.95", "--quantiles-out", str(qp)])
    assert "Self-ensemble of 8 views" in capsys.readouterr().out
    s, q = np.load(std), np.load(qp)
    assert np.asarray(Image.open(out)).shape == (72, 88) and s.shape == (72, 88) and s.dtype == np.float32 and np.isfinite(s).all()
    assert q.shape == (3, 72, 88) and (q[0] <= q[1]).all() and (q[1] <= q[2]).all()
    cli.main(base + ["--variant", "ddim", "--checkpoint", ckpts["ddim"], "--views", "flips", "--update", "ddim", "--bit-depth", "16", "--out", str(out)])
    assert "Self-ensemble of 4 views" in capsys.readouterr().out and Image.open(out).mode in ("I;16", "I")
    cli.main(base + ["--variant", "cddpm", "--checkpoint", ckpts["cddpm"], "--members", "2", "--seed", "7", "--out", str(out), "--std-out", str(std)])
    assert "Ensemble of 2 samples, tiled" in capsys.readouterr().out and np.load(std).shape == (72, 88)
