"""GPU: per-pixel quantile maps of an ensemble (include/midd.h: mi_ensemble_quantiles, mi_tile_blend_quantiles;
midd_amd.ensemble_quantiles, midd_amd.tile_blend_quantiles, DiffusionDenoiser.denoise_ensemble / denoise_tiled_ensemble with
``quantiles=``).

The arithmetic is fixed -- a total-order sort of the members, then a linear interpolation in double precision -- so both kernels
are compared bit for bit with the numpy restatement (tests/quantile_reference.py), the blend form also with ``tile_blend`` per
member followed by ``ensemble_quantiles``, and the sampler calls with the same calls without ``quantiles``."""
import numpy as np
import pytest
import torch
from PIL import Image

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native
from midd_amd.weights import make_state_dict, synthetic_xray
from tests import quantile_reference as qref
from tests import tiled_reference

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
K_STEPS = 5
LEVELS = (0.0, 0.05, 1.0 / 3.0, 0.5, 0.95, 1.0)

_sds, _models = {}, {}


def _sd():
    if "cddpm" not in _sds:
        _sds["cddpm"] = make_state_dict(UNetConfig(variant="cddpm"), seed=42)
    return _sds["cddpm"]


def _model(batch_invariant=False):
    if batch_invariant not in _models:
        m = UNetDiffusion(variant="cddpm", batch_invariant=batch_invariant)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd().items()}, strict=True)
        _models[batch_invariant] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models[batch_invariant]


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _members(B, K, chw, seed):
    """Uniform [0, 1) members with what the order has to get right planted into the first pixels: ties, signed zeros, a
    denormal, both infinities and one NaN pixel."""
    rng = np.random.default_rng(seed)
    x = rng.random((B, K, chw), dtype=np.float32)
    if K >= 2:
        x[:, 1, 8::3] = x[:, 0, 8::3]                                            # ties
        x[:, K - 1, 9::7] = x[:, K // 2, 9::7]
        x[0, :, 0] = np.where(np.arange(K) % 2 == 0, np.float32(-0.0), np.float32(0.0))
        x[0, 0, 1], x[0, K - 1, 1] = np.float32(1e-45), np.float32(-1e-45)       # denormals among ordinary values
        x[0, K - 1, 2] = np.inf
        x[0, 0, 3] = -np.inf
        x[0, 0, 4], x[0, 1, 4] = np.inf, -np.inf
        x[1, K - 1, 6] = 0.25
        x[1, :, 7] = 0.7                                                         # constant over the members
    x[1, K // 2, 5] = np.nan                                                     # the NaN pixel
    return x


def _check_against_restatement(got, x, levels):
    want = qref.quantiles(x, levels)
    assert got.shape == want.shape and got.dtype == np.float32
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (np.argwhere(diff)[:5], got[diff][:5], want[diff][:5])
    ok = ~np.isnan(got)
    step_ok = ok[:, 1:] & ok[:, :-1]
    assert (got[:, 1:] >= got[:, :-1])[step_ok].all()                            # non-decreasing along the level axis (inf >= inf: no difference is formed)


# ------------------------------------------------------------------------------ 1. ensemble_quantiles alone
@pytest.mark.parametrize("K", [1, 2, 3, 5, 8, 9, 16, 17, 33, 64])
def test_ensemble_quantiles_equal_the_restatement_bit_for_bit(K):
    """Every padded size and its boundary.  chw = 105: one pixel per thread; chw = 128: four, with 16-byte loads; the same 128
    behind a one-float offset: the pointer is not 16-byte aligned, so one pixel per thread again -- and the same bits."""
    B = 2
    for chw in (105, 128):
        x = _members(B, K, chw, seed=K * 1000 + chw)
        dev = torch.from_numpy(x).cuda()
        got = midd_amd.ensemble_quantiles(dev, LEVELS)
        assert got.shape == (B, len(LEVELS), chw) and got.dtype == torch.float32 and got.is_cuda
        _check_against_restatement(got.cpu().numpy(), x, LEVELS)
        assert (_bits(got)[1, :, 5] == 0x7FC00000).all()                         # the NaN pixel, at every level
        assert int(torch.isnan(got[1]).sum()) == len(LEVELS)                     # ... and nowhere else in that image
        if K >= 2:
            assert (got[1, :, 7] == np.float32(0.7)).all()
        if chw == 128:
            assert dev.data_ptr() % 16 == 0
            shifted = torch.empty(B * K * chw + 1, dtype=torch.float32, device="cuda")[1:].view(B, K, chw)
            shifted.copy_(dev)
            assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
            assert np.array_equal(_bits(midd_amd.ensemble_quantiles(shifted, LEVELS)), _bits(got))
    # shaped samples are read as [B, K, chw]
    img = midd_amd.ensemble_quantiles(dev.view(B, K, 2, 8, 8), LEVELS)
    assert img.shape == (B, len(LEVELS), 2, 8, 8) and np.array_equal(_bits(img).reshape(B, len(LEVELS), 128), _bits(got))


def test_eight_levels_and_one_level():
    x = _members(2, 9, 128, seed=5)
    dev = torch.from_numpy(x).cuda()
    eight = (0.0, 0.125, 0.25, 0.5, 0.5, 0.75, 0.999, 1.0)
    got = midd_amd.ensemble_quantiles(dev, eight)
    _check_against_restatement(got.cpu().numpy(), x, eight)
    assert np.array_equal(_bits(got[:, 3]), _bits(got[:, 4]))
    one = midd_amd.ensemble_quantiles(dev, 0.5)
    assert one.shape == (2, 1, 128) and np.array_equal(_bits(one[:, 0]), _bits(got[:, 3]))
    clean = torch.from_numpy(np.random.default_rng(1).random((2, 9, 128), dtype=np.float32)).cuda()
    assert torch.equal(midd_amd.ensemble_quantiles(clean, (0.5,))[:, 0], clean.median(dim=1).values)
    lib = native.lib()
    out = torch.empty(2, 128, device="cuda")
    import ctypes as C
    q = (C.c_double * 1)(0.5)
    assert lib.mi_ensemble_quantiles(dev.data_ptr(), 2, 65, 128, q, 1, out.data_ptr(), None) == -1
    assert b"members <= 64" in lib.mi_last_error()


# ------------------------------------------------------------------------------ 2. tile_blend_quantiles on synthetic tiles
@pytest.mark.parametrize("members", [3, 5])
def test_tile_blend_quantiles_equal_blend_then_quantiles_bit_for_bit(members):
    """40 x 56 / 32 / 8: 2 x 2 tiles, pixels under one, two and four of them."""
    B, C, h, w, T, O = 2, 1, 40, 56, 32, 8
    p = midd_amd.tile_plan(h, w, T, O)
    K = len(p.origins_y) * len(p.origins_x)
    assert K == 4
    rng = np.random.default_rng(members)
    tiles = rng.random((members, B, K, C, T, T), dtype=np.float32)
    tiles[members - 1, 1, :, 0, 5:9, :] *= np.float32(1e4)                       # mixed magnitudes under one pixel and across members
    tiles[1, 0, :, 0, 0, 0:4] = tiles[0, 0, :, 0, 0, 0:4]                         # ties after the blend
    tiles[0, 0, 0, 0, 3, 3] = np.nan                                             # under one tile only: one NaN pixel
    dev = torch.from_numpy(tiles).cuda()
    got = midd_amd.tile_blend_quantiles(dev, h, w, O, q=LEVELS)
    assert got.shape == (B, len(LEVELS), C, h, w) and got.dtype == torch.float32
    stacked = torch.stack([midd_amd.tile_blend(dev[m], h, w, O) for m in range(members)], dim=1)
    assert np.array_equal(_bits(got), _bits(midd_amd.ensemble_quantiles(stacked, LEVELS)))
    blended = np.stack([tiled_reference.blend(tiles[m], h, w, (O, O)) for m in range(members)], axis=1)
    assert np.array_equal(stacked.cpu().numpy(), blended, equal_nan=True)
    _check_against_restatement(got.cpu().numpy().reshape(B, len(LEVELS), -1), blended.reshape(B, members, -1), LEVELS)
    assert (_bits(got)[0, :, 0, 3, 3] == 0x7FC00000).all() and int(torch.isnan(got).sum()) == len(LEVELS)


def test_tile_equal_to_the_image_is_ensemble_quantiles():
    members, B, T = 5, 2, 32
    tiles = torch.from_numpy(np.random.default_rng(9).random((members, B, 1, 1, T, T), dtype=np.float32)).cuda()
    got = midd_amd.tile_blend_quantiles(tiles, T, T, 8, q=LEVELS)
    samples = tiles[:, :, 0].transpose(0, 1).contiguous()                        # [B, members, C, T, T]
    assert torch.equal(got, midd_amd.ensemble_quantiles(samples, LEVELS))
    with pytest.raises(ValueError, match="tiles per image"):
        midd_amd.tile_blend_quantiles(tiles, 40, 56, 8, q=LEVELS)


# ------------------------------------------------------------------------------ 3. the sampler calls
def test_denoise_ensemble_with_quantiles():
    den = _model()
    x = torch.from_numpy(synthetic_xray(2, 64, 64, seed=77)).cuda()
    kw = dict(inference_steps=K_STEPS, members=5, seed=SEED, return_samples=True)
    plain = den.denoise_ensemble(x, **kw)
    levels = (0.05, 0.5, 0.95)
    res = den.denoise_ensemble(x, quantiles=levels, **kw)
    assert isinstance(plain, midd_amd.EnsembleResult) and isinstance(res, midd_amd.EnsembleQuantileResult)
    assert res.levels == levels and res.seed == SEED and res.quantiles.shape == (2, 3, 1, 64, 64)
    assert torch.equal(res.mean, plain.mean) and torch.equal(res.std, plain.std) and torch.equal(res.samples, plain.samples)
    assert np.array_equal(_bits(res.quantiles), _bits(midd_amd.ensemble_quantiles(res.samples, levels)))
    assert torch.equal(res.quantiles[:, 1], res.samples.median(dim=1).values)
    assert np.array_equal(_bits(res.quantiles), _bits(qref.quantiles(res.samples.cpu().numpy(), levels)))
    assert (res.quantiles[:, 0] <= res.quantiles[:, 1]).all() and (res.quantiles[:, 1] <= res.quantiles[:, 2]).all()
    # without the samples: they are the call's own tensor, not returned; the same maps
    quiet = den.denoise_ensemble(x, inference_steps=K_STEPS, members=5, seed=SEED, quantiles=(0.0, 1.0))
    assert quiet.samples is None and torch.equal(quiet.mean, plain.mean) and torch.equal(quiet.std, plain.std)
    assert torch.equal(quiet.quantiles[:, 0], plain.samples.min(dim=1).values)
    assert torch.equal(quiet.quantiles[:, 1], plain.samples.max(dim=1).values)
    assert (quiet.quantiles[:, 0] <= quiet.mean).all() and (quiet.mean <= quiet.quantiles[:, 1]).all()
    mean, std, samples, seed = plain                                            # existing callers unpack four fields


def test_denoise_tiled_ensemble_with_quantiles():
    den = _model(batch_invariant=True)
    x = torch.from_numpy(synthetic_xray(1, 96, 80, seed=77)).cuda()
    kw = dict(inference_steps=K_STEPS, members=3, tile=64, overlap=16, seed=SEED, return_samples=True)
    plain = den.denoise_tiled_ensemble(x, **kw)
    levels = (0.05, 0.5, 0.95)
    maps = []
    for mb in (16, 3):                                                           # one pass of 4 tiles per member; passes of 3 and 1
        res = den.denoise_tiled_ensemble(x, quantiles=levels, max_batch=mb, **kw)
        assert isinstance(res, midd_amd.TiledEnsembleQuantileResult) and isinstance(plain, midd_amd.TiledEnsembleResult)
        assert res.levels == levels and res.quantiles.shape == (1, 3, 1, 96, 80) and res.tiles is None
        assert (res.origins_y, res.origins_x, res.seed) == (plain.origins_y, plain.origins_x, plain.seed)
        assert torch.equal(res.mean, plain.mean) and torch.equal(res.std, plain.std) and torch.equal(res.samples, plain.samples)
        assert np.array_equal(_bits(res.quantiles), _bits(midd_amd.ensemble_quantiles(res.samples, levels)))
        maps.append(res.quantiles)
    assert torch.equal(maps[0], maps[1])
    with_tiles = den.denoise_tiled_ensemble(x, quantiles=levels, return_tiles=True, **kw)
    assert with_tiles.tiles.shape == (3, 1, 4, 1, 64, 64) and torch.equal(with_tiles.quantiles, maps[0])
    assert torch.equal(midd_amd.tile_blend_quantiles(with_tiles.tiles, 96, 80, 16, q=levels), maps[0])


def test_status_word_after_a_quantile_call_is_the_samplers():
    """The quantile launch reads the members and writes its own tensor: the workspace's status word, and what check_status makes
    of it, are what the sampler passes left."""
    import ctypes as C
    den = _model()
    m = den.model
    x = torch.from_numpy(synthetic_xray(4, 64, 64, seed=77)).cuda()
    bad = x.clone()
    bad[0, 0, 5, 7] = float("nan")
    kw = dict(inference_steps=K_STEPS, members=2, seed=SEED, max_batch=2, quantiles=(0.5,))
    clean = den.denoise_ensemble(x, **kw)
    assert torch.isfinite(clean.quantiles).all()
    flags = C.c_int(-1)
    wptr, _ = m._aligned_ptr(m._ensemble_ws[1])
    assert native.lib().mi_status(wptr, torch.cuda.current_stream().cuda_stream, C.byref(flags)) == 0 and flags.value == 0
    with pytest.raises(native.MiddError) as ei:
        den.denoise_ensemble(bad, **kw)
    assert ei.value.code == -5
    m.check_status = False
    try:
        res = den.denoise_ensemble(bad, **kw)
        torch.cuda.synchronize()
        assert native.lib().mi_status(wptr, torch.cuda.current_stream().cuda_stream, C.byref(flags)) == -5
        assert flags.value & native.MI_STATUS_NONFINITE
    finally:
        m.check_status = True
    assert torch.isfinite(res.quantiles[1:]).all(), "the other images must not see image 0's NaN"
    assert torch.isfinite(den.denoise_ensemble(x, **kw).quantiles).all()         # the next call clears the word


# ------------------------------------------------------------------------------ 4. CLI
def test_cli_writes_the_quantile_maps_of_the_python_call(tmp_path):
    from midd_amd import cli, prepost
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in _sd().items()}, "noise_steps": 50}, ckpt)
    png = tmp_path / "in.png"
    Image.fromarray((synthetic_xray(1, 88, 120, seed=9)[0, 0].clip(0, 1) * 255).astype(np.uint8), mode="L").save(png)
    out, qout = tmp_path / "out.png", tmp_path / "q.npy"
    cli.main(["--image", str(png), "--out", str(out), "--checkpoint", str(ckpt), "--img-size", "64", "--inference-steps", str(K_STEPS),
              "--samples", "4", "--seed", "7", "--quantiles", "0.25,0.5", "--quantiles-out", str(qout)])
    got = np.load(qout)
    assert got.shape == (2, 64, 64) and got.dtype == np.float32 and np.isfinite(got).all() and (got[0] <= got[1]).all()
    raw = torch.from_numpy(np.asarray(Image.open(png).convert("L"), np.uint8).copy()).cuda()
    x = prepost.to_unit_float(prepost.resize_bicubic_u8(raw, (64, 64)))[None, None]
    res = _model().denoise_ensemble(x, inference_steps=K_STEPS, members=4, seed=7, quantiles=(0.25, 0.5))
    assert np.array_equal(_bits(got), _bits(res.quantiles[0, :, 0]))
    assert np.asarray(Image.open(out)).shape == (88, 120)
