"""CPU-only checks of tiled denoising (include/midd.h: mi_tile_geometry, mi_denoise_tiled, mi_tiled_workspace_bytes): the host
geometry against its numpy restatement (tests/tiled_reference.py), the argument rules of the C ABI, the host-only workspace
size and the Python argument rules.  What the device computes is judged in test_gpu_tiled.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetDiffusion, native
from tests import tiled_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_tile_geometry", "mi_tile_extract", "mi_tile_blend", "mi_denoise_tiled", "mi_tiled_workspace_bytes"}
NOISY, IMAGE, TILES = 0x100000, 0x200000, 0x300000      # non-null "device pointers" for calls that must fail before anything reads them


@pytest.fixture()
def plan():
    """An unfinalized cddpm plan: every host-side rule can be checked on it, no GPU call can succeed."""
    lib = native.lib()
    m = UNetDiffusion(variant="cddpm", **SMALL)
    cfg = native.UNetCfg()
    c = m.cfg
    cfg.in_channels, cfg.model_channels, cfg.num_levels = c.in_channels, c.model_channels, len(c.channel_mult)
    for i, v in enumerate(c.channel_mult):
        cfg.channel_mult[i] = v
    cfg.num_res_blocks, cfg.num_attention_levels = c.num_res_blocks, len(c.attention_resolutions)
    for i, v in enumerate(c.attention_resolutions):
        cfg.attention_levels[i] = v
    cfg.time_emb_dim, cfg.variant, cfg.compute_mode = c.time_emb_dim, native.MI_VARIANT["cddpm"], native.MI_COMPUTE["f16x3"]
    h = C.c_void_p()
    native.check(lib.mi_unet_plan_create(C.byref(cfg), C.byref(h)))
    yield h
    lib.mi_plan_destroy(h)


def _geometry(L, T, O):
    lib = native.lib()
    n = C.c_int(-1)
    rc = lib.mi_tile_geometry(L, T, O, C.byref(n), None, 0)
    if rc:
        return rc, None
    buf = (C.c_int * n.value)()
    assert lib.mi_tile_geometry(L, T, O, C.byref(n), buf, n.value) == 0
    return 0, list(buf)


# ------------------------------------------------------------------------------ 1. geometry
def test_header_and_binding_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in native.SYMBOLS}
    assert NEW <= declared and declared == bound
    for name in NEW:
        assert getattr(native.lib(), name) is not None
    assert "(c*H_img + y0 + y)*W_img + x0 + x" in header                      # the tiled form of counter word c0


@pytest.mark.parametrize("T", [16, 24, 32, 64])
def test_geometry_equals_the_restatement_and_covers(T):
    for O in range(0, T // 2 + 1):
        for L in range(T, 4 * T + 3):
            rc, got = _geometry(L, T, O)
            assert rc == 0, (L, T, O)
            want = ref.origins(L, T, O)
            assert got == want, (L, T, O, got, want)
            n = len(got)
            assert n == ref.tile_count(L, T, O) and (n == 1) == (L == T)
            assert got[0] == 0 and got[-1] == L - T                          # end alignment
            cover = ref.cover_counts(L, T, O)
            assert cover.min() >= 1 and cover.max() <= 3, (L, T, O, cover.max())   # every pixel; at most 3 tiles over one
            for a, b in zip(got, got[1:]):
                assert a + T - b >= O and b > a, (L, T, O, got)              # consecutive tiles overlap by at least O
    w = ref.window(T, T // 4)
    assert w[0] == 1 and w[-1] == 1 and w.max() == T // 4 + 1 and (w == w[::-1]).all()


def test_geometry_writes_at_most_cap_origins_and_refuses_bad_axes():
    lib = native.lib()
    n = C.c_int()
    buf = (C.c_int * 4)(-7, -7, -7, -7)
    assert lib.mi_tile_geometry(59, 32, 8, C.byref(n), buf, 2) == 0
    assert n.value == 3 and list(buf) == [0, 13, -7, -7]
    for (L, T, O), word in [((31, 32, 8), "tile <= image"), ((64, 32, 17), "tile / 2"), ((64, 32, -1), "overlap"), ((64, 0, 0), "positive")]:
        assert lib.mi_tile_geometry(L, T, O, C.byref(n), None, 0) == -1
        assert word in lib.mi_last_error().decode(), (L, T, O, lib.mi_last_error())
    assert lib.mi_tile_geometry(64, 32, 8, None, None, 0) == -1


# ------------------------------------------------------------------------------ 2. argument rules, before any GPU work
def _tiled(plan, noisy=NOISY, image=IMAGE, tiles=None, B=2, H=90, W=70, th=32, tw=32, oy=8, ox=8, seeded=1, seed=5,
           sample_offset=0, pass_samples=16):
    return native.lib().mi_denoise_tiled(plan, noisy, image, tiles, B, H, W, th, tw, oy, ox, None, 0, None, None, None, 50,
                                         seeded, seed, sample_offset, pass_samples, 0, None, 0, None)


@pytest.mark.parametrize("kw,words", [
    (dict(th=36), ["multiples of 8"]),                                        # a tile the planner rejects
    (dict(tw=4), ["multiples of 8"]),
    (dict(th=0), ["multiples of 8"]),
    (dict(th=96), ["tile <= image", "96", "90"]),                             # T > L
    (dict(tw=72), ["tile <= image"]),
    (dict(oy=-1), ["overlap", "tile / 2"]),
    (dict(ox=17), ["overlap", "tile / 2", "16"]),
    (dict(pass_samples=0), ["pass_samples >= 1"]),
    (dict(image=NOISY), ["alias", "noisy", "image_out"]),
    (dict(tiles=NOISY + 4), ["alias", "noisy", "tiles_out"]),
    (dict(tiles=IMAGE + 2 * 90 * 70 * 4 - 4), ["alias", "image_out", "tiles_out"]),     # the last float of image_out
    (dict(sample_offset=-2), ["sample_offset -2"]),
    (dict(H=65536, W=65536), ["2^32", "4294967296"]),
    (dict(B=1 << 30, H=64, W=64, oy=0, ox=0), ["2147483647"]),                # 2^30 images x 4 tiles
    (dict(B=0), ["B 0"]),
])
def test_every_argument_rule_names_its_limit(plan, kw, words):
    lib = native.lib()
    assert _tiled(plan, **kw) == -1, kw
    msg = lib.mi_last_error().decode()
    for w in words:
        assert w in msg, (kw, msg)
    # the workspace query judges the same geometry
    a = dict(B=2, H=90, W=70, th=32, tw=32, oy=8, ox=8, pass_samples=16)
    a.update({k: v for k, v in kw.items() if k in a})
    if a != dict(B=2, H=90, W=70, th=32, tw=32, oy=8, ox=8, pass_samples=16):
        assert lib.mi_tiled_workspace_bytes(plan, a["B"], a["H"], a["W"], a["th"], a["tw"], a["oy"], a["ox"], a["pass_samples"], 0) == 0, kw


def test_valid_arguments_reach_the_state_check(plan):
    """Inside every limit the unfinalized plan stops the call (a state error, still before any GPU work)."""
    lib = native.lib()
    assert _tiled(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _tiled(plan, H=32, W=32) == -2                                      # tile == image
    assert _tiled(plan, oy=16, ox=0) == -2                                     # the ends of the overlap range
    assert _tiled(plan, seeded=0, tiles=TILES) == -2
    assert _tiled(plan, image=NOISY + 2 * 90 * 70 * 4) == -2                   # touching, not overlapping
    assert _tiled(None) == -1 and b"null plan" in lib.mi_last_error()
    # the plan-free kernels judge their geometry on the host too
    assert lib.mi_tile_blend(TILES, 1, 1, 40, 40, 48, 32, 8, 8, IMAGE, None) == -1 and b"tile <= image" in lib.mi_last_error()
    assert lib.mi_tile_blend(None, 1, 1, 40, 40, 32, 32, 8, 8, IMAGE, None) == -1 and b"null" in lib.mi_last_error()
    assert lib.mi_tile_extract(NOISY, 1, 1, 40, 40, 32, 32, 20, 8, 0, 1, TILES, None) == -1 and b"tile / 2" in lib.mi_last_error()
    assert lib.mi_tile_extract(NOISY, 1, 1, 40, 40, 32, 32, 8, 8, 3, 2, TILES, None) == -1 and b"outside" in lib.mi_last_error()
    assert lib.mi_tile_extract(None, 1, 1, 40, 40, 32, 32, 8, 8, 0, 0, None, None) == 0      # nothing to copy


# ------------------------------------------------------------------------------ 3. workspace size (host only)
def test_workspace_bytes_on_an_unfinalized_plan(plan):
    lib = native.lib()
    ws = lib.mi_tiled_workspace_bytes
    H, W, T, O = 90, 70, 32, 8                                                 # 4 x 3 tiles
    K = len(ref.origins(H, T, O)) * len(ref.origins(W, T, O))
    assert K == 12
    tile_bytes = 1 * T * T * 4
    sizes = [ws(plan, 1, H, W, T, T, O, O, p, 1) for p in (1, 2, 4, 8, 12)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0], sizes      # grows with pass_samples
    for B, p in [(1, 4), (2, 16), (1, 5)]:
        ext, internal = ws(plan, B, H, W, T, T, O, O, p, 1), ws(plan, B, H, W, T, T, O, O, p, 0)
        assert internal - ext == B * K * tile_bytes                            # the tile outputs, exactly
        # a pass of tiles is an ensemble pass at the tile's shape: same sampler workspace, same condition buffer
        assert ext == lib.mi_ensemble_workspace_bytes(plan, B, K, T, T, p, 1)
    assert ws(plan, 1, H, W, T, T, O, O, 12, 0) == ws(plan, 1, H, W, T, T, O, O, 1000, 0)      # a pass larger than the image's tiles
    assert ws(None, 1, H, W, T, T, O, O, 4, 0) == 0


# ------------------------------------------------------------------------------ 4. the restatement itself
def test_reference_blend_properties():
    rng = np.random.default_rng(5)
    H, W, T, O = 45, 59, 32, 8
    x = rng.standard_normal((2, 3, H, W)).astype(np.float32)
    tiles = ref.extract(x, (T, T), (O, O))
    assert tiles.shape == (2, 6, 3, T, T)
    assert np.array_equal(ref.blend(tiles, H, W, (O, O)), x)                   # tiles that agree where they overlap blend to the image
    const = np.full_like(tiles, np.float32(0.3))
    assert (ref.blend(const, H, W, (O, O)) == np.float32(0.3)).all()


# ------------------------------------------------------------------------------ 5. Python surface
def test_python_surface_without_a_gpu():
    assert midd_amd.TiledResult._fields == ("image", "tiles", "origins_y", "origins_x", "seed")
    p = midd_amd.tile_plan(45, 59, 32, 8)
    assert p.tile == (32, 32) and p.overlap == (8, 8) and p.origins_y == (0, 13) and p.origins_x == (0, 13, 27)
    assert midd_amd.tile_plan(56, 56, (32, 32), (16, 16)).origins_y == (0, 12, 24)
    with pytest.raises(native.MiddError, match="tile <= image"):
        midd_amd.tile_plan(30, 64, 32, 8)
    with pytest.raises(ValueError, match="tile"):
        midd_amd.tile_plan(64, 64, 1.5, 8)
    x = torch.zeros(1, 1, 40, 48)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="seed=None"):
        ddim.denoise_tiled(x, inference_steps=2, tile=32, overlap=8, seed=1)
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="max_batch"):
        d.denoise_tiled(x, inference_steps=2, tile=32, overlap=8, seed=1, max_batch=0)
    with pytest.raises(ValueError, match="sample_offset"):
        d.denoise_tiled(x, inference_steps=2, tile=32, overlap=8, seed=1, sample_offset=-1)
    with pytest.raises(ValueError, match="step_noise"):
        d.denoise_tiled(x, inference_steps=2, tile=32, overlap=8, seed=1, step_noise=torch.zeros(1))
    for den in (ddim, d):                                                      # valid arguments, CPU tensors: never a silent fall-back
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            den.denoise_tiled(x, inference_steps=2, tile=32, overlap=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.tile_blend(torch.zeros(1, 4, 1, 32, 32), 40, 48, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.tile_extract(x, 32, 8)


def test_cli_accepts_tile_and_overlap(tmp_path):
    import inspect
    from PIL import Image
    from midd_amd import cli
    sig = inspect.signature(cli.denoise_image_diffusion).parameters
    assert sig["tile"].default is None and sig["overlap"].default == 32
    for argv in (["--tile", "x"], ["--tile", "0"], ["--tile", "64", "--samples", "4"]):
        with pytest.raises(SystemExit):
            cli.main(argv + ["--image", "nowhere.png"])
    png = tmp_path / "small.png"
    Image.fromarray(np.zeros((40, 100), np.uint8), mode="L").save(png)
    with pytest.raises(ValueError, match="img_size"):                          # a side shorter than the tile
        cli.denoise_image_diffusion(None, str(png), device_type="cpu", variant="ddim", tile=64, overlap=16)
