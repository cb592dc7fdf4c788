"""CPU-only checks of fused tiled denoising (include/midd.h: THE CONSENSUS, mi_tile_consensus, mi_denoise_tiled_fused,
mi_tiled_fused_workspace_bytes): the numpy restatement of the consensus (tests/tiled_fused_reference.py), the argument rules of the
two C calls -- every one before any GPU work --, the host-only workspace size, and the rules of the new Python names and of the
CLI's --tile-fuse.  What the device computes is judged in test_gpu_tiled_fused.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetDiffusion, native
from tests import tiled_fused_reference as fref
from tests import tiled_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_tile_consensus", "mi_denoise_tiled_fused", "mi_tiled_fused_workspace_bytes"}
NOISY, IMAGE, TILES, HIST = 0x100000, 0x200000, 0x300000, 0x500000      # non-null "device pointers" for calls that must fail before anything reads them

# (H, W, tile, overlap): 3 x 3 tiles with triple cover on both axes; 2 x 3; 2 x 3 with a small overlap; a rectangular tile and overlap
GEOMETRIES = [(25, 27, (16, 16), (8, 8)), (41, 52, (24, 24), (12, 12)), (45, 59, (32, 32), (8, 8)), (40, 36, (16, 24), (8, 5))]


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


# ------------------------------------------------------------------------------ 1. the restatement of the consensus
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_reference_consensus_properties(geom):
    H, W, tile, overlap = geom
    if (H, W) == (25, 27):
        assert ref.origins(25, 16, 8) == [0, 4, 9] and ref.cover_counts(25, 16, 8).max() == 3 and ref.cover_counts(27, 16, 8).max() == 3
    K = len(ref.origins(H, tile[0], overlap[0])) * len(ref.origins(W, tile[1], overlap[1]))
    rng = np.random.default_rng(H * 100 + W)
    tiles = rng.standard_normal((2, K, 3) + tile).astype(np.float32)
    once, image = fref.consensus(tiles, H, W, overlap, return_image=True)
    assert once.dtype == np.float32 and once.shape == tiles.shape
    assert np.array_equal(image, ref.blend(tiles, H, W, overlap))
    assert np.array_equal(fref.consensus(once, H, W, overlap).view(np.int32), once.view(np.int32))      # idempotent
    assert np.array_equal(ref.blend(once, H, W, overlap), image)                                        # the tiles now agree: same image
    shared = fref.cover_mask(2, 3, H, W, tile, overlap)
    assert np.array_equal(once.view(np.int32)[~shared], tiles.view(np.int32)[~shared])                  # single cover: the bits stay
    changed = float((once != tiles).mean())
    print(f"{geom}: {changed:.4f} of the elements change, {float(shared.mean()):.4f} lie under more than one tile")
    # every element under more than one tile changes (Gaussian values never blend to themselves); in whole percent that is 88 .. 96 %
    # for these geometries (0.9570, 0.9533, 0.8857 and 0.8750, the last being exactly 7 / 8: the share is a property of the geometry)
    assert changed == float(shared.mean()) and 88 <= int(100.0 * changed + 0.5) <= 96


# ------------------------------------------------------------------------------ 2. the symbols
def test_header_and_binding_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in native.SYMBOLS}
    assert NEW <= declared and NEW <= bound
    for name in NEW:
        assert getattr(native.lib(), name) is not None
    assert "THE CONSENSUS" in header


# ------------------------------------------------------------------------------ 3. argument rules, before any GPU work
def _consensus(tiles=TILES, B=2, Cc=1, H=90, W=70, th=32, tw=32, oy=8, ox=8, image=None):
    return native.lib().mi_tile_consensus(tiles, B, Cc, H, W, th, tw, oy, ox, image, None)


@pytest.mark.parametrize("kw,words", [
    (dict(Cc=0), ["C 0"]),
    (dict(th=96), ["tile <= image", "96", "90"]),
    (dict(tw=0), ["positive"]),
    (dict(oy=-1), ["overlap", "tile / 2"]),
    (dict(ox=17), ["overlap", "tile / 2", "16"]),
    (dict(H=100000, W=100000, th=100000, tw=100000, oy=50000, ox=0), ["46339"]),
    (dict(H=65536, W=65536), ["2^32", "4294967296"]),
    (dict(B=1 << 30, H=64, W=64, oy=0, ox=0), ["2147483647"]),
    (dict(B=0), ["B 0"]),
    (dict(tiles=None), ["null"]),
    (dict(image=TILES), ["alias", "tiles", "image_out"]),
    (dict(image=TILES + 2 * 12 * 32 * 32 * 4 - 4), ["alias", "tiles", "image_out"]),        # the last float of the tiles (4 x 3 of them)
    (dict(tiles=IMAGE + 2 * 90 * 70 * 4 - 4, image=IMAGE), ["alias", "tiles", "image_out"]),  # the last float of image_out
])
def test_every_consensus_rule_names_its_limit(kw, words):
    """What mi_tile_blend refuses, and an image_out that overlaps the tiles.  The pointers are not device memory: a call that got
    as far as a launch would not return MI_EINVAL."""
    lib = native.lib()
    assert _consensus(**kw) == -1, kw
    msg = lib.mi_last_error().decode()
    for w in words:
        assert w in msg, (kw, msg)
    if "image" not in kw and kw.get("tiles", TILES) is not None:               # the same refusal as the blend's, word for word
        a = dict(tiles=TILES, B=2, Cc=1, H=90, W=70, th=32, tw=32, oy=8, ox=8)
        a.update(kw)
        assert lib.mi_tile_blend(a["tiles"], a["B"], a["Cc"], a["H"], a["W"], a["th"], a["tw"], a["oy"], a["ox"], IMAGE, None) == -1
        assert lib.mi_last_error().decode() == msg


def _fused(plan, noisy=NOISY, image=IMAGE, tiles=None, hist=None, B=2, H=90, W=70, th=32, tw=32, oy=8, ox=8, seeded=1, seed=5,
           sample_offset=0, pass_samples=16, rule=None, t_list=None, tables=True):
    steps = np.ascontiguousarray(np.asarray([] if t_list is None else t_list, dtype=np.int32))
    tabs = [np.linspace(0.9, 0.1, 50).astype(np.float32) for _ in range(3)]
    ptrs = [t.ctypes.data_as(C.POINTER(C.c_float)) for t in tabs] if tables else [None] * 3
    return native.lib().mi_denoise_tiled_fused(plan, noisy, image, tiles, hist, B, H, W, th, tw, oy, ox,
                                               steps.ctypes.data_as(C.POINTER(C.c_int32)), len(steps), *ptrs, 50,
                                               seeded, seed, sample_offset, pass_samples, 0,
                                               None if rule is None else C.byref(rule), None, 0, None)


DDIM = native.UpdateRule(native.MI_UPDATE["ddim"], 0.5, 1)
DPM = native.UpdateRule(native.MI_UPDATE["dpmpp2m"], 0.0, 1)
TILE_BYTES = 2 * 12 * 32 * 32 * 4                                              # B = 2 images of 4 x 3 tiles


@pytest.mark.parametrize("kw,words", [
    (dict(th=36), ["multiples of 8"]),
    (dict(tw=4), ["multiples of 8"]),
    (dict(th=96), ["tile <= image", "96", "90"]),
    (dict(oy=-1), ["overlap", "tile / 2"]),
    (dict(ox=17), ["overlap", "tile / 2", "16"]),
    (dict(pass_samples=0), ["pass_samples >= 1"]),
    (dict(sample_offset=-2), ["sample_offset -2"]),
    (dict(H=65536, W=65536), ["2^32", "4294967296"]),
    (dict(B=1 << 30, H=64, W=64, oy=0, ox=0), ["2147483647"]),
    (dict(B=0), ["B 0"]),
    (dict(image=NOISY), ["alias", "noisy", "image_out"]),
    (dict(tiles=NOISY + 4), ["alias", "noisy", "tiles_out"]),
    (dict(tiles=IMAGE + 2 * 90 * 70 * 4 - 4), ["alias", "image_out", "tiles_out"]),
    (dict(rule=DPM, seeded=0, hist=NOISY + 8), ["alias", "noisy", "x0_hist"]),
    (dict(rule=DPM, seeded=0, hist=IMAGE), ["alias", "image_out", "x0_hist"]),
    (dict(rule=DPM, seeded=0, tiles=TILES, hist=TILES + TILE_BYTES - 4), ["alias", "tiles_out", "x0_hist"]),      # x0_hist holds every tile
    (dict(rule=DPM, seeded=0), ["MI_UPDATE_DPMPP2M", "x0_hist"]),                                                   # the rule needs it
    (dict(rule=DPM, seeded=1, hist=HIST), ["seeded", "MI_UPDATE_DPMPP2M"]),
    (dict(hist=HIST), ["x0_hist", "reference"]),                                                                    # no other rule takes it
    (dict(rule=DDIM, hist=HIST), ["x0_hist", "MI_UPDATE_DDIM"]),
    (dict(rule=native.UpdateRule(native.MI_UPDATE["ddim"], 1.5, 1)), ["eta"]),
    (dict(rule=native.UpdateRule(7, 0.0, 1)), ["unknown update rule"]),
    (dict(rule=DDIM, t_list=[10, 20]), ["strictly decreasing"]),
    (dict(rule=DPM, seeded=0, hist=HIST, t_list=[10, 20]), ["strictly decreasing"]),
])
def test_every_argument_rule_of_the_fused_call_names_its_limit(plan, kw, words):
    lib = native.lib()
    assert _fused(plan, **kw) == -1, kw
    msg = lib.mi_last_error().decode()
    for w in words:
        assert w in msg, (kw, msg)
    a = dict(B=2, H=90, W=70, th=32, tw=32, oy=8, ox=8, pass_samples=16)
    a.update({k: v for k, v in kw.items() if k in a})
    if a != dict(B=2, H=90, W=70, th=32, tw=32, oy=8, ox=8, pass_samples=16):  # the workspace query judges the same geometry
        assert lib.mi_tiled_fused_workspace_bytes(plan, a["B"], a["H"], a["W"], a["th"], a["tw"], a["oy"], a["ox"], a["pass_samples"], 0) == 0, kw


def test_valid_arguments_reach_the_state_check(plan):
    """Inside every limit the unfinalized plan stops the call (a state error, still before any GPU work)."""
    lib = native.lib()
    assert _fused(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _fused(plan, H=32, W=32) == -2                                      # tile == image
    assert _fused(plan, seeded=0, tiles=TILES) == -2
    assert _fused(plan, rule=DDIM, t_list=[40, 20, 0]) == -2
    assert _fused(plan, rule=DPM, seeded=0, hist=HIST, tiles=TILES, t_list=[40, 20, 0]) == -2
    assert _fused(plan, rule=DPM, seeded=0, tiles=TILES, hist=TILES + TILE_BYTES) == -2      # touching, not overlapping
    assert _fused(plan, image=NOISY + 2 * 90 * 70 * 4) == -2
    assert _fused(None) == -1 and b"null plan" in lib.mi_last_error()


# ------------------------------------------------------------------------------ 4. workspace size (host only, before finalize)
def test_workspace_bytes_on_an_unfinalized_plan(plan):
    lib = native.lib()
    ws, plain = lib.mi_tiled_fused_workspace_bytes, lib.mi_tiled_workspace_bytes
    H, W, T, O = 90, 70, 32, 8                                                 # 4 x 3 tiles
    K, tile_bytes = 12, 1 * T * T * 4

    def round256(n):
        return (n + 255) // 256 * 256

    for B, p in [(1, 4), (2, 16), (1, 5), (1, 12)]:
        ext, internal = ws(plan, B, H, W, T, T, O, O, p, 1), ws(plan, B, H, W, T, T, O, O, p, 0)
        assert ext > 0 and internal - ext == B * K * tile_bytes               # the tile states, exactly
        # the unfused call keeps one pass of condition tiles, this one those of the whole batch: nothing else differs
        n_pass = min(p, B * K)
        assert ext - plain(plan, B, H, W, T, T, O, O, p, 1) == round256(B * K * tile_bytes) - round256(n_pass * tile_bytes)
    assert ws(plan, 1, H, W, T, T, O, O, 12, 0) == ws(plan, 1, H, W, T, T, O, O, 1000, 0)
    assert ws(None, 1, H, W, T, T, O, O, 4, 0) == 0
    m = UNetDiffusion(variant="cddpm", **SMALL)
    assert "condition tiles of ALL" in m.tiled_fused_workspace_bytes.__doc__


# ------------------------------------------------------------------------------ 5. Python surface
def test_python_surface_without_a_gpu():
    import inspect
    sig = inspect.signature(DiffusionDenoiser.denoise_tiled_fused)
    assert list(sig.parameters) == ["self", "noisy_img", "inference_steps", "tile", "overlap", "max_batch", "seed", "sample_offset",
                                    "return_tiles", "update", "eta", "clip_x0"]
    assert [sig.parameters[k].default for k in ("inference_steps", "tile", "overlap", "max_batch", "seed", "sample_offset", "return_tiles",
                                                "update", "eta", "clip_x0")] == [25, 256, 32, 16, None, 0, False, "reference", 0.0, True]
    assert sig.parameters["update"].kind is inspect.Parameter.KEYWORD_ONLY and sig.return_annotation in (midd_amd.TiledResult, "TiledResult")
    csig = inspect.signature(midd_amd.tile_consensus)
    assert list(csig.parameters) == ["tiles", "H", "W", "overlap", "inplace", "return_image"]
    assert [csig.parameters[k].default for k in ("overlap", "inplace", "return_image")] == [32, False, False]
    assert midd_amd.sampler.tile_consensus is midd_amd.tile_consensus
    assert hasattr(UNetDiffusion, "run_tiled_fused") and hasattr(UNetDiffusion, "tiled_fused_workspace_bytes")
    x = torch.zeros(1, 1, 40, 48)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="seed=None"):
        ddim.denoise_tiled_fused(x, inference_steps=2, tile=32, overlap=8, seed=1)
    with pytest.raises(ValueError, match="dpmpp2m.*no seed"):
        ddim.denoise_tiled_fused(x, inference_steps=2, tile=32, overlap=8, seed=1, update="dpmpp2m")
    with pytest.raises(ValueError, match="eta"):
        ddim.denoise_tiled_fused(x, inference_steps=2, tile=32, overlap=8, eta=0.5)
    with pytest.raises(TypeError):
        ddim.denoise_tiled_fused(x, inference_steps=2, tile=32, overlap=8, step_noise=torch.zeros(1))      # there is no such argument
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="max_batch"):
        d.denoise_tiled_fused(x, inference_steps=2, tile=32, overlap=8, seed=1, max_batch=0)
    with pytest.raises(ValueError, match="sample_offset"):
        d.denoise_tiled_fused(x, inference_steps=2, tile=32, overlap=8, seed=1, sample_offset=-1)
    for den in (ddim, d):                                                      # valid arguments, CPU tensors: never a silent fall-back
        for kw in ({}, {"update": "ddim"}, {"update": "dpmpp2m"}):
            with pytest.raises(RuntimeError, match="noisy_img is on cpu: the MI355X path has no CPU fallback"):
                den.denoise_tiled_fused(x, inference_steps=2, tile=32, overlap=8, **kw)
    with pytest.raises(RuntimeError, match="tiles is on cpu: tiling runs only on a ROCm GPU, there is no CPU fallback"):
        midd_amd.tile_consensus(torch.zeros(1, 4, 1, 32, 32), 40, 48, 8)
    with pytest.raises(ValueError, match="5-dimensional"):
        midd_amd.tile_consensus(torch.zeros(4, 1, 32, 32), 40, 48, 8)
    with pytest.raises(ValueError, match="contiguous"):
        midd_amd.tile_consensus(torch.zeros(1, 4, 1, 32, 64)[..., ::2], 40, 48, 8, inplace=True)
    with pytest.raises(ValueError, match="tile must be in"):
        ddim.model.tiled_fused_workspace_bytes(1, 16, 16, tile=0)


# ------------------------------------------------------------------------------ 6. CLI
def test_cli_tile_fuse_rules(tmp_path):
    import inspect
    from midd_amd import cli
    assert inspect.signature(cli.denoise_image_diffusion).parameters["tile_fuse"].default == "end"
    assert inspect.signature(cli.check_options).parameters["tile_fuse"].default == "end"
    cli.check_options(tile=64, tile_fuse="step", variant="ddim")
    cli.check_options(tile=64, tile_fuse="step", update="dpmpp2m", variant="ddim", bit_depth=16, window=(1.0, 99.0))
    cli.check_options(tile=64, tile_fuse="step", update="ddim", eta=0.5, seed=3)
    cli.check_options(tile_fuse="end")                                         # the default needs nothing
    with pytest.raises(ValueError, match=r"--tile-fuse step .* needs --tile N"):
        cli.check_options(tile_fuse="step")
    for flag, kw in (("--members", dict(members=4)), ("--views", dict(views="auto")), ("--samples", dict(samples=4)),
                     ("--self-ensemble", dict(self_ensemble="auto"))):
        with pytest.raises(ValueError, match=f"--tile-fuse step cannot be combined with {flag}"):
            cli.check_options(tile=64, tile_fuse="step", **kw)
    with pytest.raises(ValueError, match="--tile-fuse takes end or step"):
        cli.check_options(tile=64, tile_fuse="both")
    for argv in (["--tile-fuse", "step"], ["--tile", "64", "--tile-fuse", "both"], ["--tile", "64", "--tile-fuse", "step", "--members", "4"],
                 ["--tile", "64", "--tile-fuse", "step", "--views"], ["--tile-fuse", "step", "--samples", "4"],
                 ["--tile-fuse", "step", "--self-ensemble"]):
        with pytest.raises(SystemExit) as ei:
            cli.main(argv + ["--image", "nowhere.png"])
        assert ei.value.code == 2, argv
