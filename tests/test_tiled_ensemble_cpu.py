"""CPU-only checks of ensembles of tiled runs (include/midd.h: mi_denoise_tiled_ensemble, mi_tiled_ensemble_workspace_bytes,
mi_tile_blend_reduce): the argument rules of the C ABI on an unfinalized plan, the host-only workspace size, the numpy
restatement and the Python argument rules.  What the device computes is judged in test_gpu_tiled_ensemble.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetDiffusion, native
from tests import ensemble_reference, tiled_reference
from tests import tiled_ensemble_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_denoise_tiled_ensemble", "mi_tiled_ensemble_workspace_bytes", "mi_tile_blend_reduce"}
# non-null "device pointers", 1 MiB apart, for calls that must fail before anything reads them (every buffer below is < 1 MiB)
NOISY, MEAN, STD, SAMPLES, TILES = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
IMG_BYTES = 2 * 90 * 70 * 4                                 # noisy / mean_out / std_out of the default case below


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


def test_header_and_binding_declare_the_three_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in native.SYMBOLS}
    assert NEW <= declared and NEW <= bound and declared == bound
    for name in NEW:
        assert getattr(native.lib(), name) is not None
    assert "seed, sample_offset   as mi_denoise_seeded (sample_offset counts IMAGES); c3 is 0" in header      # still true of mi_denoise_tiled
    assert "c3 = member_offset + m" in header


# ------------------------------------------------------------------------------ 1. argument rules, before any GPU work
DEFAULT = dict(noisy=NOISY, mean=MEAN, std=STD, samples=None, tiles=None, B=2, members=3, H=90, W=70, th=32, tw=32, oy=8, ox=8,
               seed=5, sample_offset=0, member_offset=0, pass_samples=16)


def _call(plan, **kw):
    a = dict(DEFAULT)
    a.update(kw)
    return native.lib().mi_denoise_tiled_ensemble(
        plan, a["noisy"], a["mean"], a["std"], a["samples"], a["tiles"], a["B"], a["members"], a["H"], a["W"], a["th"], a["tw"],
        a["oy"], a["ox"], None, 0, None, None, None, 50, a["seed"], a["sample_offset"], a["member_offset"], a["pass_samples"], 0,
        None, 0, None)


@pytest.mark.parametrize("kw,words", [
    # the tile rules (mi_denoise_tiled's)
    (dict(th=36), ["multiples of 8"]),
    (dict(tw=4), ["multiples of 8"]),
    (dict(th=0), ["multiples of 8"]),
    (dict(th=96), ["tile <= image", "96", "90"]),
    (dict(tw=72), ["tile <= image"]),
    (dict(oy=-1), ["overlap", "tile / 2"]),
    (dict(ox=17), ["overlap", "tile / 2", "16"]),
    (dict(pass_samples=0), ["pass_samples >= 1"]),
    (dict(sample_offset=-2), ["sample_offset -2"]),
    (dict(H=65536, W=65536), ["2^32", "4294967296"]),
    (dict(B=1 << 30, H=64, W=64, oy=0, ox=0), ["B * tiles", "2147483647"]),   # 2^30 images x 4 tiles
    (dict(B=0), ["B 0"]),
    # the member rules (mi_denoise_ensemble's)
    (dict(members=0), ["members 0", "members >= 1"]),
    (dict(member_offset=-1), ["member_offset -1"]),
    (dict(member_offset=(1 << 32) - 2), ["2^32", "4294967296"]),              # + 3 members
    (dict(members=1), ["std_out", "members >= 2"]),
    (dict(mean=None, std=None), ["no output", "tiles_out"]),
    # B * members * tiles: 2^20 images x 4 tiles pass the tile rule, x 2^10 members do not
    (dict(B=1 << 20, H=64, W=64, oy=0, ox=0, members=1 << 10), ["B * members * tiles", "2147483647"]),
    # each aliasing pair of the five buffers
    (dict(mean=NOISY), ["alias", "noisy", "mean_out"]),
    (dict(std=NOISY + IMG_BYTES - 4), ["alias", "noisy", "std_out"]),         # the last float of noisy
    (dict(samples=NOISY + 4), ["alias", "noisy", "samples_out"]),
    (dict(tiles=NOISY + 4), ["alias", "noisy", "tiles_out"]),
    (dict(std=MEAN), ["alias", "mean_out", "std_out"]),
    (dict(samples=MEAN + IMG_BYTES - 4), ["alias", "mean_out", "samples_out"]),
    (dict(tiles=MEAN - 4), ["alias", "mean_out", "tiles_out"]),               # tiles_out runs into mean_out
    (dict(samples=STD - 4), ["alias", "std_out", "samples_out"]),
    (dict(tiles=STD + 8), ["alias", "std_out", "tiles_out"]),
    (dict(samples=SAMPLES, tiles=SAMPLES + 3 * IMG_BYTES - 4), ["alias", "samples_out", "tiles_out"]),      # the last float of samples_out
])
def test_every_argument_rule_names_its_limit(plan, kw, words):
    lib = native.lib()
    assert _call(plan, **kw) == -1, kw
    msg = lib.mi_last_error().decode()
    for w in words:
        assert w in msg, (kw, msg)
    # the workspace query judges the same geometry and the same member count
    keys = ("B", "members", "H", "W", "th", "tw", "oy", "ox", "pass_samples")
    a = {k: DEFAULT[k] for k in keys}
    a.update({k: v for k, v in kw.items() if k in a})
    if a != {k: DEFAULT[k] for k in keys} and a["members"] != 1:
        assert lib.mi_tiled_ensemble_workspace_bytes(plan, *[a[k] for k in keys], 0) == 0, kw


def test_valid_arguments_reach_the_state_check(plan):
    """Inside every limit the unfinalized plan stops the call (a state error, still before any GPU work)."""
    lib = native.lib()
    assert _call(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _call(plan, samples=SAMPLES, tiles=TILES) == -2
    assert _call(plan, mean=None, std=None, tiles=TILES) == -2                 # the tiles alone are an output
    assert _call(plan, members=1, std=None) == -2                              # one member: a mean, no std
    assert _call(plan, member_offset=(1 << 32) - 3) == -2                      # the last three member words
    assert _call(plan, H=32, W=32) == -2                                       # tile == image
    assert _call(plan, mean=NOISY + IMG_BYTES) == -2                           # touching, not overlapping
    assert _call(plan, samples=SAMPLES, tiles=SAMPLES + 3 * IMG_BYTES) == -2
    assert _call(plan, B=1 << 20, H=64, W=64, oy=0, ox=0, members=511, mean=None, std=None, tiles=TILES, noisy=None) == -2      # 2^31 - 2^22 tiles
    assert _call(None) == -1 and b"null plan" in lib.mi_last_error()


def test_blend_reduce_rules():
    lib = native.lib()

    def call(tiles=TILES, B=2, members=3, Cc=1, H=45, W=59, th=32, tw=32, oy=8, ox=8, mean=MEAN, std=STD, samples=None):
        return lib.mi_tile_blend_reduce(tiles, B, members, Cc, H, W, th, tw, oy, ox, mean, std, samples, None)

    for kw, word in [(dict(th=48), "tile <= image"), (dict(ox=17), "tile / 2"), (dict(oy=-1), "overlap"), (dict(Cc=0), "C 0"),
                     (dict(H=65536, W=65536), "4294967296"), (dict(B=0), "B 0"), (dict(B=65536), "65535"),
                     (dict(B=1 << 30, H=64, W=64, oy=0, ox=0), "B * tiles"),
                     (dict(B=1 << 15, H=64, W=64, oy=0, ox=0, members=1 << 15), "B * members * tiles"),
                     (dict(members=0), "members >= 1"), (dict(members=1), "members >= 2"),
                     (dict(tiles=None), "null"), (dict(mean=None), "null")]:
        assert call(**kw) == -1, kw
        assert word in lib.mi_last_error().decode(), (kw, lib.mi_last_error())


# ------------------------------------------------------------------------------ 2. workspace size (host only)
def test_workspace_bytes_on_an_unfinalized_plan(plan):
    lib = native.lib()
    ws, tiled = lib.mi_tiled_ensemble_workspace_bytes, lib.mi_tiled_workspace_bytes
    H, W, T, O = 90, 70, 32, 8                                                 # 4 x 3 tiles
    K = len(tiled_reference.origins(H, T, O)) * len(tiled_reference.origins(W, T, O))
    assert K == 12
    tile_bytes = 1 * T * T * 4
    for B, M, p in [(1, 1, 4), (1, 3, 4), (2, 3, 16), (1, 8, 5), (2, 2, 1000)]:    # (a pass of 5: a tail of 2; 1000: one pass per member)
        internal, ext = ws(plan, B, M, H, W, T, T, O, O, p, 0), ws(plan, B, M, H, W, T, T, O, O, p, 1)
        assert internal > 0 and ext > 0
        # the passes of a member are mi_denoise_tiled's: its workspace, and the tiles of the other members - 1
        assert internal == tiled(plan, B, H, W, T, T, O, O, p, 0) + (M - 1) * B * K * tile_bytes, (B, M, p)
        assert ext == tiled(plan, B, H, W, T, T, O, O, p, 1)
        assert internal - ext == M * B * K * tile_bytes                        # the whole tile storage
    assert ws(None, 1, 2, H, W, T, T, O, O, 4, 0) == 0
    assert ws(plan, 1, 0, H, W, T, T, O, O, 4, 0) == 0 and b"members" in lib.mi_last_error()
    assert ws(plan, 1, 2, H, W, 36, T, O, O, 4, 0) == 0 and b"multiples of 8" in lib.mi_last_error()


# ------------------------------------------------------------------------------ 3. the restatement itself
def test_reference_blend_reduce_composes_the_two_restatements():
    rng = np.random.default_rng(11)
    H, W, T, O = 45, 59, 32, 8
    tiles = rng.standard_normal((3, 2, 6, 2, T, T)).astype(np.float32)
    mean, std, samples = ref.blend_reduce(tiles, H, W, (O, O))
    assert samples.shape == (2, 3, 2, H, W) and mean.shape == std.shape == (2, 2, H, W)
    assert all(a.dtype == np.float32 for a in (mean, std, samples))
    for m in range(3):
        assert np.array_equal(samples[:, m], tiled_reference.blend(tiles[m], H, W, (O, O)))
    want_mean, want_std = ensemble_reference.reduce(samples)
    assert np.array_equal(mean, want_mean) and np.array_equal(std, want_std)
    assert np.allclose(std, samples.astype(np.float64).std(axis=1, ddof=1), rtol=1e-6, atol=1e-7)
    one_mean, one_std, one = ref.blend_reduce(tiles[:1], H, W, (O, O))
    assert one_std is None and np.array_equal(one_mean, one[:, 0])             # one member: the mean is its blended image
    const = np.full((4, 1, 6, 1, T, T), np.float32(0.3))
    cm, cs, _ = ref.blend_reduce(const, H, W, (O, O))
    assert (cm == np.float32(0.3)).all() and (cs == 0).all()


# ------------------------------------------------------------------------------ 4. Python surface
def test_python_surface_without_a_gpu():
    assert midd_amd.TiledEnsembleResult._fields == ("mean", "std", "samples", "tiles", "origins_y", "origins_x", "seed")
    x = torch.zeros(1, 1, 40, 48)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="cddpm"):
        ddim.denoise_tiled_ensemble(x, inference_steps=2, members=2, tile=32, overlap=8)
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    kw = dict(inference_steps=2, tile=32, overlap=8, seed=1)
    with pytest.raises(ValueError, match="max_batch"):
        d.denoise_tiled_ensemble(x, max_batch=0, **kw)
    with pytest.raises(ValueError, match="sample_offset"):
        d.denoise_tiled_ensemble(x, sample_offset=-1, **kw)
    with pytest.raises(ValueError, match="member_offset"):
        d.denoise_tiled_ensemble(x, member_offset=-1, **kw)
    with pytest.raises(ValueError, match="members"):
        d.denoise_tiled_ensemble(x, members=0, **kw)
    with pytest.raises(ValueError, match=r"2\*\*32"):
        d.denoise_tiled_ensemble(x, members=2, member_offset=(1 << 32) - 1, **kw)
    with pytest.raises(ValueError, match="seed"):
        d.denoise_tiled_ensemble(x, inference_steps=2, tile=32, overlap=8, seed=-1)
    with pytest.raises(ValueError, match="step_noise"):
        d.denoise_tiled_ensemble(x, step_noise=torch.zeros(1), **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                 # valid arguments, CPU tensors: never a silent fall-back
        d.denoise_tiled_ensemble(x, members=2, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.denoise_tiled_ensemble(x, members=2, inference_steps=2, tile=32, overlap=8)      # seed drawn
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.tile_blend_reduce(torch.zeros(2, 1, 4, 1, 32, 32), 40, 48, 8)
    with pytest.raises(ValueError, match="6-dimensional"):
        midd_amd.tile_blend_reduce(torch.zeros(1, 4, 1, 32, 32), 40, 48, 8)
