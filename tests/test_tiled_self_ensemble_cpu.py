"""CPU-only checks of the tiled self-ensemble (include/midd.h: TILED SELF-ENSEMBLE): the geometry for H != W, "a view's tiles are
the tiles of the viewed image", the host-side rules of the new calls in their documented order (on an unfinalized plan: nothing
reaches a GPU), the workspace query, the Python and CLI argument resolution, and the kernels' resource numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import UNetDiffusion, native
from tests import self_ensemble_reference as sref
from tests import tiled_reference as tref
from tests import tiled_self_ensemble_reference as tsref
from tests.isa_dump import isa_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_tile_blend_unview_reduce", "mi_tile_blend_unview_quantiles", "mi_denoise_tiled_self_ensemble", "mi_tiled_self_ensemble_workspace_bytes"}
# non-null "device pointers", 1 MiB apart, for calls that must fail before anything reads them (every buffer below is < 1 MiB)
NOISY, MEAN, STD, SAMPLES, TILES = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
IMG_BYTES = 2 * 90 * 70 * 4


def test_the_new_symbols_are_declared_and_mirrored():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in native.SYMBOLS}
    assert NEW <= declared and NEW <= bound
    for name in NEW:
        assert getattr(native.lib(), name) is not None
    for name in ("TiledSelfEnsembleResult", "TiledSelfEnsembleQuantileResult", "view_codes_tiled", "tile_blend_unview_reduce",
                 "tile_blend_unview_quantiles"):
        assert hasattr(midd_amd, name), name
    assert hasattr(midd_amd.DiffusionDenoiser, "denoise_tiled_self_ensemble") and hasattr(UNetDiffusion, "run_tiled_self_ensemble")


# ------------------------------------------------------------------------------ 1. the geometry for H != W
@pytest.mark.parametrize("shape", [(5, 3), (41, 27)])
def test_view_and_unview_are_inverse_and_match_the_header_formulas(shape):
    H, W = shape
    x = np.arange(H * W, dtype=np.float32).reshape(H, W)
    for g in range(8):
        v = tsref.view(x, g)
        assert v.shape == ((W, H) if g & 4 else (H, W)), g
        assert np.array_equal(v, tsref.view_entry(x, g)), g
        assert np.array_equal(tsref.unview(v, g), x), g
        assert np.array_equal(tsref.unview_entry(v, g, H, W), x), g
        y = np.arange(v.size, dtype=np.float32).reshape(v.shape)                 # view(unview(.)) is the identity of the view's frame
        assert np.array_equal(tsref.view(tsref.unview(y, g), g), y), g


def test_the_general_form_agrees_with_the_square_form():
    x = np.random.default_rng(3).random((2, 7, 7)).astype(np.float32)
    for g in range(8):
        assert np.array_equal(np.stack([tsref.view_entry(p, g) for p in x]), sref.view(x, g)), g
        assert np.array_equal(np.stack([tsref.unview_entry(p, g, 7, 7) for p in x]), sref.unview(x, g)), g


def _origins(L, T, O):
    n = C.c_int()
    native.check(native.lib().mi_tile_geometry(L, T, O, C.byref(n), None, 0))
    o = (C.c_int * n.value)()
    native.check(native.lib().mi_tile_geometry(L, T, O, C.byref(n), o, n.value))
    return list(o)


def test_tiles_of_the_view_are_not_the_view_of_the_tiles():
    """The origin formula rounds down: the mirror of the origins of L = 41, T = 16, O = 4 is another set, that of L = 40 the same."""
    assert _origins(41, 16, 4) == tref.origins(41, 16, 4) == [0, 8, 16, 25]
    assert sorted(41 - 16 - o for o in _origins(41, 16, 4)) == [0, 9, 17, 25]
    o40 = _origins(40, 16, 4)
    assert sorted(40 - 16 - o for o in o40) == o40 == tref.origins(40, 16, 4)
    for L, same in ((41, False), (40, True)):
        x = np.random.default_rng(L).random((1, 1, L, L)).astype(np.float32)
        of_view = tsref.view_tiles(x, (16, 16), (4, 4), [1])[0]                 # the tiles of the mirrored image
        view_of = tref.extract(x, (16, 16), (4, 4))[..., ::-1]                   # the mirrored tiles of the image ...
        nx = len(tref.origins(L, 16, 4))
        view_of = view_of.reshape(1, nx, nx, 1, 16, 16)[:, :, ::-1].reshape(of_view.shape)      # ... in mirrored column order
        assert np.array_equal(of_view, view_of) == same, L


def test_reference_members_are_the_composition_of_the_existing_restatements():
    rng = np.random.default_rng(11)
    H, W, T, O = 41, 27, (16, 16), (4, 4)
    x = rng.random((2, 1, H, W)).astype(np.float32)
    tiles = tsref.view_tiles(x, T, O, tsref.D4)
    assert tiles.shape == (8, 2, 4 * 2, 1, 16, 16)
    m = tsref.members(tiles, H, W, O, tsref.D4)                                  # blending the un-denoised tiles gives the image back
    assert m.shape == (2, 8, 1, H, W) and all(np.array_equal(m[:, k], x) for k in range(8))
    mean, std, _ = tsref.reduce(tiles, H, W, O, tsref.D4)
    assert np.array_equal(mean, x) and not std.any()


# ------------------------------------------------------------------------------ 2. view_codes_tiled
def test_view_codes_tiled_resolution_and_errors():
    f = midd_amd.view_codes_tiled
    assert f(2500, 2048, 256, 32) == f(40, 24, 16, 4, "auto") == f(40, 24, 16, 4, "d4") == tuple(range(8))      # square tile: d4 whatever H, W
    assert f(40, 56, (16, 24), (4, 8)) == f(40, 56, (16, 16), (4, 8)) == f(64, 64, (16, 24), 4) == (0, 1, 2, 3)      # else the flips
    assert f(40, 24, 16, 4, "flips") == (0, 1, 2, 3) and f(40, 24, 16, 4, [6, 0, 3]) == (6, 0, 3)
    assert f(40, 56, (16, 24), (4, 8), [3, 1]) == (3, 1)
    assert midd_amd.view_codes(40, 24) == (0, 1, 2, 3)                           # view_codes is what it was
    for kw, word in [(dict(views="rot"), "'auto', 'flips', 'd4'"), (dict(views=5), "sequence"), (dict(views=[]), "between 1 and 8"),
                     (dict(views=list(range(8)) + [0]), "between 1 and 8"), (dict(views=[0, 8]), r"\[0, 7\]"), (dict(views=[0, True]), r"\[0, 7\]"),
                     (dict(views=[2, 2]), "repeated"), (dict(tile=(16, 24), views="d4"), "square tile and overlap"),
                     (dict(overlap=(4, 8), views=[0, 5]), "square tile and overlap"), (dict(tile=0), "tile"), (dict(overlap=-1), "overlap"),
                     (dict(H=0), "H")]:
        args = dict(H=40, W=24, tile=16, overlap=4, views="auto")
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            f(**args)


def test_python_calls_refuse_before_any_gpu_work():
    den = midd_amd.DiffusionDenoiser(UNetDiffusion(variant="ddim", **SMALL), noise_steps=50)
    x = torch.zeros(1, 1, 40, 24)
    with pytest.raises(ValueError, match="dpmpp2m"):
        den.denoise_tiled_self_ensemble(x, 2, tile=16, overlap=4, update="dpmpp2m")
    with pytest.raises(ValueError, match="seed=None"):
        den.denoise_tiled_self_ensemble(x, 2, tile=16, overlap=4, seed=3)
    with pytest.raises(ValueError, match="square tile and overlap"):
        den.denoise_tiled_self_ensemble(x, 2, tile=(16, 8), overlap=4, views="d4")
    with pytest.raises(ValueError, match="quantile"):
        den.denoise_tiled_self_ensemble(x, 2, tile=16, overlap=4, quantiles=(1.5,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        den.denoise_tiled_self_ensemble(x, 2, tile=16, overlap=4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.tile_blend_unview_reduce(torch.zeros(8, 1, 6, 1, 16, 16), 40, 24, 4)
    with pytest.raises(ValueError, match="holds 3 views, the view list 8"):
        midd_amd.tile_blend_unview_reduce(torch.zeros(3, 1, 6, 1, 16, 16), 40, 24, 4)
    with pytest.raises(ValueError, match="levels"):
        midd_amd.tile_blend_unview_quantiles(torch.zeros(8, 1, 6, 1, 16, 16), 40, 24, 4)


# ------------------------------------------------------------------------------ 3. the native rules, on an unfinalized plan
@pytest.fixture(scope="module")
def plan():
    lib = native.lib()
    c = UNetDiffusion(variant="cddpm", **SMALL).cfg
    cfg = native.UNetCfg()
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


TAB = np.linspace(1e-4, 0.02, 50, dtype=np.float32)
AH = np.cumprod(1.0 - TAB.astype(np.float64)).astype(np.float32)
FP = C.POINTER(C.c_float)


def _call(plan, null_plan=False, noisy=NOISY, mean=MEAN, std=STD, samples=None, tiles=None, B=2, H=90, W=70, th=32, tw=32, oy=8, ox=8,
          views=(0, 3), n_views=None, sample_offset=0, member_offset=0, pass_samples=16, rule=None, t_list=(40, 20, 0)):
    v = None if views is None else (C.c_int32 * max(1, len(views)))(*views)
    t = (C.c_int32 * len(t_list))(*t_list)
    r = None if rule is None else C.byref(native.UpdateRule(*rule))
    tab = TAB.ctypes.data_as(FP)
    return native.lib().mi_denoise_tiled_self_ensemble(
        None if null_plan else plan, noisy, mean, std, samples, tiles, B, H, W, th, tw, oy, ox, v, len(views or ()) if n_views is None else n_views,
        t, len(t_list), tab, tab, AH.ctypes.data_as(FP), 50, 1, 5, sample_offset, member_offset, pass_samples, 0, r, None, 0, None)


def _reports(rc, first, never=()):
    msg = native.lib().mi_last_error().decode()
    assert rc == -1, msg
    for w in first:
        assert w in msg, msg
    for w in never:
        assert w not in msg, msg


@pytest.mark.parametrize("kw,first,never", [
    # the rule's own cases come first, MI_UPDATE_DPMPP2M by name
    (dict(rule=(2, 0.0, 1), null_plan=True), ["MI_UPDATE_DPMPP2M", "mi_denoise_tiled_self_ensemble", "limit"], ["null plan"]),
    (dict(rule=(1, 1.5, 1), null_plan=True), ["eta"], ["null plan"]),
    (dict(rule=(1, 0.0, 1), t_list=(20, 40, 0), null_plan=True), ["decreasing"], ["null plan"]),
    (dict(rule=(7, 0.0, 1), null_plan=True), ["unknown update rule 7"], ["null plan"]),
    # then the plan and the view list, as check_views without the H == W clause
    (dict(null_plan=True, views=()), ["null plan"], ["n_views"]),
    (dict(views=(), th=36), ["n_views 0 outside [1, 8]", "limit"], ["multiples"]),
    (dict(views=tuple(range(8)), n_views=9), ["n_views 9 outside [1, 8]"], []),
    (dict(views=None, n_views=2, th=36), ["null argument: views"], ["multiples"]),
    (dict(views=(0, 8), th=36), ["views[1] = 8 outside [0, 7]", "limit"], ["multiples"]),
    (dict(views=(3, 3), th=36), ["views[1] = 3 repeats views[0]"], ["multiples"]),
    (dict(views=(3, 3, 5), tw=64), ["repeats"], ["transposes"]),
    # then the transposing rule: a square tile and overlap, NOT a square image
    (dict(views=(0, 5), tw=64, th=36), ["views[1] = 5 transposes", "th == tw and oy == ox", "H == W is not needed"], ["multiples"]),
    (dict(views=(6,), ox=4, pass_samples=0), ["views[0] = 6 transposes", "overlap 8x4", "limit"], ["pass_samples"]),
    # then everything mi_denoise_tiled_ensemble refuses, in its order, with members = n_views
    (dict(th=36, pass_samples=0), ["multiples of 8"], ["pass_samples"]),
    (dict(th=96, tw=96, views=(0, 5)), ["tile height 96 exceeds the image height 90"], ["width"]),
    (dict(oy=17, ox=17, pass_samples=0), ["overlap 17 of tile height 32"], ["pass_samples"]),
    (dict(pass_samples=0, sample_offset=-2), ["pass_samples >= 1"], ["sample_offset"]),
    (dict(sample_offset=-2, B=0), ["sample_offset -2"], ["B 0"]),
    (dict(B=0, member_offset=-1), ["B 0 must be positive"], ["member_offset"]),
    (dict(member_offset=-1, mean=None, std=None), ["member_offset -1"], ["no output"]),
    (dict(member_offset=(1 << 32) - 1, mean=None, std=None), ["member_offset + members <= 4294967296"], ["no output"]),
    (dict(B=1 << 28, H=64, W=64, oy=0, ox=0, views=tuple(range(8)), mean=None, std=None), ["B * members * tiles"], ["no output"]),
    (dict(B=65536, H=64, W=64, oy=0, ox=0, mean=None, std=None), ["B 65536 outside [1, 65535]"], ["no output"]),
    (dict(mean=None, std=None, views=(0,)), ["no output", "tiles_out"], ["std_out needs"]),
    (dict(views=(4,), mean=NOISY), ["std_out needs at least two views"], ["alias"]),
    (dict(mean=NOISY, std=NOISY + 4), ["noisy and mean_out alias"], ["std_out alias"]),
    (dict(samples=SAMPLES, tiles=SAMPLES + 2 * IMG_BYTES - 4), ["samples_out and tiles_out alias", "every round"], ["finalize"]),
])
def test_the_call_reports_the_first_broken_rule(plan, kw, first, never):
    _reports(_call(plan, **kw), first, never)


def test_the_state_check_comes_after_every_argument_rule(plan):
    lib = native.lib()
    assert _call(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _call(plan, views=tuple(range(8)), H=41, W=27, th=16, tw=16, oy=4, ox=4) == -2      # all 8 views of a non-square image: accepted
    assert _call(plan, rule=(1, 0.5, 1)) == -2                                                  # DDIM, any eta
    assert _call(plan, noisy=None, mean=None, std=None, tiles=TILES) == -2                      # a null noisy is judged after the state
    # mi_dihedral_views and mi_denoise_self_ensemble keep their H == W rule
    v = (C.c_int32 * 2)(0, 5)
    assert lib.mi_dihedral_views(NOISY, 2, 1, 32, 40, v, 2, 0, 4, MEAN, None) == -1 and b"need H == W" in lib.mi_last_error()


def test_the_stand_alone_calls_refuse_in_their_order():
    lib = native.lib()
    q_ok = (C.c_double * 2)(0.1, 0.9)

    def red(tiles=TILES, B=2, Cc=1, H=40, W=56, th=16, tw=24, oy=4, ox=8, views=(0, 3), n=None, mean=MEAN, std=STD, samples=None):
        v = None if views is None else (C.c_int32 * max(1, len(views)))(*views)
        return lib.mi_tile_blend_unview_reduce(tiles, B, Cc, H, W, th, tw, oy, ox, v, len(views or ()) if n is None else n, mean, std, samples, None)

    def qnt(tiles=TILES, views=(0, 3), q=q_ok, nq=2, out=MEAN, tw=24, ox=8):
        v = (C.c_int32 * len(views))(*views)
        return lib.mi_tile_blend_unview_quantiles(tiles, 2, 1, 40, 56, 16, tw, 4, ox, v, len(views), q, nq, out, None)

    for kw, words in [(dict(Cc=0, views=()), ["C 0 must be positive"]), (dict(th=48, views=()), ["tile height 48 exceeds"]),
                      (dict(oy=9, views=()), ["overlap 9 of tile height 16"]), (dict(views=()), ["n_views 0 outside [1, 8]"]),
                      (dict(views=None, n=2), ["null argument: views"]), (dict(views=(0, 9)), ["outside [0, 7]"]), (dict(views=(1, 1)), ["repeats"]),
                      (dict(views=(0, 4)), ["views[1] = 4 transposes", "16x24", "th == tw and oy == ox"]),       # the non-square tile refuses a transposing code
                      (dict(views=(0, 4), tw=16, B=0), ["B 0 must be positive"]),
                      (dict(tw=16, ox=8, views=(7,)), ["views[0] = 7 transposes", "overlap 4x8"]),
                      (dict(B=65536, H=16, W=24, oy=0, ox=0), ["B 65536 outside [1, 65535]"]),
                      (dict(mean=None, std=None), ["no output"]), (dict(views=(2,)), ["std_out needs at least two views"]),
                      (dict(tiles=None), ["null argument"])]:
        rc = red(**kw)
        msg = lib.mi_last_error().decode()
        assert rc == -1 and all(w in msg for w in words), (kw, msg)
    bad = (C.c_double * 2)(0.1, 1.5)
    for kw, word in [(dict(views=(0, 5)), "transposes"), (dict(q=bad), "outside [0, 1]"), (dict(nq=9), "nq 9"), (dict(out=None), "null argument")]:
        assert qnt(**kw) == -1 and word in lib.mi_last_error().decode(), kw


def test_workspace_query_is_its_documented_sum_and_works_before_finalize(plan):
    lib = native.lib()
    B, H, W, T, O, P = 2, 90, 70, 32, 8, 5
    K = len(tref.origins(H, T, O)) * len(tref.origins(W, T, O))
    base = lib.mi_tiled_workspace_bytes(plan, B, H, W, T, T, O, O, P, 1)
    assert base > 0
    copy = (B * 1 * H * W * 4 + 255) // 256 * 256
    for G in (1, 4, 8):
        assert lib.mi_tiled_self_ensemble_workspace_bytes(plan, B, G, H, W, T, T, O, O, P, 1) == base + copy
        assert lib.mi_tiled_self_ensemble_workspace_bytes(plan, B, G, H, W, T, T, O, O, P, 0) == base + copy + G * B * K * T * T * 4
    for args, word in [((None, B, 4, H, W, T, T, O, O, P, 0), "null plan"), ((plan, B, 0, H, W, T, T, O, O, P, 0), "n_views 0"),
                       ((plan, B, 9, H, W, T, T, O, O, P, 0), "n_views 9"), ((plan, B, 4, H, W, 36, T, O, O, P, 0), "multiples of 8"),
                       ((plan, B, 4, H, W, T, T, O, O, 0, 0), "pass_samples"), ((plan, 65536, 4, 32, 32, T, T, 0, 0, P, 0), "65535")]:
        assert lib.mi_tiled_self_ensemble_workspace_bytes(*args) == 0 and word in lib.mi_last_error().decode(), args


# ------------------------------------------------------------------------------ 4. the CLI
def test_cli_resolves_the_tiled_ensembles(capsys, tmp_path):
    import inspect
    from PIL import Image
    from midd_amd import cli
    sig = inspect.signature(cli.denoise_image_diffusion).parameters
    assert sig["views"].default is None and sig["members"].default is None
    base = ["--image", "nowhere.png"]
    for argv, word in [(["--views"], "need --tile"), (["--members", "4"], "need --tile"),
                       (["--tile", "64", "--views", "--members", "4"], "cannot be combined"),
                       (["--tile", "64", "--views", "rot"], "invalid choice"),
                       (["--tile", "64", "--views", "--update", "dpmpp2m"], "--update dpmpp2m cannot be combined with --views"),
                       (["--tile", "64", "--members", "0"], "--members needs K >= 1"),
                       (["--tile", "64", "--members", "4", "--variant", "ddim"], "use --views"),
                       (["--tile", "64", "--members", "4", "--update", "ddim", "--eta", "0.5"], "reference's update"),
                       (["--tile", "64", "--members", "1", "--std-out", "s.npy"], "--members K with K >= 2"),
                       (["--tile", "64", "--members", "65", "--quantiles", "0.5", "--quantiles-out", "q.npy"], "K <= 64"),
                       (["--tile", "64", "--views", "--quantiles", "0.5"], "come together"),
                       (["--tile", "64", "--std-out", "s.npy"], "--std-out needs --samples")]:
        with pytest.raises(SystemExit):
            cli.main(argv + base)
        assert word in capsys.readouterr().err, argv
    for kw, word in [(dict(views="auto"), "need --tile"), (dict(tile=64, views="auto", members=4), "cannot be combined"),
                     (dict(tile=64, views="rot"), "auto, flips or d4"), (dict(tile=64, views="d4", update="dpmpp2m"), "--views"),
                     (dict(tile=64, members=4, variant="ddim"), "--members needs the stochastic"),
                     (dict(tile=64, members=1, std_out="s.npy"), "K >= 2")]:
        args = dict(variant="cddpm")
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            cli.denoise_image_diffusion(None, "nowhere.png", **args)
    # accepted argument sets get as far as the image: --views with --std-out, quantiles, --update ddim, --bit-depth 16 and --window
    png = tmp_path / "small.png"
    Image.fromarray(np.zeros((40, 100), np.uint8), mode="L").save(png)
    for kw in (dict(views="auto", std_out="s.npy", variant="ddim"), dict(views="flips", quantiles=(0.5,), quantiles_out="q.npy", update="ddim", variant="ddim"),
               dict(views="d4", update="ddim", eta=0.5, bit_depth=16), dict(members=4, std_out="s.npy", quantiles=(0.1, 0.9), quantiles_out="q.npy")):
        with pytest.raises(ValueError, match="shorter than the tile"):
            cli.denoise_image_diffusion(None, str(png), device_type="cpu", tile=64, overlap=16, **{"variant": "cddpm", **kw})


# ------------------------------------------------------------------------------ 5. static: the kernels' resource numbers
def test_every_instantiation_is_free_of_scratch_and_spills_and_only_the_transposing_forms_use_lds():
    """The members of a thread's pixels (8 views x 4 pixels), the blend's accumulators and the sort keys live in registers: every
    instantiation has a private segment of 0 bytes and spills nothing.  The forms for lists without a transposing view allocate
    no LDS; the transposing ones hold one padded 32 x 33 patch per transposing view (at most four), the view kernel one."""
    isa = isa_dump("tiled_views.hip")
    patch = 32 * 33 * 4
    seen = {}
    for m in re.finditer(r"\n(_ZN4midd\d+(\w+?_kernel)(?:ILi(\d)E?)?(?:ILb|Lb)?([01])?E?\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", isa, re.S):
        name, kind, kp, tr, body = m.groups()
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        seen[(kind, kp, tr)] = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
    assert seen == {("plane_view_kernel", None, None): patch,
                    ("tile_blend_unview_reduce_kernel", None, "1"): 4 * patch, ("tile_blend_unview_reduce_kernel", None, "0"): 0,
                    ("tile_blend_unview_quantiles_kernel", "2", "1"): 2 * patch, ("tile_blend_unview_quantiles_kernel", "2", "0"): 0,
                    ("tile_blend_unview_quantiles_kernel", "4", "1"): 4 * patch, ("tile_blend_unview_quantiles_kernel", "4", "0"): 0,
                    ("tile_blend_unview_quantiles_kernel", "8", "1"): 4 * patch, ("tile_blend_unview_quantiles_kernel", "8", "0"): 0}, seen
    meta = re.findall(r"\.name:\s+(_ZN4midd\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                      r"(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)", isa)
    assert len(meta) == 9, [m[0] for m in meta]
    for name, private, sgpr_spills, vgpr_spills in meta:
        assert (int(private), int(sgpr_spills), int(vgpr_spills)) == (0, 0, 0), name
