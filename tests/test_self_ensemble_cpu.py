"""CPU-only checks of the geometric self-ensemble (include/midd.h: THE GEOMETRY, mi_dihedral_*, mi_denoise_self_ensemble): the numpy
restatement's own properties, the view-list resolver, every argument rule of the C ABI -- each reported before any device call,
and the earlier one when two are broken -- the workspace query, the Python and CLI argument rules, and the new kernels' ISA (no
scratch).  What the device computes is judged in test_gpu_self_ensemble.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetDiffusion, native
from tests import self_ensemble_reference as sref
from tests.isa_dump import isa_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_dihedral_views", "mi_dihedral_reduce", "mi_dihedral_quantiles", "mi_denoise_self_ensemble", "mi_self_ensemble_workspace_bytes"}
# non-null "device pointers", 1 MiB apart, for calls that must fail before anything reads them (every buffer below is < 1 MiB)
NOISY, MEAN, STD, SAMPLES, OUT = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000


def _codes(*v):
    return (C.c_int32 * len(v))(*v), len(v)


def _levels(*v):
    return (C.c_double * len(v))(*v), len(v)


# ------------------------------------------------------------------------------ 1. the restatement
def _asym(H, W, seed=0):
    return np.random.default_rng(seed).random((2, H, W), dtype=np.float32)


@pytest.mark.parametrize("H,W,codes", [(5, 7, sref.FLIPS), (6, 6, sref.D4), (7, 7, sref.D4)])
def test_unview_inverts_view(H, W, codes):
    x = _asym(H, W)
    for g in codes:
        v = sref.view(x, g)
        assert v.shape == ((2, W, H) if g & 4 else (2, H, W))
        assert np.array_equal(sref.unview(v, g), x), g
        assert np.array_equal(sref.view(sref.unview(x, g), g), x), g


def test_view_codes_are_the_named_symmetries():
    x = _asym(6, 6)
    assert np.array_equal(sref.view(x, 0), x)
    assert np.array_equal(sref.view(x, 1), x[..., :, ::-1]) and np.array_equal(sref.view(x, 2), x[..., ::-1, :])
    assert np.array_equal(sref.view(x, 3), np.rot90(x, 2, axes=(-2, -1)))
    assert np.array_equal(sref.view(x, 4), np.swapaxes(x, -1, -2))
    assert np.array_equal(sref.view(x, 5), np.rot90(x, -1, axes=(-2, -1)))          # clockwise quarter turn
    assert np.array_equal(sref.view(x, 6), np.rot90(x, 1, axes=(-2, -1)))           # counter-clockwise quarter turn
    assert np.array_equal(sref.view(x, 7), np.rot90(x, 2, axes=(-2, -1)).swapaxes(-1, -2))      # anti-transpose
    # the same on a non-square array, where a quarter turn changes the shape
    y = _asym(5, 7)
    assert np.array_equal(sref.view(y, 5), np.rot90(y, -1, axes=(-2, -1))) and np.array_equal(sref.view(y, 6), np.rot90(y, 1, axes=(-2, -1)))


def test_the_eight_views_of_an_asymmetric_image_differ():
    x = _asym(6, 6)
    vs = [sref.view(x, g) for g in sref.D4]
    for i in range(8):
        for j in range(i):
            assert not np.array_equal(vs[i], vs[j]), (i, j)


def test_reduce_and_quantiles_are_the_ensemble_arithmetic_of_the_aligned_members():
    from tests import ensemble_reference as eref
    from tests import quantile_reference as qref
    rng = np.random.default_rng(3)
    vo = rng.random((2, 8, 1, 6, 6), dtype=np.float32)
    mean, std, m = sref.reduce(vo, sref.D4)
    assert np.array_equal(m[1, 5, 0], np.rot90(vo[1, 5, 0], 1))               # unview of the clockwise turn is the counter-clockwise one
    want_mean, want_std = eref.reduce(m)
    assert np.array_equal(mean, want_mean) and np.array_equal(std, want_std)
    assert np.array_equal(sref.quantiles(vo, sref.D4, (0.0, 0.5, 1.0)), qref.quantiles(m, (0.0, 0.5, 1.0)))
    # the views of one image, turned back, are eight copies of it: mean = image, std = 0
    img = rng.random((1, 1, 6, 6), dtype=np.float32)
    mean, std, m = sref.reduce(sref.views(img, sref.D4), sref.D4)
    assert np.array_equal(mean, img) and not std.any() and all(np.array_equal(m[0, k], img[0]) for k in range(8))


# ------------------------------------------------------------------------------ 2. view_codes
def test_view_codes_resolves_the_spellings():
    assert midd_amd.view_codes(64, 64, "auto") == (0, 1, 2, 3, 4, 5, 6, 7) == midd_amd.view_codes(64, 64)
    assert midd_amd.view_codes(40, 104, "auto") == (0, 1, 2, 3)
    assert midd_amd.view_codes(64, 64, "flips") == (0, 1, 2, 3) == midd_amd.view_codes(40, 104, "flips")
    assert midd_amd.view_codes(64, 64, "d4") == (0, 1, 2, 3, 4, 5, 6, 7)
    assert midd_amd.view_codes(64, 64, [3, 6, 5, 0]) == (3, 6, 5, 0)              # the caller's order
    assert midd_amd.view_codes(40, 104, (2,)) == (2,)
    assert midd_amd.view_codes(64, 64, np.array([0, 7])) == (0, 7)


@pytest.mark.parametrize("H,W,views,word", [
    (64, 64, (0, 5, 5), "view code 5 is repeated"), (64, 64, (0, 8), "integer in [0, 7] (got 8)"), (64, 64, (-1,), "integer in [0, 7]"),
    (64, 64, (), "between 1 and 8 view codes (got 0)"), (64, 64, tuple(range(8)) + (0,), "between 1 and 8 view codes (got 9)"),
    (40, 104, (0, 4), "view code 4 transposes the image: codes 4 .. 7 need H == W (got 40x104"), (40, 104, "d4", "codes 4 .. 7 need H == W"),
    (64, 64, "rot", "'auto', 'flips', 'd4'"), (64, 64, 3, "sequence of view codes"), (64, 64, (1.0,), "integer in [0, 7]"),
    (64, 64, (True,), "integer in [0, 7]"), (0, 64, "auto", "H must be"),
])
def test_view_codes_refuses(H, W, views, word):
    with pytest.raises(ValueError) as exc:
        midd_amd.view_codes(H, W, views)
    assert word in str(exc.value)


# ------------------------------------------------------------------------------ 3. declarations and the C ABI's argument rules
def test_header_and_binding_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n: a for n, _, a in native.SYMBOLS}
    assert NEW <= declared and declared == set(bound)
    for name in NEW:
        assert getattr(native.lib(), name) is not None
    assert "THE GEOMETRY" in header and "g = 4*t + 2*fy + fx" in header and "numpy.rot90(x, -1)" in header
    # the self-ensemble is mi_denoise_ensemble with (views, n_views) for `members` and a `seeded` switch
    ens, own = bound["mi_denoise_ensemble"], bound["mi_denoise_self_ensemble"]
    assert own[:5] == ens[:5] and own[10:16] == ens[9:15] and own[17:] == ens[15:] and own[16] is C.c_int
    assert bound["mi_self_ensemble_workspace_bytes"] == bound["mi_ensemble_workspace_bytes"]


@pytest.fixture(scope="module")
def plan():
    """An unfinalized DDIM plan: every host-side rule can be checked on it, no GPU call can succeed."""
    lib = native.lib()
    c = UNetDiffusion(**SMALL).cfg
    cfg = native.UNetCfg()
    cfg.in_channels, cfg.model_channels, cfg.num_levels = c.in_channels, c.model_channels, len(c.channel_mult)
    for i, v in enumerate(c.channel_mult):
        cfg.channel_mult[i] = v
    cfg.num_res_blocks, cfg.num_attention_levels = c.num_res_blocks, len(c.attention_resolutions)
    for i, v in enumerate(c.attention_resolutions):
        cfg.attention_levels[i] = v
    cfg.time_emb_dim, cfg.variant, cfg.compute_mode = c.time_emb_dim, native.MI_VARIANT["ddim"], native.MI_COMPUTE["f16x3"]
    h = C.c_void_p()
    native.check(lib.mi_unet_plan_create(C.byref(cfg), C.byref(h)))
    yield h
    lib.mi_plan_destroy(h)


def _reports(rc, first, never=()):
    """The call failed with MI_EINVAL, its message holds every word of `first` and none of `never` (the other broken rule)."""
    msg = native.lib().mi_last_error().decode()
    assert rc == -1, msg
    for w in first:
        assert w in msg, msg
    for w in never:
        assert w not in msg, msg


def _self_ensemble(plan, null_plan=False, noisy=NOISY, mean=MEAN, std=STD, samples=None, B=2, H=32, W=32, views=(0, 1, 2, 3, 4, 5, 6, 7),
                   n_views=None, seeded=0, sample_offset=0, member_offset=0, pass_samples=16):
    arr = None if views is None else (C.c_int32 * max(1, len(views)))(*views)
    return native.lib().mi_denoise_self_ensemble(None if null_plan else plan, noisy, mean, std, samples, B, H, W, arr,
                                                 (0 if views is None else len(views)) if n_views is None else n_views, None, 0,
                                                 None, None, None, 50, seeded, 5, sample_offset, member_offset, pass_samples, 0, None, 0, None)


@pytest.mark.parametrize("kw,word", [
    (dict(null_plan=True), "null plan"),
    (dict(views=()), "n_views 0 outside [1, 8]"), (dict(views=(0,) * 9), "n_views 9 outside [1, 8]"), (dict(n_views=-1), "1 <= n_views <= 8"),
    (dict(views=None, n_views=4), "null argument: views"),
    (dict(views=(0, 8)), "views[1] = 8 outside [0, 7]"), (dict(views=(-1,)), "views[0] = -1 outside [0, 7]"),
    (dict(views=(0, 5, 3, 5)), "views[3] = 5 repeats views[1]"),
    (dict(H=40, W=104, views=(0, 1, 6)), "views[2] = 6 transposes a 40x104 image"), (dict(H=40, W=104), "view codes 4 .. 7 need H == W"),
    (dict(mean=None, std=None), "no output"),
    (dict(views=(3,)), "std_out needs at least two views"),
    (dict(pass_samples=0), "pass_samples >= 1"),
    (dict(mean=NOISY), "noisy and mean_out alias"), (dict(std=NOISY + 4), "noisy and std_out alias"),
    (dict(samples=NOISY), "noisy and samples_out alias"), (dict(std=MEAN), "mean_out and std_out alias"),
    (dict(samples=MEAN + 4), "mean_out and samples_out alias"), (dict(samples=STD + 8), "std_out and samples_out alias"),
    (dict(B=0), "B 0 outside [1, 65535]"), (dict(B=65536), "B 65536 outside [1, 65535]"),
    (dict(H=65536, W=65536), "4294967296"), (dict(H=0, W=0), "bad image shape"),
    (dict(sample_offset=-1), "sample_offset -1"), (dict(sample_offset=-1, seeded=1), "sample_offset -1"),
    (dict(member_offset=-1), "member_offset -1"), (dict(member_offset=(1 << 32) - 7, seeded=1), "member_offset + members <= 4294967296"),
])
def test_self_ensemble_rules_are_reported_before_any_gpu_work(plan, kw, word):
    _reports(_self_ensemble(plan, **kw), [word])


@pytest.mark.parametrize("kw,first,never", [
    (dict(null_plan=True, views=()), ["null plan"], ["n_views"]),
    (dict(views=None, n_views=9), ["n_views 9"], ["null"]),
    (dict(views=(8, 8)), ["outside [0, 7]"], ["repeats"]),
    (dict(views=(0, 0, 9)), ["repeats"], ["outside [0, 7]"]),                                                  # in list order
    (dict(views=(4, 4), H=40, W=104), ["repeats"], ["transposes"]),
    (dict(views=(0, 4), H=40, W=104, member_offset=-1), ["transposes"], ["member_offset"]),
    (dict(member_offset=-1, pass_samples=0), ["member_offset -1"], ["pass_samples"]),
    (dict(member_offset=(1 << 32) - 7, pass_samples=0), ["4294967296"], ["pass_samples"]),
    (dict(pass_samples=0, B=0), ["pass_samples >= 1"], ["B 0"]),
    (dict(B=0, sample_offset=-2), ["B 0 outside"], ["sample_offset"]),
    (dict(sample_offset=-2, H=0, W=0), ["sample_offset -2"], ["bad image shape"]),
    (dict(H=65536, W=65536, mean=None, std=None), ["4294967296"], ["no output"]),
    (dict(mean=None, std=None, views=(0,)), ["no output", "samples_out"], ["finalize"]),
    (dict(views=(0,), mean=NOISY), ["std_out needs at least two views"], ["alias"]),
    (dict(mean=NOISY, std=NOISY + 4), ["noisy and mean_out alias"], ["std_out alias"]),
    (dict(std=MEAN, samples=NOISY), ["noisy and samples_out alias"], ["std_out alias"]),
    (dict(std=MEAN, samples=MEAN + 4), ["mean_out and std_out alias"], ["samples_out alias"]),
])
def test_self_ensemble_reports_the_first_broken_rule(plan, kw, first, never):
    _reports(_self_ensemble(plan, **kw), first, never)


def test_self_ensemble_alias_message_and_state_check(plan):
    lib = native.lib()
    assert _self_ensemble(plan, mean=NOISY) == -1
    assert lib.mi_last_error().decode() == ("noisy and mean_out alias (overlap): noisy is read by every pass and the reduce writes "
                                            "mean_out, std_out and samples_out in one launch")
    assert _self_ensemble(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _self_ensemble(plan, noisy=None, samples=SAMPLES) == -2      # a null noisy is judged after the state
    assert _self_ensemble(plan, H=40, W=104, views=(0, 1, 2, 3)) == -2  # the shape-keeping views take a non-square image


def test_workspace_query_is_the_ensemble_layout_and_answers_before_finalize(plan):
    lib = native.lib()
    for B, G, H, W, p in [(2, 8, 32, 32, 16), (2, 8, 32, 32, 5), (1, 4, 40, 104, 16), (3, 1, 64, 64, 2), (4, 3, 32, 32, 64)]:
        want = lib.mi_ensemble_workspace_bytes(plan, B, G, H, W, p, 0)
        assert want > B * G * H * W * 4
        # the view outputs always live in the workspace: samples_external does not shrink it (include/midd.h)
        assert lib.mi_self_ensemble_workspace_bytes(plan, B, G, H, W, p, 0) == want
        assert lib.mi_self_ensemble_workspace_bytes(plan, B, G, H, W, p, 1) == want
        assert lib.mi_ensemble_workspace_bytes(plan, B, G, H, W, p, 1) == want - B * G * H * W * 4      # ... and are its last bytes
    for args, word in [((2, 0, 32, 32, 16, 0), "n_views 0"), ((2, 9, 32, 32, 16, 0), "n_views 9"), ((0, 8, 32, 32, 16, 0), "B 0"),
                       ((2, 8, 32, 32, 0, 0), "pass_samples"), ((2, 8, 33, 32, 16, 0), ""), ((2, 8, 65536, 65536, 16, 0), "4294967296")]:
        assert lib.mi_self_ensemble_workspace_bytes(plan, *args) == 0, args
        assert word in lib.mi_last_error().decode(), (args, lib.mi_last_error())
    assert lib.mi_self_ensemble_workspace_bytes(None, 2, 8, 32, 32, 16, 0) == 0


def _views_call(images=NOISY, B=2, Cc=1, H=32, W=32, views=(0, 1, 2, 3, 4, 5, 6, 7), v0=0, n=4, dst=OUT):
    arr = None if views is None else (C.c_int32 * max(1, len(views)))(*views)
    return native.lib().mi_dihedral_views(images, B, Cc, H, W, arr, 0 if views is None else len(views), v0, n, dst, None)


def _reduce_call(vo=SAMPLES, B=2, Cc=1, H=32, W=32, views=(0, 1, 2, 3, 4, 5, 6, 7), mean=MEAN, std=STD, samples=None):
    arr = None if views is None else (C.c_int32 * max(1, len(views)))(*views)
    return native.lib().mi_dihedral_reduce(vo, B, Cc, H, W, arr, 0 if views is None else len(views), mean, std, samples, None)


def _quantiles_call(vo=SAMPLES, B=2, Cc=1, H=32, W=32, views=(0, 1, 2, 3, 4, 5, 6, 7), q=None, out=OUT):
    arr = None if views is None else (C.c_int32 * max(1, len(views)))(*views)
    q = _levels(0.05, 0.5, 0.95) if q is None else q
    return native.lib().mi_dihedral_quantiles(vo, B, Cc, H, W, arr, 0 if views is None else len(views), q[0], q[1], out, None)


GEOMETRY = [(dict(views=()), "n_views 0 outside [1, 8]"), (dict(views=(0,) * 9), "n_views 9"), (dict(views=(0, 8)), "views[1] = 8 outside [0, 7]"),
            (dict(views=(2, 7, 2)), "views[2] = 2 repeats views[0]"), (dict(H=40, W=104), "view codes 4 .. 7 need H == W"),
            (dict(Cc=0), "C 0"), (dict(B=0), "B 0 outside"), (dict(B=65536), "65535"), (dict(H=65536, W=65536), "4294967296"),
            (dict(H=0), "bad image shape")]


@pytest.mark.parametrize("call", [_views_call, _reduce_call, _quantiles_call])
def test_standalone_calls_refuse_the_geometry_errors(call):
    for kw, word in GEOMETRY:
        _reports(call(**kw), [word])
    _reports(call(views=None), ["n_views 0"])


def test_standalone_calls_own_rules():
    lib = native.lib()
    for kw, word in [(dict(v0=-1), "views [-1"), (dict(n=-1), "outside the 2 * 8 virtual samples"), (dict(v0=13, n=4), "outside the 2 * 8"),
                     (dict(v0=17, n=0), "outside the 2 * 8"), (dict(B=65535, n=65536), "n <= 65535"), (dict(images=None), "null"), (dict(dst=None), "null")]:
        _reports(_views_call(**kw), [word])
    assert _views_call(n=0) == 0 and _views_call(v0=16, n=0) == 0 and _views_call(n=0, images=None, dst=None) == 0      # nothing to do: MI_OK
    for kw, word in [(dict(mean=None, std=None), "no output"), (dict(views=(6,)), "std_out needs at least two views"), (dict(vo=None), "null")]:
        _reports(_reduce_call(**kw), [word])
    q3 = _levels(0.05, 0.5, 0.95)
    for kw, word in [(dict(q=(q3[0], 0)), "1 <= nq <= 8"), (dict(q=(q3[0], 9)), "1 <= nq <= 8"), (dict(q=(None, 2)), "null"),
                     (dict(q=_levels(0.5, -0.1)), "q[1]"), (dict(q=_levels(float("nan"))), "q[0]"), (dict(vo=None), "null"), (dict(out=None), "null")]:
        _reports(_quantiles_call(**kw), [word])
    # the view list is judged before a call's own rules
    _reports(_views_call(views=(0, 0), v0=-1), ["repeats"], ["virtual samples"])
    _reports(_reduce_call(views=(0, 9), mean=None, std=None), ["outside [0, 7]"], ["no output"])
    _reports(_quantiles_call(H=40, W=104, q=(q3[0], 0)), ["transposes"], ["nq"])
    assert lib.mi_last_error()


# ------------------------------------------------------------------------------ 4. Python surface and CLI
def test_python_surface_without_a_gpu():
    assert midd_amd.SelfEnsembleResult._fields == ("mean", "std", "samples", "views", "seed")
    assert midd_amd.SelfEnsembleQuantileResult._fields == midd_amd.SelfEnsembleResult._fields + ("quantiles", "levels")
    x = torch.zeros(1, 1, 32, 32)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    cddpm = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="the DDIM variant takes seed=None"):
        ddim.denoise_self_ensemble(x, inference_steps=2, seed=1)
    for d in (ddim, cddpm):
        with pytest.raises(ValueError, match="repeated"):
            d.denoise_self_ensemble(x, inference_steps=2, views=(1, 1))
        with pytest.raises(ValueError, match="need H == W"):
            d.denoise_self_ensemble(torch.zeros(1, 1, 32, 40), inference_steps=2, views="d4")
        with pytest.raises(ValueError, match="quantile level"):
            d.denoise_self_ensemble(x, inference_steps=2, quantiles=(1.5,))
        with pytest.raises(ValueError, match="max_batch"):
            d.denoise_self_ensemble(x, inference_steps=2, max_batch=0)
        with pytest.raises(ValueError, match="member_offset"):
            d.denoise_self_ensemble(x, inference_steps=2, member_offset=(1 << 32) - 3)
        # valid arguments, CPU tensors: never a silent fall-back
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            d.denoise_self_ensemble(x, inference_steps=2, quantiles=(0.5,))
    with pytest.raises(ValueError, match="seed must be"):
        cddpm.denoise_self_ensemble(x, inference_steps=2, seed=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.dihedral_views(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.dihedral_reduce(torch.zeros(1, 8, 1, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.dihedral_quantiles(torch.zeros(1, 4, 1, 32, 40), "flips", (0.5,))
    with pytest.raises(ValueError, match="holds 3 views per image, the view list 8"):
        midd_amd.dihedral_reduce(torch.zeros(1, 3, 1, 32, 32))
    with pytest.raises(ValueError, match="levels"):
        midd_amd.dihedral_quantiles(torch.zeros(1, 8, 1, 32, 32))
    with pytest.raises(ValueError, match="5-dimensional"):
        midd_amd.dihedral_reduce(torch.zeros(8, 1, 32, 32))


def test_cli_refuses_what_is_out_of_scope(capsys):
    import inspect
    from midd_amd import cli
    assert inspect.signature(cli.denoise_image_diffusion).parameters["self_ensemble"].default is None
    base = ["--image", "nowhere.png"]
    for argv, word in [(["--self-ensemble", "--samples", "4"], "--self-ensemble cannot be combined with --samples"),
                       (["--self-ensemble", "--tile", "64"], "--self-ensemble cannot be combined with --tile"),
                       (["--self-ensemble", "d4", "--variant", "ddim", "--samples", "4"], "--self-ensemble cannot be combined with --samples"),
                       (["--self-ensemble", "rot"], "invalid choice"),
                       (["--self-ensemble", "--quantiles", "0.5"], "come together"),
                       (["--self-ensemble", "--quantiles", "1.5", "--quantiles-out", "q.npy"], "[0, 1]")]:
        with pytest.raises(SystemExit):
            cli.main(argv + base)
        assert word in capsys.readouterr().err, argv
    for kw, word in [(dict(samples=4), "--samples"), (dict(tile=64), "--tile"), (dict(step_noise=torch.zeros(1)), "step_noise")]:
        with pytest.raises(ValueError, match=word):
            cli.denoise_image_diffusion(None, "nowhere.png", variant="ddim", self_ensemble="auto", **kw)
    with pytest.raises(ValueError, match="auto, flips or d4"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="ddim", self_ensemble="rot")


# ------------------------------------------------------------------------------ 5. static: the kernels' ISA
@pytest.fixture(scope="module")
def pointwise_isa():
    return isa_dump("dihedral.hip")


def test_no_dihedral_kernel_touches_scratch_and_only_the_transposing_forms_use_lds(pointwise_isa):
    """The members of a thread's pixels (8 views x 4 pixels) and the sort keys live in registers: every instantiation has a private
    segment of 0 bytes and no scratch instruction.  The forms for lists without a transposing view allocate no LDS and have no
    barrier; the transposing ones hold four padded 32 x 33 patches, the fill one."""
    seen = {}
    for m in re.finditer(r"\n(_ZN4midd\d+(dihedral_\w+?_kernel)(ILb([01])E)?\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", pointwise_isa, re.S):
        name, kind, tr, body = m.group(1), m.group(2), m.group(4), m.group(5)
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert "scratch_" not in body, name
        lds = int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1))
        seen[(kind, tr)] = lds
        if tr == "0":
            assert lds == 0 and "s_barrier" not in body and "ds_read" not in body and "ds_write" not in body, name
        else:
            assert "s_barrier" in body and "ds_read" in body and "ds_write" in body, name
        if kind == "dihedral_quantiles_kernel":
            assert "v_min_u32" in body and "v_max_u32" in body and not re.search(r"v_fma\w*_f64", body), name
    patch = 32 * 33 * 4
    assert seen == {("dihedral_views_kernel", None): patch, ("dihedral_reduce_kernel", "0"): 0, ("dihedral_reduce_kernel", "1"): 4 * patch,
                    ("dihedral_quantiles_kernel", "0"): 0, ("dihedral_quantiles_kernel", "1"): 4 * patch}
