"""CPU-only checks of the per-pixel quantile maps of an ensemble (include/midd.h: mi_ensemble_quantiles, mi_tile_blend_quantiles):
the numpy restatement against numpy's own quantile, the argument rules of the C ABI (every refusal comes before any device call),
the Python and CLI argument rules, and the kernels' ISA: no instantiation may touch scratch.  What the device computes is judged in
test_gpu_quantiles.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetDiffusion, native
from tests import quantile_reference as qref
from tests.isa_dump import isa_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_ensemble_quantiles", "mi_tile_blend_quantiles"}
SAMPLES, OUT = 0x100000, 0x900000           # non-null "device pointers" for calls that must fail before anything reads them
SWEEP_K = (1, 2, 3, 5, 8, 9, 16, 17, 33, 64)
SWEEP_Q = (0.0, 1.0, 0.5, 1.0 / 3.0, 0.05, 0.95, 0.25, 0.999)


def _ulps(a, b):
    """Distance in fp32 units in the last place between two non-negative float32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _members(K, n=4096, seed=0):
    """Uniform [0, 1) members [1, K, n] with ties planted: a third of the pixels repeat one of their members."""
    rng = np.random.default_rng(seed + K)
    x = rng.random((1, K, n), dtype=np.float32)
    if K >= 2:
        x[0, 1, ::3] = x[0, 0, ::3]
        x[0, K - 1, 1::7] = x[0, K // 2, 1::7]
    return x


# ------------------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("K", SWEEP_K)
def test_restatement_is_numpys_linear_quantile_within_one_ulp(K):
    """numpy interpolates as a + (b - a) * g too, but picks a and b and rounds the steps differently; both are correctly rounded
    double operations on fp32 inputs in [0, 1), so the fp32 results differ by the last bit at most."""
    x = _members(K)
    got = qref.quantiles(x, SWEEP_Q)
    assert got.shape == (1, len(SWEEP_Q), x.shape[2]) and got.dtype == np.float32
    want = np.quantile(x.astype(np.float64), SWEEP_Q, axis=1).astype(np.float32)      # [nq, 1, n]
    worst = int(_ulps(got[0], want[:, 0]).max())
    print(f"K = {K}: worst distance to numpy.quantile over {len(SWEEP_Q)} levels = {worst} ulp")
    assert worst <= 1
    assert np.array_equal(got[0, 0], x[0].min(axis=0)) and np.array_equal(got[0, 1], x[0].max(axis=0))      # q = 0, q = 1
    assert (np.diff(qref.quantiles(x, sorted(SWEEP_Q)), axis=1) >= 0).all()            # non-decreasing in q
    if K % 2 == 1:
        assert np.array_equal(got[0, 2], np.median(x[0], axis=0))                      # bit for bit


def test_restatement_integer_positions_return_a_member():
    x = _members(5)
    got = qref.quantiles(x, (0.25, 0.75))                                              # pos = 1, 3
    s = np.sort(x, axis=1)
    assert np.array_equal(got[0, 0], s[0, 1]) and np.array_equal(got[0, 1], s[0, 3])
    one = _members(1)
    assert np.array_equal(qref.quantiles(one, (0.0, 0.3, 1.0)), np.repeat(one, 3, axis=1))      # one member: every quantile is it


def test_restatement_nan_signed_zero_and_infinities():
    x = _members(5, n=8)
    x[0, 2, 3] = np.nan
    x[0, :, 4] = (-0.0, 0.0, -0.0, 1.0, -1.0)
    x[0, :, 5] = (np.inf, 0.25, -np.inf, 0.5, 0.75)
    x[0, :, 6] = (1e-45, -1e-45, 0.0, 1e-40, -1e-40)                                     # denormals
    got = qref.quantiles(x, (0.0, 0.3, 0.5, 1.0))
    assert (got[0, :, 3].view(np.uint32) == 0x7FC00000).all()                           # a NaN member: the canonical NaN at every level
    assert not np.isnan(got[0, :, :3]).any()
    order = qref.sort_members(x)
    assert order[0, :, 4].view(np.uint32).tolist() == [0xBF800000, 0x80000000, 0x80000000, 0, 0x3F800000]      # -1 < -0 = -0 < +0 < 1
    assert order[0, :, 5].tolist() == [-np.inf, 0.25, 0.5, 0.75, np.inf]
    assert order[0, :, 6].tolist() == sorted(x[0, :, 6].tolist())
    assert got[0, 2, 5] == 0.5 and got[0, 2, 6] == 0.0
    # what the formula makes of an infinite end: 0 * inf at an integer position, the canonical NaN; +inf inside an interval
    assert got[0, 0, 5:6].view(np.uint32)[0] == 0x7FC00000 and got[0, 3, 5:6].view(np.uint32)[0] == 0x7FC00000
    assert qref.quantiles(x, (0.9,))[0, 0, 5] == np.inf
    assert np.array_equal(qref.unkeys(qref.keys(x)).view(np.uint32), x.view(np.uint32))


# ------------------------------------------------------------------------------ 2. declarations and the C ABI's argument rules
def test_header_and_binding_declare_the_two_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n: a for n, _, a in native.SYMBOLS}
    assert NEW <= declared and declared == set(bound)
    for name in NEW:
        assert getattr(native.lib(), name) is not None
    assert "k = bits ^ (sign ? 0xFFFFFFFF : 0x80000000)" in header and "members <= 64" in header
    # the quantile form of a reduce call: the outputs are replaced by (q, nq, out)
    assert bound["mi_tile_blend_quantiles"][:10] == bound["mi_tile_blend_reduce"][:10]


def _levels(*v):
    return (C.c_double * len(v))(*v), len(v)


def test_ensemble_quantiles_rules():
    lib = native.lib()
    q3 = _levels(0.05, 0.5, 0.95)

    def call(samples=SAMPLES, B=2, members=5, chw=64, q=q3, out=OUT):
        return lib.mi_ensemble_quantiles(samples, B, members, chw, q[0], q[1], out, None)

    cases = [(dict(members=0), "members >= 1"), (dict(B=0), "65535"), (dict(B=65536), "65535"), (dict(chw=0), "chw"),
             (dict(chw=1 << 32), "4294967296"), (dict(samples=None), "null"), (dict(out=None), "null"),
             (dict(members=65), "members <= 64"), (dict(members=1 << 20), "members <= 64"),
             (dict(q=(q3[0], 0)), "1 <= nq <= 8"), (dict(q=(q3[0], 9)), "1 <= nq <= 8"), (dict(q=(q3[0], -1)), "1 <= nq <= 8"),
             (dict(q=(None, 3)), "null"),
             (dict(q=_levels(0.5, -0.1)), "q[1]"), (dict(q=_levels(1.0000001)), "q[0]"), (dict(q=_levels(0.0, 1.0, float("nan"))), "q[2]"),
             (dict(q=_levels(float("inf"))), "[0, 1]"), (dict(q=_levels(-0.1)), "[0, 1]")]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.mi_last_error().decode(), (kw, lib.mi_last_error())


def test_tile_blend_quantiles_rules():
    lib = native.lib()
    q3 = _levels(0.05, 0.5, 0.95)

    def call(tiles=SAMPLES, B=2, members=3, Cc=1, H=45, W=59, th=32, tw=32, oy=8, ox=8, q=q3, out=OUT):
        return lib.mi_tile_blend_quantiles(tiles, B, members, Cc, H, W, th, tw, oy, ox, q[0], q[1], out, None)

    cases = [(dict(th=48), "tile <= image"), (dict(ox=17), "tile / 2"), (dict(oy=-1), "overlap"), (dict(Cc=0), "C 0"),
             (dict(H=65536, W=65536), "4294967296"), (dict(B=0), "B 0"), (dict(B=65536), "65535"),
             (dict(B=1 << 30, H=64, W=64, oy=0, ox=0), "B * tiles"),
             (dict(B=1 << 15, H=64, W=64, oy=0, ox=0, members=1 << 15), "B * members * tiles"),
             (dict(members=0), "members >= 1"), (dict(tiles=None), "null"), (dict(out=None), "null"),
             (dict(members=65), "members <= 64"),
             (dict(q=(q3[0], 0)), "1 <= nq <= 8"), (dict(q=(q3[0], 9)), "1 <= nq <= 8"), (dict(q=(None, 2)), "null"),
             (dict(q=_levels(-0.1)), "q[0]"), (dict(q=_levels(0.5, 1.0000001)), "q[1]"), (dict(q=_levels(float("nan"))), "q[0]")]
    for kw, word in cases:
        assert call(**kw) == -1, kw
        assert word in lib.mi_last_error().decode(), (kw, lib.mi_last_error())


# ------------------------------------------------------------------------------ 3. Python surface
def test_python_surface_without_a_gpu():
    assert midd_amd.EnsembleResult._fields == ("mean", "std", "samples", "seed")      # untouched: existing callers unpack them
    assert midd_amd.TiledEnsembleResult._fields == ("mean", "std", "samples", "tiles", "origins_y", "origins_x", "seed")
    assert midd_amd.EnsembleQuantileResult._fields == midd_amd.EnsembleResult._fields + ("quantiles", "levels")
    assert midd_amd.TiledEnsembleQuantileResult._fields == midd_amd.TiledEnsembleResult._fields + ("quantiles", "levels")
    x = torch.zeros(1, 1, 32, 32)
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    tiled = dict(inference_steps=2, tile=32, overlap=8, seed=1)
    for bad in ((), (0.5,) * 9, (0.5, -0.1), (1.0000001,), (float("nan"),), ("0.5",), (True,), object()):
        with pytest.raises(ValueError, match="quantile level"):
            d.denoise_ensemble(x, inference_steps=2, members=4, seed=1, quantiles=bad)
        with pytest.raises(ValueError, match="quantile level"):
            d.denoise_tiled_ensemble(x, members=2, quantiles=bad, **tiled)
        with pytest.raises(ValueError, match="quantile level"):
            midd_amd.ensemble_quantiles(torch.zeros(1, 4, 8), bad)
        with pytest.raises(ValueError, match="quantile level"):
            midd_amd.tile_blend_quantiles(torch.zeros(2, 1, 1, 1, 32, 32), 32, 32, 8, q=bad)
    with pytest.raises(ValueError, match="members <= 64"):
        d.denoise_ensemble(x, inference_steps=2, members=65, seed=1, quantiles=(0.5,))
    with pytest.raises(ValueError, match="members <= 64"):
        d.denoise_tiled_ensemble(x, members=65, quantiles=(0.5,), **tiled)
    with pytest.raises(ValueError, match="members <= 64"):
        midd_amd.ensemble_quantiles(torch.zeros(1, 65, 8), (0.5,))
    with pytest.raises(ValueError, match="members <= 64"):
        midd_amd.tile_blend_quantiles(torch.zeros(65, 1, 1, 1, 32, 32), 32, 32, 8, q=(0.5,))
    with pytest.raises(ValueError, match="members"):
        midd_amd.ensemble_quantiles(torch.zeros(4, 8), (0.5,))
    with pytest.raises(ValueError, match="6-dimensional"):
        midd_amd.tile_blend_quantiles(torch.zeros(1, 4, 1, 32, 32), 40, 48, 8, q=(0.5,))
    with pytest.raises(ValueError, match="levels"):
        midd_amd.tile_blend_quantiles(torch.zeros(2, 1, 1, 1, 32, 32), 32, 32, 8)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="deterministic sampler has no ensemble"):
        ddim.denoise_ensemble(x, inference_steps=2, members=4, seed=1, quantiles=(0.5,))
    # valid arguments, CPU tensors: never a silent fall-back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.denoise_ensemble(x, inference_steps=2, members=4, seed=1, quantiles=(0.05, 0.5, 0.95))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.denoise_tiled_ensemble(x, members=2, quantiles=(0.5,), **tiled)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.ensemble_quantiles(torch.zeros(1, 4, 8), (0.5,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.tile_blend_quantiles(torch.zeros(2, 1, 1, 1, 32, 32), 32, 32, 8, q=0.5)


def test_cli_refuses_quantiles_without_what_they_need(capsys):
    import inspect
    from midd_amd import cli
    sig = inspect.signature(cli.denoise_image_diffusion).parameters
    assert sig["quantiles"].default is None and sig["quantiles_out"].default is None
    base = ["--image", "nowhere.png"]
    for argv, word in [(["--quantiles", "0.5", "--quantiles-out", "q.npy"], "--samples"),                      # no --samples
                       (["--samples", "4", "--quantiles", "0.5"], "come together"),                               # no --quantiles-out
                       (["--samples", "4", "--quantiles-out", "q.npy"], "come together"),
                       (["--samples", "65", "--quantiles", "0.5", "--quantiles-out", "q.npy"], "K <= 64"),
                       (["--samples", "4", "--quantiles", "0.5,1.5", "--quantiles-out", "q.npy"], "[0, 1]"),
                       (["--samples", "4", "--quantiles", "-0.1", "--quantiles-out", "q.npy"], "[0, 1]"),
                       (["--samples", "4", "--quantiles", "0.1,x", "--quantiles-out", "q.npy"], "[0, 1]"),
                       (["--samples", "4", "--quantiles", ",".join(["0.5"] * 9), "--quantiles-out", "q.npy"], "up to 8"),
                       (["--samples", "4", "--variant", "ddim", "--quantiles", "0.5", "--quantiles-out", "q.npy"], "cddpm"),
                       (["--tile", "64", "--samples", "4", "--quantiles", "0.5", "--quantiles-out", "q.npy"], "--tile")]:
        with pytest.raises(SystemExit):
            cli.main(argv + base)
        assert word in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="come together"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", samples=4, quantiles=(0.5,))
    with pytest.raises(ValueError, match="K <= 64"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", samples=65, quantiles=(0.5,), quantiles_out="q.npy")
    with pytest.raises(ValueError, match="K <= 64"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", quantiles=(0.5,), quantiles_out="q.npy")
    with pytest.raises(ValueError, match="quantile level"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", samples=4, quantiles=(1.5,), quantiles_out="q.npy")


# ------------------------------------------------------------------------------ 4. static: the kernels' ISA
@pytest.fixture(scope="module")
def pointwise_isa():
    return isa_dump("ensemble.hip") + isa_dump("tiles.hip")


def _metadata(text):
    """kernel symbol -> {field: int} from the code object's metadata notes."""
    notes = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - ", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_no_quantile_kernel_touches_scratch(pointwise_isa):
    """The sort lives in registers only if no register array is indexed by a run-time value: every instantiation -- KP in
    {2, 4, 8, 16, 32, 64}, V in {1, 4}, and the six blend forms -- has a private segment of 0 bytes, no spilled VGPR and no scratch
    instruction, and the interpolation of the plain kernel (which has no division) carries no fused multiply-add."""
    meta = _metadata(pointwise_isa)
    seen = set()
    for name, fields in meta.items():
        m = re.search(r"(ensemble_quantiles_kernel|tile_blend_quantiles_kernel)ILi(\d+)E(?:Li(\d+)E)?", name)
        if not m:
            continue
        seen.add((m.group(1), int(m.group(2)), int(m.group(3) or 0)))
        assert fields["private_segment_fixed_size"] == 0, (name, fields)
        assert fields["vgpr_spill_count"] == 0, (name, fields)
        start = pointwise_isa.index("\n" + name + ":")
        body = pointwise_isa[start:pointwise_isa.index(".end_amdhsa_kernel", start)]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert "scratch_" not in body, name
        assert "v_min_u32" in body and "v_max_u32" in body, name
        if m.group(1) == "ensemble_quantiles_kernel":
            assert not re.search(r"v_fma\w*_f64", body), name
    want = {("ensemble_quantiles_kernel", kp, v) for kp in (2, 4, 8, 16, 32, 64) for v in (1, 4)}
    want |= {("tile_blend_quantiles_kernel", kp, 0) for kp in (2, 4, 8, 16, 32, 64)}
    assert seen == want
