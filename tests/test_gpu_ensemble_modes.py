"""GPU: the principal modes of an ensemble's spread (include/midd.h: THE ENSEMBLE MODES, mi_ensemble_gram, mi_ensemble_project;
midd_amd.ensemble_modes, DiffusionDenoiser.ensemble_modes).

The arithmetic is fixed, the order of the double sums included, so the device is compared bit for bit with the numpy restatement
(tests/ensemble_modes_reference.py): the Gram matrix, the invalid counts and -- given the same weights -- the modes, at member
counts on both sides of the small / tiled dispatch (K <= 8: one launch; above: mean pre-pass and block pairs, full and partial
blocks), at sizes around the chunk of 4096 elements, on the 16-byte path and the element path, with planted NaN and Inf members.
The host step between the two launches is the package's own on both sides, so equal Gram bits give equal weights."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native
from midd_amd.ensemble import gram_eigen
from midd_amd.weights import make_state_dict, synthetic_xray
from tests import ensemble_modes_reference as ref

pytestmark = pytest.mark.gpu

CHUNK = ref.CHUNK
SMALL = dict(model_channels=16, time_emb_dim=64)
SEED = 0x5EEDC0DE12345678
# (shape [B, K, C, H, W], modes): the issue's four shapes, then chw = chunk - 1, chunk, chunk + 1, 2 chunk + 3 in one launch (K = 8) and
# in block pairs with a partial block (K = 9), then two chunks and a partial one on the 16-byte path
SHAPES = [((1, 2, 1, 5, 7), 1), ((2, 3, 2, 9, 11), 2), ((1, 8, 1, 33, 31), 3), ((1, 64, 1, 16, 17), 8)]
SHAPES += [((1, K, 1, 1, n), M) for K, M in ((8, 7), (9, 4)) for n in (CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3)]
SHAPES += [((2, 8, 1, 1, 2 * CHUNK + 4), 2), ((1, 17, 1, 1, 2 * CHUNK + 4), 5)]

_cases, _models = {}, {}


def _case(shape, M):
    """(members, the restatement's Gram, its weights and modes): computed once, shared, never written.  Where the image is long
    enough a NaN and a +inf member are planted (in the first and the last image)."""
    key = (shape, M)
    if key not in _cases:
        B, K = shape[:2]
        chw = int(np.prod(shape[2:]))
        x = ref.philox_case(B, K, chw, seed=500 + K, nan_at=(0, K - 1, 9) if chw > 30 else None, inf_at=(B - 1, 0, chw - 3) if chw > 30 else None)
        g = ref.gram(x)
        mu, v, w = gram_eigen(g.gram, M)
        _cases[key] = (x.reshape(shape), g, w, ref.project(x, w))
    return _cases[key]


def _same(got, g: ref.Gram, modes, shape):
    chw = int(np.prod(shape[2:]))
    assert np.array_equal(got.gram.numpy().view(np.uint64), g.gram.view(np.uint64)), (got.gram, g.gram)
    assert np.array_equal(got.valid.numpy(), chw - g.invalid)
    assert got.modes.shape == (shape[0], modes.shape[1]) + shape[2:]
    assert np.array_equal(got.modes.cpu().numpy().reshape(modes.shape).view(np.uint32), modes.view(np.uint32))


def _project(x, w):
    """mi_ensemble_project on device members with the given host weights [B, M, K]."""
    B, K = x.shape[:2]
    chw = x[0, 0].numel()
    wd = torch.from_numpy(np.ascontiguousarray(w)).cuda()
    out = torch.empty((B, w.shape[1], chw), dtype=torch.float32, device="cuda")
    native.check(native.lib().mi_ensemble_project(x.data_ptr(), B, K, chw, wd.data_ptr(), w.shape[1], out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


# ------------------------------------------------------------------------------ 1. the kernels against the restatement
@pytest.mark.parametrize("shape,M", SHAPES)
def test_device_equals_the_restatement_bit_for_bit(shape, M):
    x, g, w, modes = _case(shape, M)
    xd = torch.from_numpy(x).cuda()
    got = midd_amd.ensemble_modes(xd, M)
    _same(got, g, modes, shape)
    assert np.array_equal(_project(xd, w).view(np.uint32), modes.view(np.uint32))      # the projection alone, given the weights
    chw = int(np.prod(shape[2:]))
    if chw > 30:      # the planted NaN and +inf: counted, left out, NaN in every mode
        assert g.invalid.sum() == 2 and g.invalid[0] >= 1
        assert np.array_equal(modes.view(np.uint32)[0, :, 9], np.full(M, 0x7FC00000, np.uint32))
        assert np.array_equal(modes.view(np.uint32)[-1, :, chw - 3], np.full(M, 0x7FC00000, np.uint32))
    K = shape[1]
    assert got.variance.shape == (shape[0], M) and got.coefficients.shape == (shape[0], K, M) and got.total_variance.shape == (shape[0],)
    assert bool((got.variance[:, :-1] >= got.variance[:, 1:]).all()) and bool((got.explained.sum(dim=1) <= 1.0 + 1e-12).all())


@pytest.mark.parametrize("shape,M", [((2, 8, 1, 1, 2 * CHUNK + 4), 2), ((1, 17, 1, 1, 2 * CHUNK + 4), 5)])
def test_the_alignment_path_does_not_show(shape, M):
    """The same members 16-byte aligned and in a view offset by one float, which takes the element-load path: the same bits."""
    x, g, w, modes = _case(shape, M)
    buf = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    for off in (0, 1):
        xs = buf[off:off + x.size].view(shape)
        xs.copy_(torch.from_numpy(x))
        assert xs.data_ptr() % 16 == 4 * off and xs.is_contiguous()
        _same(midd_amd.ensemble_modes(xs, M), g, modes, shape)
        assert np.array_equal(_project(xs, w).view(np.uint32), modes.view(np.uint32))


def test_the_same_call_twice_gives_the_same_bits_and_an_unbatched_input_its_image():
    shape, M = (1, 17, 1, 1, 2 * CHUNK + 4), 5
    x, g, w, modes = _case(shape, M)
    xd = torch.from_numpy(x).cuda()
    a, b = midd_amd.ensemble_modes(xd, M), midd_amd.ensemble_modes(xd, M)
    bits = lambda t: t.view({torch.float32: torch.int32, torch.float64: torch.int64}.get(t.dtype, t.dtype))      # (the planted NaN: compare bits)
    for f in midd_amd.EnsembleModes._fields:
        assert torch.equal(bits(getattr(a, f)), bits(getattr(b, f))), f
    one = midd_amd.ensemble_modes(xd[0], M)
    assert one.modes.shape == (M,) + shape[2:] and one.gram.shape == (17, 17) and one.valid.dim() == 0 and one.coefficients.shape == (17, M)
    assert torch.equal(one.gram, a.gram[0]) and torch.equal(bits(one.modes), bits(a.modes[0]))


def test_planted_structure_on_the_device():
    x, p1, p2 = ref.planted_case()
    got = midd_amd.ensemble_modes(torch.from_numpy(x).cuda(), 3)
    corr = lambda a, b: abs(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    m = got.modes.cpu().numpy()[0, :, 0]
    print(f"corr {corr(m[0], p1):.6f} {corr(m[1], p2):.6f}; explained {got.explained[0].tolist()}")
    assert corr(m[0], p1) > 0.999 and corr(m[1], p2) > 0.999
    assert abs(float(got.explained[0, 0] / got.explained[0, 1]) / 4.0 - 1.0) < 0.05
    assert int(got.valid[0]) == 32 * 32 and abs(float(got.variance[0, 0]) / (1024 * 0.04 ** 2) - 1.0) < 0.01
    # the modes of all 15 directions would add up to the variance; three of them already hold all but the noise, whose variance is
    # 1e-6 a pixel on average and chi-square with 15 degrees of freedom: below 4e-6 at every one of 1024 pixels, 1e-5 with room
    std = midd_amd.ensemble_reduce(torch.from_numpy(x).cuda())[1].cpu().numpy()[0, 0].astype(np.float64)
    assert np.abs((m.astype(np.float64) ** 2).sum(axis=0) - std ** 2).max() < 1e-5


# ------------------------------------------------------------------------------ 2. end to end
def _denoiser():
    if "cddpm" not in _models:
        sd = make_state_dict(UNetConfig(variant="cddpm", **SMALL), seed=42)
        m = UNetDiffusion(variant="cddpm", **SMALL)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        _models["cddpm"] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models["cddpm"]


def _status_word(model) -> int:
    """mi_status of the resident ensemble workspace, read directly."""
    assert model.check_status and model._ensemble_ws is not None
    wptr, _ = UNetDiffusion._aligned_ptr(model._ensemble_ws[1])
    flags = C.c_int(-1)
    native.check(native.lib().mi_status(wptr, torch.cuda.current_stream().cuda_stream, C.byref(flags)))
    return flags.value


def _equal_modes(a, b):
    for f in midd_amd.EnsembleModes._fields:
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def _noisy(B, H, W):
    clean = torch.from_numpy(synthetic_xray(B, H, W, seed=31)).cuda()
    return (clean + 0.1 * torch.from_numpy(synthetic_xray(B, H, W, seed=32)).cuda() - 0.05).clamp(0, 1)


def test_denoiser_ensemble_modes_is_the_composition():
    d = _denoiser()
    noisy = _noisy(2, 32, 32)
    kw = dict(inference_steps=2, members=4, seed=SEED, sample_offset=1, member_offset=2)
    res, pm = d.ensemble_modes(noisy, modes=3, **kw)
    assert _status_word(d.model) == 0
    want = d.denoise_ensemble(noisy, return_samples=True, **kw)
    assert torch.equal(res.samples, want.samples) and torch.equal(res.mean, want.mean) and torch.equal(res.std, want.std) and res.seed == SEED
    _equal_modes(pm, midd_amd.ensemble_modes(want.samples, 3))
    assert pm.modes.shape == (2, 3, 1, 32, 32) and int(pm.valid.sum()) == 2 * 32 * 32 and bool((pm.variance > 0).all())
    host = ref.gram(want.samples.cpu().numpy())
    assert np.array_equal(pm.gram.numpy().view(np.uint64), host.gram.view(np.uint64))
    # all K - 1 = 3 modes: their squares are the std map's square, to the fp32 roundings of both
    total = (pm.modes.double() ** 2).sum(dim=1)
    assert bool(((total - res.std.double() ** 2).abs() <= 4 * 2.0 ** -23 * res.std.double() ** 2).all())


def test_denoiser_ensemble_modes_tiled_is_the_composition():
    d = _denoiser()
    noisy = _noisy(1, 40, 24)
    kw = dict(inference_steps=2, members=3, seed=SEED, tile=16, overlap=4)
    res, pm = d.ensemble_modes(noisy, modes=2, **kw)
    assert _status_word(d.model) == 0
    want = d.denoise_tiled_ensemble(noisy, return_samples=True, **kw)
    assert torch.equal(res.samples, want.samples) and torch.equal(res.mean, want.mean) and res.origins_y == want.origins_y
    _equal_modes(pm, midd_amd.ensemble_modes(want.samples, 2))
    assert pm.modes.shape == (1, 2, 1, 40, 24) and int(pm.valid[0]) == 40 * 24


# ------------------------------------------------------------------------------ 3. the CLI
def test_cli_modes_with_samples(tmp_path, capsys):
    """--modes / --modes-out / --modes-json beside --samples K: the file and the JSON are ensemble_modes of the run's members."""
    from PIL import Image
    from midd_amd import cli
    noisy = synthetic_xray(1, 72, 88, seed=10)[0, 0].clip(0, 1)
    png = tmp_path / "in.png"
    Image.fromarray((noisy * 255).astype(np.uint8), mode="L").save(png)
    ckpt = str(tmp_path / "cddpm.pth")                                         # the CLI builds the reference's default topology
    sd = make_state_dict(UNetConfig(variant="cddpm"), seed=42)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "noise_steps": 50}, ckpt)
    out_npy, out_json = tmp_path / "modes.npy", tmp_path / "modes.json"
    cli.main(["--image", str(png), "--variant", "cddpm", "--checkpoint", ckpt, "--inference-steps", "2", "--seed", "7", "--out", str(tmp_path / "out.png"),
              "--samples", "3", "--img-size", "64", "--modes", "2", "--modes-out", str(out_npy), "--modes-json", str(out_json)])
    out = capsys.readouterr().out
    got = json.loads(out_json.read_text())
    modes = np.load(out_npy)
    assert "Principal modes of 3 members" in out and "Modes saved" in out and "Mode figures saved" in out
    assert modes.shape == (2, 1, 64, 64) and modes.dtype == np.float32 and np.isfinite(modes).all()
    assert got["members"] == 3 and got["modes"] == 2 and (got["height"], got["width"]) == (64, 64) and got["seed"] == 7 and got["valid"] == 64 * 64
    assert len(got["variance"]) == 2 and got["variance"][0] >= got["variance"][1] >= 0.0 and len(got["coefficients"]) == 3
    assert abs(sum(got["explained"]) - 1.0) < 1e-9                             # K - 1 = 2 modes hold everything
    assert abs((modes.astype(np.float64) ** 2).sum() - got["total_variance"]) <= 1e-5 * got["total_variance"]
