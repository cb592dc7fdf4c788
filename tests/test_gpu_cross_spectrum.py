"""GPU: the Welch cross-spectrum (include/midd.h: THE CROSS SPECTRUM, mi_cross_spectrum; midd_amd.cross_spectrum,
DiffusionDenoiser.spectral_fidelity / ensemble_frc, cli --fidelity-out).

The arithmetic is fixed -- the detrend sums of both fields, the packed radix-2 transform, the separation in double, the chunked
accumulation, the radial sums -- so the device is compared bit for bit with the numpy restatement
(tests/cross_spectrum_reference.py): every output, doubles viewed as uint64, on the NPS suite's shapes.  The float64 gate of the
header section (numpy.fft, the bound derived from Higham's Theorem 24.2, relative to the COMBINED energy) is applied to the device
output directly, and to known answers.

Measured on an MI355X (test_device_against_float64_fft2, the largest of the four quantities): 6.1e-8, 7.2e-8 and 7.8e-8 for R = 32, 64,
128 (y = x / 2 in test_known_answers_under_the_gate: 7.3e-8, 8.7e-8, 9.5e-8); the bounds are 8.3e-6, 9.9e-6 and 1.15e-5."""
import json

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion
from midd_amd.weights import make_state_dict, synthetic_xray
from tests import cross_spectrum_reference as xref
from tests import nps_reference as ref

pytestmark = pytest.mark.gpu

SMALL = dict(model_channels=16, time_emb_dim=64)
SEED = 0x5EEDC0DE12345678
SHAPES = [(32, 16, 32, 32), (32, 16, 70, 83), (32, 5, 40, 45), (64, 32, 100, 131), (128, 64, 128, 200)]      # (R, S, H, W): the NPS suite's
BKC = [(1, 1, 1), (2, 3, 1), (1, 2, 2)]
PLANES = ("sxx", "syy", "sxy_re", "sxy_im")
RADIALS = ("radial_xx", "radial_yy", "radial_xy_re", "radial_xy_im")
_fields, _models = {}, {}


def _field(B, K, C, H, W):
    """(x, y paired [B, K, ..], y single [B, C, ..]) as numpy: seeded noise on ramps, y partly x; shared and never written."""
    key = (B, K, C, H, W)
    if key not in _fields:
        x = ref.philox_field((B, K, C, H, W), seed=H * W + K, ramp=0.3)
        n5 = ref.philox_field((B, K, C, H, W), seed=H * W + 55, ramp=0.1)
        n4 = ref.philox_field((B, C, H, W), seed=H * W + 77, ramp=0.25)
        _fields[key] = (x, (np.float32(0.6) * x + np.float32(0.4) * n5).astype(np.float32),
                        (np.float32(0.6) * x[:, 0] + np.float32(0.4) * n4).astype(np.float32))
    return _fields[key]


def _dev(a):
    return torch.from_numpy(a).cuda()


def _stack(got, names):
    return np.stack([getattr(got, n).numpy() for n in names])


def _same(got, want: xref.Xs):
    B, C = want.rois_used.shape
    for names, w in ((PLANES, want.planes), (RADIALS, want.radial)):
        g = _stack(got, names).reshape(w.shape)
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (names, np.abs(g - w).max())
    assert np.array_equal(got.radial_count.numpy(), want.radial_count)
    assert np.array_equal(got.rois_used.numpy().reshape(B, C), want.rois_used)
    assert np.array_equal(got.rois_skipped.numpy().reshape(B, C), want.rois_skipped)


def _as5(y):
    return y[:, None] if y.ndim == 4 else y


def _run(x, y, R, S, detrend="plane", window="hann", exclude_axes=False):
    """The device call and the restatement on the same numpy inputs (y [B, K, ..] or [B, C, ..], broadcast)."""
    got = midd_amd.cross_spectrum(_dev(x), _dev(y), R, S, detrend, window, exclude_axes, return_planes=True)
    want = xref.cross_spectrum(_as5(x), _as5(y), R, S, detrend, None if window is None else ref.hann(R), exclude_axes)
    return got, want


def _equal(a, b, fields=PLANES + RADIALS + ("radial_count", "freqs", "rois_used", "rois_skipped")):
    for f in fields:
        assert torch.equal(getattr(a, f).view(torch.int64), getattr(b, f).view(torch.int64)), f
    assert (a.roi, a.step) == (b.roi, b.step)


# ------------------------------------------------------------------------------ 1. the kernels against the restatement
@pytest.mark.parametrize("B,K,C", BKC)
@pytest.mark.parametrize("R,S,H,W", SHAPES)
def test_device_equals_the_restatement_bit_for_bit(R, S, H, W, B, K, C):
    """Every detrend x window on / off x y paired / broadcast x exclude_axes on / off: four planes, four radial arrays, the counts."""
    x, y5, y4 = _field(B, K, C, H, W)
    ny, nx = (H - R) // S + 1, (W - R) // S + 1
    for detrend in ("none", "mean", "plane"):
        for window in (None, "hann"):
            for y in (y5, y4):
                for ex in (False, True):
                    got, want = _run(x, y, R, S, detrend, window, ex)
                    assert got.sxy_im.shape == (B, C, R, R) and got.radial_xy_re.shape == (B, C, R // 2 + 1) and (got.roi, got.step) == (R, S)
                    assert int(got.rois_used.sum()) == B * C * K * ny * nx and int(got.rois_skipped.sum()) == 0
                    _same(got, want)
                    assert bool(torch.isnan(got.radial_xx[..., 0]).all()) == ex and not bool(torch.isnan(got.radial_xx[..., 1:]).any())
    assert got.freqs.tolist() == [r / R for r in range(R // 2 + 1)]
    # x with one realisation beside K draws of y, and the planes left on the device unless asked for
    swapped, want = _run(y4, x, R, S)
    _same(swapped, want)
    lean = midd_amd.cross_spectrum(_dev(y4), _dev(x), R, S)
    assert lean.sxx is None and lean.sxy_im is None
    _equal(lean, swapped, RADIALS + ("radial_count", "rois_used", "rois_skipped"))


@pytest.mark.parametrize("K,H,W,rois", [(3, 48, 48, 12), (4, 48, 48, 16), (1, 32, 288, 17), (3, 70, 83, 36), (2, 32, 288, 34)])
def test_roi_counts_around_the_chunk(K, H, W, rois):
    """R = 32, S = 16: below a chunk of 16 ROIs, exactly one, one more, and two chunks with a partial third (36; 34 with a member
    boundary inside a chunk)."""
    x, y5, y4 = _field(1, K, 1, H, W)
    for y in (y5, y4):
        got, want = _run(x, y, 32, 16)
        assert int(got.rois_used[0, 0]) == rois == int(want.rois_used[0, 0])
        _same(got, want)


# ------------------------------------------------------------------------------ 2. alignment
def _offset(x: torch.Tensor) -> torch.Tensor:
    """The same values one element off 16-byte alignment."""
    buf = torch.empty(x.numel() + 1, dtype=x.dtype, device=x.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[1:].view(x.shape)
    out.copy_(x)
    return out


@pytest.mark.parametrize("R,S,H,W", [(32, 16, 64, 80), (64, 32, 100, 132)])
def test_alignment_changes_no_bit(R, S, H, W):
    """W a multiple of 4 and the base aligned: every row quad is a 16-byte load.  One element off: none is.  Judged per field."""
    x, y5, _ = _field(2, 2, 1, H, W)
    xd, yd = _dev(x), _dev(y5)
    assert xd.data_ptr() % 16 == 0 and yd.data_ptr() % 16 == 0
    base = midd_amd.cross_spectrum(xd, yd, R, S, return_planes=True)
    _same(base, xref.cross_spectrum(x, y5, R, S, "plane", ref.hann(R)))
    for a, b in ((_offset(xd), yd), (xd, _offset(yd)), (_offset(xd), _offset(yd))):
        assert (a.data_ptr() % 16, b.data_ptr() % 16) != (0, 0)
        _equal(midd_amd.cross_spectrum(a, b, R, S, return_planes=True), base)


# ------------------------------------------------------------------------------ 3. independence
def test_groups_are_independent_and_the_call_repeats():
    R, S, H, W = 32, 16, 70, 83
    x, y5, y4 = _field(2, 3, 2, H, W)
    xd, yd, y4d = _dev(x), _dev(y5), _dev(y4)
    full = midd_amd.cross_spectrum(xd, yd, R, S, return_planes=True)
    _equal(midd_amd.cross_spectrum(xd, yd, R, S, return_planes=True), full)
    for bi in range(2):
        for c in range(2):
            one = midd_amd.cross_spectrum(xd[bi:bi + 1, :, c:c + 1], yd[bi:bi + 1, :, c:c + 1], R, S, return_planes=True)
            for f in PLANES + RADIALS:
                assert torch.equal(getattr(one, f)[0, 0].view(torch.int64), getattr(full, f)[bi, c].view(torch.int64)), f
            assert int(one.rois_used[0, 0]) == int(full.rois_used[bi, c]) == 36
    # the accepted shapes: [B, C, H, W] is K = 1, [H, W] drops the group axes
    four = midd_amd.cross_spectrum(xd[:, 0], y4d, R, S, return_planes=True)
    five = midd_amd.cross_spectrum(xd[:, :1], y4d[:, None], R, S, return_planes=True)
    _equal(four, five)
    assert four.sxx.shape == (2, 2, R, R)
    flat = midd_amd.cross_spectrum(xd[1, 0, 1], y4d[1, 1], R, S, return_planes=True)
    assert flat.sxy_re.shape == (R, R) and flat.radial_xy_re.shape == (R // 2 + 1,) and flat.rois_used.shape == ()
    assert torch.equal(flat.sxy_re.view(torch.int64), four.sxy_re[1, 1].view(torch.int64))
    assert flat.frc().shape == (R // 2 + 1,) and flat.resolution().shape == () and 0.0 < float(flat.resolution()) <= 0.5


# ------------------------------------------------------------------------------ 4. non-finite data
@pytest.mark.parametrize("bad_x,bad_y", [(((20, 40), np.nan), None), (None, ((0, 0), np.inf)), (((33, 17), np.nan), ((40, 20), -np.inf)),
                                          (((69, 82), np.nan), None)])
def test_a_non_finite_pixel_skips_exactly_the_rois_that_cover_it(bad_x, bad_y):
    """70 x 83, R 32, S 16: 12 ROIs per member.  The pixels sit in member 1 of 2, in x only, in y only, and one of each in the same
    ROIs (counted once); (69, 82) lies in no ROI."""
    R, S, H, W = 32, 16, 70, 83
    x, y5, _ = _field(1, 2, 1, H, W)
    x, y = x.copy(), y5.copy()
    covered = set()
    for arr, spot in ((x, bad_x), (y, bad_y)):
        if spot is not None:
            (py, px), v = spot
            arr[0, 1, 0, py, px] = v
            covered |= {(iy, ix) for iy in range(3) for ix in range(4) if iy * S <= py < iy * S + R and ix * S <= px < ix * S + R}
    got, want = _run(x, y, R, S)
    assert int(got.rois_skipped[0, 0]) == len(covered) <= 6 and int(got.rois_used[0, 0]) == 24 - len(covered)
    _same(got, want)
    assert all(bool(torch.isfinite(getattr(got, f)).all()) for f in PLANES)


def test_an_all_nan_group_is_nan_and_leaves_the_others_alone():
    R, S, H, W = 32, 16, 70, 83
    x, y5, _ = _field(2, 3, 2, H, W)
    clean = midd_amd.cross_spectrum(_dev(x), _dev(y5), R, S, return_planes=True)
    y = y5.copy()
    y[1, :, 0] = np.nan
    got, want = _run(x, y, R, S)
    _same(got, want)
    assert int(got.rois_used[1, 0]) == 0 and int(got.rois_skipped[1, 0]) == 36
    for f in PLANES + RADIALS:
        assert np.all(getattr(got, f)[1, 0].numpy().view(np.uint64) == np.uint64(ref.QNAN)), f
        for bi, c in ((0, 0), (0, 1), (1, 1)):
            assert torch.equal(getattr(got, f)[bi, c].view(torch.int64), getattr(clean, f)[bi, c].view(torch.int64)), f
    assert np.isnan(float(got.resolution()[1, 0])) and not np.isnan(float(got.resolution()[0, 0]))


# ------------------------------------------------------------------------------ 5. the device against float64 numpy.fft
@pytest.mark.parametrize("R,S,H,W", [SHAPES[1], SHAPES[3], SHAPES[4]])
def test_device_against_float64_fft2(R, S, H, W):
    """sum |S - S*| / sum (sxx* + syy*) <= 2 rho + rho^2 for each of the four quantities, on the device output itself."""
    x, y5, y4 = _field(2, 3, 1, H, W)
    for y in (y5, y4):
        got = midd_amd.cross_spectrum(_dev(x), _dev(y), R, S, "mean", "hann", return_planes=True)
        errs = xref.gate_errors(_stack(got, PLANES), xref.float64_spectra(x, _as5(y), R, S, "mean", ref.hann(R)))
        print(f"R={R} {H}x{W} Ky={_as5(y).shape[1]}: errors {['%.3e' % e for e in errs]}, bound {ref.error_bound(R):.3e}")
        assert max(errs) <= ref.error_bound(R)
        assert min(errs) > 0.0                                     # fp32 arithmetic, not a float64 transform in disguise


# ------------------------------------------------------------------------------ 6. known answers
@pytest.mark.parametrize("R,S,H,W", [SHAPES[1], SHAPES[3], SHAPES[4]])
def test_known_answers_under_the_gate(R, S, H, W):
    """y = x and y = x / 2 (exact in fp32): the four planes against the float64 spectra, and against each other, each difference as
    sum |.| / sum (sxx* + syy*) <= 2 rho + rho^2."""
    x, _, _ = _field(2, 3, 1, H, W)
    xd = _dev(x)
    bound = ref.error_bound(R)
    for factor in (1.0, 0.5):
        got = midd_amd.cross_spectrum(xd, factor * xd, R, S, return_planes=True)
        exact = xref.float64_spectra(x, np.float32(factor) * x, R, S, "plane", ref.hann(R))
        norm = float((exact[0] + exact[1]).sum())
        errs = xref.gate_errors(_stack(got, PLANES), exact)
        e_yy = float((got.syy - factor * factor * got.sxx).abs().sum()) / norm
        e_re = float((got.sxy_re - factor * got.sxx).abs().sum()) / norm
        e_im = float(got.sxy_im.abs().sum()) / norm
        print(f"R={R} y = {factor} x: against float64 {['%.3e' % e for e in errs]}; sum|syy - {factor * factor} sxx| / norm {e_yy:.3e}, "
              f"sum|sxy_re - {factor} sxx| / norm {e_re:.3e}, sum|sxy_im| / norm {e_im:.3e}; bound {bound:.3e}; "
              f"transfer {got.transfer()[0, 0, 1:4].tolist()}")
        assert max(errs) <= bound and max(e_yy, e_re, e_im) <= bound


def test_scaling_by_two_is_exact():
    """Independent of the restatement: a power of two commutes with every rounding here (the inputs are far from the subnormals), so
    cross_spectrum(2x, 2y) is 4 * cross_spectrum(x, y) bit for bit."""
    R, S, H, W = 64, 32, 100, 131
    x, y5, _ = _field(2, 3, 1, H, W)
    one = midd_amd.cross_spectrum(_dev(x), _dev(y5), R, S, return_planes=True)
    two = midd_amd.cross_spectrum(_dev(x) * 2.0, _dev(y5) * 2.0, R, S, return_planes=True)
    for f in PLANES + RADIALS:
        assert torch.equal((4.0 * getattr(one, f)).view(torch.int64), getattr(two, f).view(torch.int64)), f


# ------------------------------------------------------------------------------ 7. compositions
def _denoiser():
    if "cddpm" not in _models:
        sd = make_state_dict(UNetConfig(variant="cddpm", **SMALL), seed=42)
        m = UNetDiffusion(variant="cddpm", **SMALL)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        _models["cddpm"] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models["cddpm"]


def test_compositions_equal_their_parts_and_change_no_existing_call():
    d = _denoiser()
    clean = torch.from_numpy(synthetic_xray(1, 64, 64, seed=31)).cuda()
    noisy = torch.from_numpy(synthetic_xray(1, 64, 64, seed=32)).cuda()
    kw = dict(inference_steps=3, members=4, seed=SEED)
    before = d.denoise_ensemble(noisy, return_samples=True, **kw)
    single = d.denoise(noisy, inference_steps=3, seed=SEED)
    nps = midd_amd.noise_power_spectrum(before.samples, before.mean, 32)
    # one image
    res, fid, base = d.spectral_fidelity(clean, noisy, inference_steps=3, seed=SEED, roi=32)
    assert torch.equal(res, single)
    _equal(fid, midd_amd.cross_spectrum(clean, single, 32), RADIALS + ("rois_used",))
    _equal(base, midd_amd.cross_spectrum(clean, noisy, 32), RADIALS + ("rois_used",))
    assert fid.sxx is None and int(fid.rois_used[0, 0]) == 9
    # members: the samples beside the broadcast truth
    res, fid, base = d.spectral_fidelity(clean, noisy, roi=32, return_planes=True, **kw)
    assert torch.equal(res.samples, before.samples) and torch.equal(res.mean, before.mean) and res.seed == SEED
    _equal(fid, midd_amd.cross_spectrum(clean, before.samples, 32, return_planes=True))
    _same(fid, xref.cross_spectrum(clean.cpu().numpy()[:, None], before.samples.cpu().numpy(), 32, 16, "plane", ref.hann(32)))
    assert int(fid.rois_used[0, 0]) == 4 * 9
    # the FRC between the draw halves
    res, frc = d.ensemble_frc(noisy, roi=32, **kw)
    assert torch.equal(res.samples, before.samples)
    _equal(frc, midd_amd.cross_spectrum(before.samples[:, 0::2], before.samples[:, 1::2], 32), RADIALS + ("rois_used",))
    assert int(frc.rois_used[0, 0]) == 2 * 9 and frc.frc().shape == (1, 1, 17) and 0.0 < float(frc.resolution()[0, 0]) <= 0.5
    # the calls beside them return what they returned before
    after = d.denoise_ensemble(noisy, return_samples=True, **kw)
    assert torch.equal(after.samples, before.samples) and torch.equal(after.mean, before.mean) and torch.equal(after.std, before.std)
    assert torch.equal(d.denoise(noisy, inference_steps=3, seed=SEED), single)
    again = midd_amd.noise_power_spectrum(before.samples, before.mean, 32)
    assert torch.equal(again.nps.view(torch.int64), nps.nps.view(torch.int64)) and torch.equal(again.radial.view(torch.int64), nps.radial.view(torch.int64))


def test_compositions_tiled():
    d = _denoiser()
    clean = torch.from_numpy(synthetic_xray(1, 96, 80, seed=34)).cuda()
    noisy = torch.from_numpy(synthetic_xray(1, 96, 80, seed=33)).cuda()
    kw = dict(inference_steps=3, seed=SEED, tile=64, overlap=16)
    res, fid, base = d.spectral_fidelity(clean, noisy, roi=32, detrend="mean", exclude_axes=True, **kw)
    want = d.denoise_tiled(noisy, **kw)
    assert torch.equal(res.image, want.image)
    _equal(fid, midd_amd.cross_spectrum(clean, want.image, 32, None, "mean", "hann", True), RADIALS + ("rois_used",))
    _equal(base, midd_amd.cross_spectrum(clean, noisy, 32, None, "mean", "hann", True), RADIALS + ("rois_used",))
    assert int(fid.rois_used[0, 0]) == 5 * 4 and bool(torch.isnan(fid.radial_xx[0, 0, 0]))
    res, frc = d.ensemble_frc(noisy, members=2, roi=32, **kw)
    ens = d.denoise_tiled_ensemble(noisy, members=2, return_samples=True, **kw)
    assert torch.equal(res.samples, ens.samples) and res.origins_y == ens.origins_y
    _equal(frc, midd_amd.cross_spectrum(ens.samples[:, 0::2], ens.samples[:, 1::2], 32), RADIALS + ("rois_used",))
    res, fid, _ = d.spectral_fidelity(clean, noisy, members=2, roi=32, **kw)
    assert torch.equal(res.samples, ens.samples)
    _equal(fid, midd_amd.cross_spectrum(clean, ens.samples, 32), RADIALS + ("rois_used",))


# ------------------------------------------------------------------------------ 8. the CLI
def test_cli_fidelity_out(tmp_path, capsys):
    """--fidelity-out beside --truth (with --samples 3: no draw pairs) and beside --samples 4 alone: the JSON holds the library call's
    arrays on the run's own tensors."""
    from PIL import Image

    from midd_amd import cli
    clean = synthetic_xray(1, 72, 88, seed=9)[0, 0].clip(0, 1)
    noisy = (clean + 0.08 * (synthetic_xray(1, 72, 88, seed=10)[0, 0] - 0.5)).clip(0, 1)
    png, truth = tmp_path / "in.png", tmp_path / "truth.png"
    Image.fromarray((noisy * 255).astype(np.uint8), mode="L").save(png)
    Image.fromarray((clean * 255).astype(np.uint8), mode="L").save(truth)
    ckpt = str(tmp_path / "cddpm.pth")                                         # the CLI builds the reference's default topology
    sd = make_state_dict(UNetConfig(variant="cddpm"), seed=42)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "noise_steps": 50}, ckpt)
    base = ["--image", str(png), "--variant", "cddpm", "--checkpoint", ckpt, "--inference-steps", "2", "--seed", "7", "--img-size", "64"]
    images = {}
    for name, extra, kinds in (("truth", ["--samples", "3", "--truth", str(truth)], {"truth_output", "truth_noisy"}),
                               ("draws", ["--samples", "4"], {"draws"})):
        out_json, out_png = tmp_path / f"{name}.json", tmp_path / f"{name}.png"
        cli.main(base + extra + ["--out", str(out_png), "--fidelity-out", str(out_json), "--fidelity-roi", "32", "--fidelity-step", "8"])
        out = capsys.readouterr().out
        got = json.loads(out_json.read_text())
        assert "Spectral fidelity" in out and "Spectral fidelity saved" in out
        assert {k for k in got if k in ("truth_output", "truth_noisy", "draws")} == kinds
        assert (got["roi"], got["step"], got["height"], got["width"], got["seed"]) == (32, 8, 64, 64, 7) and got["freqs"] == [r / 32 for r in range(17)]
        for kind in kinds:
            e = got[kind]
            assert e["rois_used"] == e.get("members", 2) // 2 * 25 and e["rois_skipped"] == 0 and len(e["frc"]) == 17 == len(e["transfer"])
            assert all(-1.0 - 1e-9 <= v <= 1.0 + 1e-9 for v in e["frc"][1:]) and 0.0 < e["resolution"] <= 0.5      # (bin 0 is the detrended DC)
        images[name] = (got, np.asarray(Image.open(out_png)))
        cli.main(base + extra + ["--out", str(tmp_path / "plain.png")])       # the run's image bits are those of the call without the flag
        capsys.readouterr()
        assert np.array_equal(np.asarray(Image.open(tmp_path / "plain.png")), images[name][1])
    # the draws again, through the library on the tensor the CLI builds: the same arrays
    dev = torch.device("cuda")
    inp = torch.from_numpy(np.asarray(Image.open(png).convert("L").resize((64, 64), Image.BICUBIC), np.uint8).astype(np.float32) / 255.0)[None, None].to(dev)
    model = UNetDiffusion(in_channels=1, model_channels=48, channel_mult=(1, 2, 3, 4), num_res_blocks=2, attention_resolutions=(3,), dropout=0.0,
                          time_emb_dim=192, variant="cddpm")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    res = DiffusionDenoiser(model.to(dev).eval(), noise_steps=50).denoise_ensemble(inp, inference_steps=2, members=4, seed=7, return_samples=True)
    want = midd_amd.cross_spectrum(res.samples[:, 0::2], res.samples[:, 1::2], 32, 8)
    got = images["draws"][0]["draws"]
    assert got["frc"] == want.frc()[0, 0].tolist() and got["transfer"] == want.transfer()[0, 0].tolist()
    assert got["resolution"] == float(want.resolution()[0, 0]) and got["members"] == 4
