"""GPU: the noise power spectrum (include/midd.h: THE NOISE POWER SPECTRUM, mi_noise_power_spectrum; midd_amd.noise_power_spectrum,
DiffusionDenoiser.ensemble_nps, cli --nps-out).

The arithmetic is fixed -- the detrend sums, the radix-2 butterflies, the chunked double accumulation, the radial sums -- so the device
is compared bit for bit with the numpy restatement (tests/nps_reference.py): every output, doubles viewed as uint64, at ROI counts
below, at and above the chunk of 16, on rows that take the 16-byte loads and rows that do not.  The same gate as the restatement's
(float64 numpy.fft, the bound derived from Higham's Theorem 24.2) is applied to the device output directly."""
import json

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion
from midd_amd.weights import make_state_dict, synthetic_xray
from tests import nps_reference as ref

pytestmark = pytest.mark.gpu

SMALL = dict(model_channels=16, time_emb_dim=64)
SEED = 0x5EEDC0DE12345678
# (R, S, H, W): a single ROI; unused rows and columns with an odd width, so most rows miss the 16-byte path; a step that divides
# nothing; the two larger transforms
SHAPES = [(32, 16, 32, 32), (32, 16, 70, 83), (32, 5, 40, 45), (64, 32, 100, 131), (128, 64, 128, 200)]
BKC = [(1, 1, 1), (2, 3, 1), (1, 2, 2)]
_fields, _models = {}, {}


def _field(B, K, C, H, W):
    """(a, b) as numpy: seeded noise on a ramp, shared and never written."""
    key = (B, K, C, H, W)
    if key not in _fields:
        _fields[key] = (ref.philox_field((B, K, C, H, W), seed=H * W + K, ramp=0.3), ref.philox_field((B, C, H, W), seed=H * W + 77, ramp=0.25))
    return _fields[key]


def _same(got, want: ref.Nps):
    B, C = want.rois_used.shape
    for name in ("nps", "radial"):
        g, w = getattr(got, name).numpy().reshape(getattr(want, name).shape), getattr(want, name)
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), (name, np.abs(g - w).max())
    assert np.array_equal(got.radial_count.numpy(), want.radial_count)
    assert np.array_equal(got.rois_used.numpy().reshape(B, C), want.rois_used)
    assert np.array_equal(got.rois_skipped.numpy().reshape(B, C), want.rois_skipped)


def _run(a, b, R, S, detrend="plane", window="hann", scale=1.0, exclude_axes=False):
    """The device call and the restatement on the same numpy inputs."""
    got = midd_amd.noise_power_spectrum(torch.from_numpy(a).cuda(), None if b is None else torch.from_numpy(b).cuda(), R, S, detrend, window,
                                        scale, exclude_axes)
    want = ref.noise_power_spectrum(a, b, R, S, detrend, None if window is None else ref.hann(R), scale, exclude_axes)
    return got, want


# ------------------------------------------------------------------------------ 1. the kernels against the restatement
@pytest.mark.parametrize("B,K,C", BKC)
@pytest.mark.parametrize("R,S,H,W", SHAPES)
def test_device_equals_the_restatement_bit_for_bit(R, S, H, W, B, K, C):
    """Every detrend x window on / off x with / without b x exclude_axes on / off."""
    a, b = _field(B, K, C, H, W)
    ny, nx = (H - R) // S + 1, (W - R) // S + 1
    for detrend in ("none", "mean", "plane"):
        for window in (None, "hann"):
            for sub in (None, b):
                for ex in (False, True):
                    got, want = _run(a, sub, R, S, detrend, window, 1.0 if ex else 1.5, ex)
                    assert got.nps.shape == (B, C, R, R) and got.radial.shape == (B, C, R // 2 + 1) and (got.roi, got.step) == (R, S)
                    assert int(got.rois_used.sum()) == B * C * K * ny * nx and int(got.rois_skipped.sum()) == 0
                    _same(got, want)
                    assert bool(torch.isnan(got.radial[..., 0]).all()) == ex and not bool(torch.isnan(got.radial[..., 1:]).any())
    assert got.freqs.tolist() == [r / R for r in range(R // 2 + 1)]


@pytest.mark.parametrize("K,H,W,rois", [(3, 48, 48, 12), (4, 48, 48, 16), (1, 32, 288, 17), (3, 70, 83, 36), (2, 32, 288, 34)])
def test_roi_counts_around_the_chunk(K, H, W, rois):
    """R = 32, S = 16: below a chunk of 16 ROIs, exactly one, one more, and two chunks with a partial third (36; 34 with a member
    boundary inside a chunk)."""
    a, b = _field(1, K, 1, H, W)
    got, want = _run(a, b, 32, 16)
    assert int(got.rois_used[0, 0]) == rois == int(want.rois_used[0, 0])
    _same(got, want)


def test_the_order_of_the_chunk_sums_on_the_device():
    """The hand-made case of the CPU suite: an impulse with P >= 2^53 in ROI 0, then 32 ROIs with P = 1."""
    x = np.float32(2.0 ** 26.5)
    while float(x) ** 2 < 2.0 ** 53:
        x = np.nextafter(x, np.float32(np.inf))
    a = np.zeros((1, 33, 1, 32, 32), np.float32)
    a[0, 0, 0, 0, 0] = x
    a[0, 1:, 0, 0, 0] = 1.0
    got, want = _run(a, None, 32, 32, "none", None)
    _same(got, want)
    assert float(got.nps[0, 0, 3, 5]) == (float(x) ** 2 + 16.0) / (33.0 * 1024.0)


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
    """W a multiple of 4 and the base aligned: every row quad is a 16-byte load.  One element off: none is."""
    a, b = _field(2, 2, 1, H, W)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    assert ad.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
    base = midd_amd.noise_power_spectrum(ad, bd, R, S)
    _same(base, ref.noise_power_spectrum(a, b, R, S, "plane", ref.hann(R)))
    for x, y in ((_offset(ad), bd), (ad, _offset(bd)), (_offset(ad), _offset(bd))):
        assert (x.data_ptr() % 16, y.data_ptr() % 16) != (0, 0)
        got = midd_amd.noise_power_spectrum(x, y, R, S)
        for f in ("nps", "radial", "radial_count", "rois_used", "rois_skipped"):
            assert torch.equal(getattr(got, f).view(torch.int64), getattr(base, f).view(torch.int64)), f


# ------------------------------------------------------------------------------ 3. independence
def test_groups_are_independent_and_the_call_repeats():
    R, S, H, W = 32, 16, 70, 83
    a, b = _field(2, 3, 2, H, W)
    ad, bd = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    full = midd_amd.noise_power_spectrum(ad, bd, R, S)
    again = midd_amd.noise_power_spectrum(ad, bd, R, S)
    for f in ("nps", "radial", "radial_count", "rois_used", "rois_skipped"):
        assert torch.equal(getattr(full, f).view(torch.int64), getattr(again, f).view(torch.int64)), f
    for bi in range(2):
        for c in range(2):
            one = midd_amd.noise_power_spectrum(ad[bi:bi + 1, :, c:c + 1], bd[bi:bi + 1, c:c + 1], R, S)
            assert torch.equal(one.nps[0, 0].view(torch.int64), full.nps[bi, c].view(torch.int64))
            assert torch.equal(one.radial[0, 0].view(torch.int64), full.radial[bi, c].view(torch.int64))
            assert int(one.rois_used[0, 0]) == int(full.rois_used[bi, c]) == 36
    # the accepted shapes: [B, C, H, W] is K = 1, [H, W] drops the group axes
    four = midd_amd.noise_power_spectrum(ad[:, 0], bd, R, S)
    five = midd_amd.noise_power_spectrum(ad[:, :1], bd, R, S)
    assert torch.equal(four.nps.view(torch.int64), five.nps.view(torch.int64)) and four.nps.shape == (2, 2, R, R)
    flat = midd_amd.noise_power_spectrum(ad[1, 0, 1], bd[1, 1], R, S)
    assert flat.nps.shape == (R, R) and flat.radial.shape == (R // 2 + 1,) and flat.rois_used.shape == ()
    assert torch.equal(flat.nps.view(torch.int64), four.nps[1, 1].view(torch.int64)) and float(flat.variance()) > 0.0


# ------------------------------------------------------------------------------ 4. non-finite data
@pytest.mark.parametrize("where,bad", [((20, 40), np.nan), ((0, 0), np.inf), ((69, 82), -np.inf), ((33, 17), np.nan)])
def test_a_non_finite_pixel_skips_exactly_the_rois_that_cover_it(where, bad):
    """70 x 83, R 32, S 16: 12 ROIs per member.  The pixel sits in member 1 of 2; (69, 82) lies in no ROI."""
    R, S, H, W = 32, 16, 70, 83
    a, b = _field(1, 2, 1, H, W)
    a = a.copy()
    a[0, 1, 0, where[0], where[1]] = bad
    covering = sum(1 for iy in range(3) for ix in range(4) if iy * S <= where[0] < iy * S + R and ix * S <= where[1] < ix * S + R)
    assert covering <= 4
    got, want = _run(a, b, R, S)
    assert int(got.rois_skipped[0, 0]) == covering and int(got.rois_used[0, 0]) == 24 - covering >= 20
    _same(got, want)
    assert bool(torch.isfinite(got.nps).all())
    # Inf - Inf in f = a - b is a NaN of the field
    if bad == np.inf:
        b2 = b.copy()
        b2[0, 0, where[0], where[1]] = np.inf
        got2, want2 = _run(a, b2, R, S)
        assert int(got2.rois_skipped[0, 0]) == 1 + covering       # member 0 now holds -Inf there as well
        _same(got2, want2)


def test_an_all_nan_group_is_nan_and_leaves_the_others_alone():
    R, S, H, W = 32, 16, 70, 83
    a, b = _field(2, 3, 2, H, W)
    clean = midd_amd.noise_power_spectrum(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), R, S)
    a = a.copy()
    a[1, :, 0] = np.nan
    got, want = _run(a, b, R, S)
    _same(got, want)
    assert int(got.rois_used[1, 0]) == 0 and int(got.rois_skipped[1, 0]) == 36
    assert bool(torch.isnan(got.nps[1, 0]).all()) and bool(torch.isnan(got.radial[1, 0]).all())
    for bi, c in ((0, 0), (0, 1), (1, 1)):
        assert torch.equal(got.nps[bi, c].view(torch.int64), clean.nps[bi, c].view(torch.int64))
        assert torch.equal(got.radial[bi, c].view(torch.int64), clean.radial[bi, c].view(torch.int64))


# ------------------------------------------------------------------------------ 5. the device against float64 numpy.fft
@pytest.mark.parametrize("R,S,H,W", SHAPES[1:])
def test_device_against_float64_fft2(R, S, H, W):
    """The gate of the CPU suite on the device output itself, not through the restatement's transform."""
    a, b = _field(2, 3, 1, H, W)
    w = ref.hann(R)
    got = midd_amd.noise_power_spectrum(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), R, S, "mean", "hann").nps.numpy()
    f = a - b[:, None]
    for bi in range(2):
        d = ref.detrend_window(ref.cut_rois(f[bi, :, 0], R, S), "mean", w)
        want = (np.abs(np.fft.fft2(d.astype(np.float64))) ** 2).mean(axis=0) / float((w.astype(np.float64) ** 2).sum() ** 2)
        err = np.abs(got[bi, 0] - want).sum() / want.sum()
        print(f"R={R} {H}x{W} image {bi}: relative L1 error {err:.3e}, bound {ref.error_bound(R):.3e}")
        assert err <= ref.error_bound(R)


# ------------------------------------------------------------------------------ 6. compositions
def _denoiser():
    if "cddpm" not in _models:
        sd = make_state_dict(UNetConfig(variant="cddpm", **SMALL), seed=42)
        m = UNetDiffusion(variant="cddpm", **SMALL)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        _models["cddpm"] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models["cddpm"]


def _equal_nps(a, b):
    for f in ("nps", "radial", "radial_count", "freqs", "rois_used", "rois_skipped"):
        assert torch.equal(getattr(a, f).view(torch.int64), getattr(b, f).view(torch.int64)), f
    assert (a.roi, a.step) == (b.roi, b.step)


def test_ensemble_nps_is_the_composition_and_changes_no_existing_call():
    d = _denoiser()
    noisy = torch.from_numpy(synthetic_xray(1, 64, 64, seed=32)).cuda()
    kw = dict(inference_steps=3, members=3, seed=SEED)
    before = d.denoise_ensemble(noisy, return_samples=True, **kw)
    single = d.denoise(noisy, inference_steps=3, seed=SEED)
    res, sp = d.ensemble_nps(noisy, roi=32, **kw)
    assert torch.equal(res.samples, before.samples) and torch.equal(res.mean, before.mean) and torch.equal(res.std, before.std) and res.seed == SEED
    _equal_nps(sp, midd_amd.noise_power_spectrum(before.samples, before.mean, 32, scale=3 / 2))
    host = ref.noise_power_spectrum(before.samples.cpu().numpy(), before.mean.cpu().numpy(), 32, 16, "plane", ref.hann(32), 1.5)
    _same(sp, host)
    assert int(sp.rois_used[0, 0]) == 3 * 9 and bool((sp.nps >= 0).all()) and float(sp.variance()[0, 0]) > 0.0
    res64, sp64 = d.ensemble_nps(noisy, **kw)                                 # the default ROI of 64: one ROI per member
    _equal_nps(sp64, midd_amd.noise_power_spectrum(before.samples, before.mean, scale=1.5))
    assert int(sp64.rois_used[0, 0]) == 3 and sp64.step == 32
    # the calls beside it return what they returned before it ran
    after = d.denoise_ensemble(noisy, return_samples=True, **kw)
    assert torch.equal(after.samples, before.samples) and torch.equal(after.mean, before.mean) and torch.equal(after.std, before.std)
    assert torch.equal(d.denoise(noisy, inference_steps=3, seed=SEED), single)


def test_ensemble_nps_tiled_is_the_composition():
    d = _denoiser()
    noisy = torch.from_numpy(synthetic_xray(1, 96, 80, seed=33)).cuda()
    kw = dict(inference_steps=3, members=3, seed=SEED, tile=64, overlap=16)
    res, sp = d.ensemble_nps(noisy, roi=32, detrend="mean", exclude_axes=True, **kw)
    want = d.denoise_tiled_ensemble(noisy, return_samples=True, **kw)
    assert torch.equal(res.samples, want.samples) and torch.equal(res.mean, want.mean) and res.origins_y == want.origins_y
    _equal_nps(sp, midd_amd.noise_power_spectrum(want.samples, want.mean, 32, None, "mean", "hann", 1.5, True))
    assert int(sp.rois_used[0, 0]) == 3 * 5 * 4 and bool(torch.isnan(sp.radial[0, 0, 0]))


# ------------------------------------------------------------------------------ 7. the CLI
def test_cli_nps_out(tmp_path, capsys):
    """--nps-out beside --samples K with --truth and beside --tile N --members K: the JSON holds the radial arrays of
    the library call on the run's own tensors."""
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
    base = ["--image", str(png), "--variant", "cddpm", "--checkpoint", ckpt, "--inference-steps", "2", "--seed", "7", "--out", str(tmp_path / "out.png")]
    for extra, kinds, shape in ((["--img-size", "64", "--nps-roi", "32", "--nps-step", "8", "--samples", "3", "--truth", str(truth)],
                                 {"method_noise", "ensemble_spread", "residual"}, (64, 64)),
                                (["--tile", "64", "--overlap", "16", "--members", "2"], {"method_noise", "ensemble_spread"}, (72, 88))):
        out_json = tmp_path / "nps.json"
        cli.main(base + extra + ["--nps-out", str(out_json)])
        out = capsys.readouterr().out
        got = json.loads(out_json.read_text())
        R = got["roi"]
        assert "Noise power spectrum" in out and "Noise power spectra saved" in out
        assert {k for k in got if k in ("method_noise", "ensemble_spread", "residual")} == kinds
        assert (got["height"], got["width"]) == shape and got["freqs"] == [r / R for r in range(R // 2 + 1)] and got["seed"] == 7
        ny, nx = (shape[0] - R) // got["step"] + 1, (shape[1] - R) // got["step"] + 1
        for kind in kinds:
            e = got[kind]
            K = e.get("members", 1)
            assert e["rois_used"] == K * ny * nx and e["rois_skipped"] == 0 and len(e["radial"]) == R // 2 + 1 == len(e["radial_count"])
            assert all(v >= 0.0 for v in e["radial"]) and e["variance"] > 0.0
            assert e["radial_count"] == ref.radial_profile(np.zeros((R, R)), False)[1].tolist()
    # the tiled method noise again, through the library on the tensors the CLI builds: the same radial array
    dev = torch.device("cuda")
    inp = torch.from_numpy(np.asarray(Image.open(png).convert("L"), np.uint8).astype(np.float32) / 255.0)[None, None].to(dev)
    model = UNetDiffusion(in_channels=1, model_channels=48, channel_mult=(1, 2, 3, 4), num_res_blocks=2, attention_resolutions=(3,), dropout=0.0,
                          time_emb_dim=192, variant="cddpm")
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    res = DiffusionDenoiser(model.to(dev).eval(), noise_steps=50).denoise_tiled_ensemble(inp, inference_steps=2, members=2, tile=64, overlap=16,
                                                                                         seed=7, return_samples=True)
    want = midd_amd.noise_power_spectrum(inp, res.mean, 64)
    assert got["method_noise"]["radial"] == want.radial[0, 0].tolist() and got["method_noise"]["variance"] == float(want.variance()[0, 0])
    spread = midd_amd.noise_power_spectrum(res.samples, res.mean, 64, scale=2.0)
    assert got["ensemble_spread"]["radial"] == spread.radial[0, 0].tolist()
