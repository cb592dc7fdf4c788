"""CPU-only checks of the cross-spectrum (include/midd.h: THE CROSS SPECTRUM, mi_cross_spectrum): the numpy restatement
(tests/cross_spectrum_reference.py) against float64 numpy.fft within the bound derived from Higham's Theorem 24.2 relative to the two
fields' combined energy, the separation identities on hand-made inputs that involve no FFT library, the sign of the Im Sxy mirror, the
host-side curves, the argument rules of the C ABI through the library loaded without a device, the Python and CLI argument rules, and
the ISA metadata of the new kernels.  What the device computes is judged in test_gpu_cross_spectrum.py."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetDiffusion, native
from tests import cross_spectrum_reference as xref
from tests import nps_reference as ref
from tests.isa_dump import isa_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_cross_spectrum", "mi_cross_spectrum_workspace_bytes"}
SIZES = (32, 64, 128)


# ------------------------------------------------------------------------------ 1. the restatement against float64 numpy.fft
def _blur(x):
    """A 3 x 3 box blur with edge replication, in float32: the high frequencies of x removed."""
    p = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(1, 1), (1, 1)], mode="edge")
    H, W = x.shape[-2:]
    return (sum(p[..., i:i + H, j:j + W] for i in range(3) for j in range(3)) / np.float32(9.0)).astype(np.float32)


@pytest.mark.parametrize("R", SIZES)
@pytest.mark.parametrize("kind,detrend,windowed", [("noise", "mean", False), ("noise", "plane", True), ("blur", "plane", True),
                                                   ("weak", "mean", True), ("single", "none", False)])
def test_restatement_against_float64_fft2(R, kind, detrend, windowed):
    """sum |S - S*| / sum (sxx* + syy*) <= 2 rho + rho^2 for each of the four quantities: noise-on-a-ramp pairs, a blurred pair, a y
    of 1e-3 of x's amplitude (the error is relative to the COMBINED energy), and a y with one realisation."""
    H, W = R + R // 2 + 3, 2 * R + 5
    x = ref.philox_field((1, 2, 1, H, W), seed=R + 1, ramp=0.3)
    if kind == "blur":
        y = _blur(x)
    elif kind == "weak":
        y = (np.float32(1e-3) * ref.philox_field((1, 2, 1, H, W), seed=R + 2, ramp=0.1)).astype(np.float32)
    elif kind == "single":
        y = ref.philox_field((1, 1, 1, H, W), seed=R + 3, ramp=0.2)
    else:
        y = ref.philox_field((1, 2, 1, H, W), seed=R + 2, ramp=0.1)
    w = ref.hann(R) if windowed else None
    got = xref.cross_spectrum(x, y, R, R // 2, detrend, w)
    errs = xref.gate_errors(got.planes, xref.float64_spectra(x, y, R, R // 2, detrend, w))
    print(f"R={R} {kind} detrend={detrend} window={windowed}: errors {['%.3e' % e for e in errs]}, bound {ref.error_bound(R):.3e}")
    assert max(errs) <= ref.error_bound(R)
    assert min(errs[:2]) > 0                                     # fp32 arithmetic, not a float64 transform in disguise
    assert got.rois_used[0, 0] == 2 * 2 * 3 and got.rois_skipped[0, 0] == 0


# ------------------------------------------------------------------------------ 2. the separation, no FFT library
@pytest.mark.parametrize("R", SIZES)
def test_an_impulse_in_x_only(R):
    """x = a at one pixel, y = 0: Z = X exactly (every butterfly adds or subtracts a product with a unit-modulus twiddle), so
    Sxx = |X|^2 = a^2 at every frequency up to the transform's bound, and Syy, Sxy are at most that bound of it."""
    a = np.float32(0.75)
    x = np.zeros((1, 1, 1, R, R), np.float32)
    x[0, 0, 0, 3, 5] = a
    got = xref.cross_spectrum(x, np.zeros_like(x), R, R, "none", None).planes[:, 0, 0]
    bound, total = ref.error_bound(R), float(a) ** 2                 # sum (sxx* + syy*): R^2 entries of a^2 / S_w, S_w = R^2
    assert np.abs(got[0] - total / (R * R)).sum() <= bound * total
    for q in (1, 2, 3):
        assert np.abs(got[q]).sum() <= bound * total, q


@pytest.mark.parametrize("R,sy,sx", [(32, 0, 1), (64, 3, 0), (128, 2, 5), (32, 31, 17)])
def test_y_a_shifted_x(R, sy, sx):
    """x an impulse a at the origin, y the same impulse at (sy, sx): X = a, Y = a exp(-2 pi i (v sy + u sx) / R), so
    Sxy = X conj(Y) = a^2 exp(+2 pi i (v sy + u sx) / R) / S_w and Sxx = Syy = a^2 / S_w."""
    a = 0.5
    x = np.zeros((1, 1, 1, R, R), np.float32)
    y = np.zeros_like(x)
    x[0, 0, 0, 0, 0] = a
    y[0, 0, 0, sy, sx] = a
    got = xref.cross_spectrum(x, y, R, R, "none", None).planes[:, 0, 0]
    v, u = np.mgrid[0:R, 0:R]
    ang = 2.0 * np.pi * (v * sy + u * sx) / R
    want = np.stack([np.ones((R, R)), np.ones((R, R)), np.cos(ang), np.sin(ang)]) * (a * a / (R * R))
    norm = (want[0] + want[1]).sum()
    errs = [float(np.abs(got[q] - want[q]).sum() / norm) for q in range(4)]
    print(f"R={R} shift ({sy}, {sx}): errors {['%.3e' % e for e in errs]}, bound {ref.error_bound(R):.3e}")
    assert max(errs) <= ref.error_bound(R)
    assert np.abs(want[3]).sum() > 0.2 * norm                       # the imaginary part is really there, with this sign


@pytest.mark.parametrize("R", SIZES)
def test_the_mirror_copies_three_planes_and_negates_the_fourth(R):
    x = ref.philox_field((1, 1, 1, R, R + 9), seed=3 * R, ramp=0.2)
    y = ref.philox_field((1, 1, 1, R, R + 9), seed=3 * R + 1)
    got = xref.cross_spectrum(x, y, R, 4, "mean", ref.hann(R)).planes[:, 0, 0]
    mv = (R - np.arange(R)) % R
    for q, sign in ((0, 1.0), (1, 1.0), (2, 1.0), (3, -1.0)):
        mirrored = got[q][mv][:, mv]                                  # entry (-v, -u)
        inner = (slice(None), slice(1, R // 2))                       # 0 < u < R/2: the written mirror
        assert np.array_equal(got[q][inner], sign * mirrored[inner]), q
    assert np.abs(got[3]).max() > 0 and got[3][0, 0] == 0.0 and got[3][R // 2, R // 2] == 0.0
    # the device writes the negation, not a second computation: (v, u) and (-v, -u) of Im Sxy cancel exactly in every radial bin
    radial = xref.cross_spectrum(x, y, R, 4, "mean", ref.hann(R)).radial[3, 0, 0]
    assert np.abs(radial).max() <= 1e-12 * np.abs(got[3]).max()


def test_the_summation_order_is_the_specified_one():
    """Chunks of 16 ROIs, as in the NPS: Sxx = x^2 >= 2^53 in ROI 0, Sxx = 1 in the 32 ROIs after it."""
    R = 32
    big32 = np.float32(2.0 ** 26.5)
    while float(big32) ** 2 < 2.0 ** 53:
        big32 = np.nextafter(big32, np.float32(np.inf))
    x = np.zeros((1, 33, 1, R, R), np.float32)
    x[0, 0, 0, 0, 0] = big32
    x[0, 1:, 0, 0, 0] = 1.0
    got = xref.cross_spectrum(x, np.zeros((1, 1, 1, R, R), np.float32), R, R, "none", None).planes[0, 0, 0]
    big = float(big32) ** 2
    assert big + 1.0 == big and np.all(got == got[0, 0])
    assert got[0, 0] == (big + 16.0) / (33.0 * 1024.0) != (big + 32.0) / (33.0 * 1024.0)


# ------------------------------------------------------------------------------ 3. the curves on the host
def _spectrum(xx, yy, re, used=1):
    t = lambda v: torch.tensor([[v]], dtype=torch.float64)      # noqa: E731
    bins = len(xx)
    return midd_amd.CrossSpectrum(None, None, None, None, t(xx), t(yy), t(re), t([0.0] * bins), torch.ones(bins, dtype=torch.int64),
                                  torch.arange(bins, dtype=torch.float64) / (2 * (bins - 1)), torch.tensor([[used]]), torch.tensor([[0]]),
                                  2 * (bins - 1), bins - 1)


def test_transfer_frc_and_resolution():
    sp = _spectrum([4.0, 4.0, 4.0, 4.0, 4.0], [1.0, 1.0, 1.0, 1.0, 1.0], [2.0, 1.8, 1.0, 0.2, 0.1])
    assert sp.transfer()[0, 0].tolist() == [0.5, 0.45, 0.25, 0.05, 0.025]
    assert sp.frc()[0, 0].tolist() == [1.0, 0.9, 0.5, 0.1, 0.05]
    # 1/7 lies between bins 2 (0.5) and 3 (0.1): f = 0.25 + (0.5 - 1/7) / 0.4 * 0.125
    assert float(sp.resolution()[0, 0]) == pytest.approx(0.25 + (0.5 - 1.0 / 7.0) / 0.4 * 0.125, abs=1e-15)
    assert float(sp.resolution(0.5)[0, 0]) == 0.25                   # bin 2 sits ON the threshold, bin 3 is the first below: the crossing is at bin 2
    assert float(sp.resolution(0.95)[0, 0]) == 0.125                 # bin 1 itself is below: its own frequency
    assert float(sp.resolution(0.01)[0, 0]) == 0.5                   # never below
    assert math.isnan(float(_spectrum([math.nan] * 5, [math.nan] * 5, [math.nan] * 5, used=0).resolution()[0, 0]))


# ------------------------------------------------------------------------------ 4. the C ABI: every rule before anything is read
X_, Y_, PL, RAD, CNT, USED, SKIP, WS = (0x10000000 * (i + 1) for i in range(8))      # non-null "device pointers"
NEED = 2 * 3 * (4 * 32 * 17 + 1) * 8


def _call(**kw):
    """mi_cross_spectrum with fake pointers: every call here must fail before anything reads them."""
    a = dict(x=X_, y=Y_, B=2, Kx=3, Ky=3, C=1, H=70, W=83, roi=32, step=16, detrend=2, window=None, flags=0, planes=PL, radial=RAD,
             radial_count=CNT, rois_used=USED, rois_skipped=SKIP, workspace=WS, workspace_bytes=NEED)
    a.update(kw)
    lib = native.lib()
    w = a["window"]
    if isinstance(w, (list, tuple)):
        w = (C.c_float * len(w))(*w)
    elif isinstance(w, int):
        w = C.cast(w, C.POINTER(C.c_float))
    rc = lib.mi_cross_spectrum(a["x"], a["y"], a["B"], a["Kx"], a["Ky"], a["C"], a["H"], a["W"], a["roi"], a["step"], a["detrend"], w, a["flags"],
                               a["planes"], a["radial"], a["radial_count"], a["rois_used"], a["rois_skipped"], a["workspace"],
                               a["workspace_bytes"], None)
    return rc, lib.mi_last_error().decode()


FAKE_WINDOW = 0x90000000          # never read: every rule below is judged before the window
RULES = [
    (dict(Ky=0), ["Ky 0", "at least one realisation"]),
    (dict(Kx=2), ["Kx 2, Ky 3", "Kx, Ky in {K, 1}"]),
    (dict(roi=48), ["roi 48 outside {32, 64, 128}"]),
    (dict(step=0), ["step 0 below 1"]),
    (dict(C=0), ["C 0", "at least 1"]),
    (dict(B=65536), ["65536 groups outside [1, 65535]"]),
    (dict(H=31), ["image 31 x 83 smaller than the ROI 32 x 32"]),
    (dict(detrend=3), ["detrend 3 outside"]),
    (dict(flags=2), ["flags 0x2", "unknown bits"]),
    (dict(planes=None), ["null argument"]),
    (dict(radial=RAD + 4), ["8-byte aligned"]),
    (dict(workspace_bytes=NEED - 1), ["workspace too small", str(NEED)]),
    (dict(rois_used=PL + 8), ["planes and rois_used alias"]),
]


@pytest.mark.parametrize("first", range(len(RULES)))
def test_every_argument_rule_in_its_place(first):
    """Rule `first` alone, and rule `first` with every later rule broken as well: its message either way, and the (fake) window,
    the last thing the call looks at, is never read."""
    for broken in (RULES[first:first + 1], RULES[first:]):
        kw = dict(window=FAKE_WINDOW)
        for change, _ in reversed(broken):
            kw.update(change)
        if "Ky" in kw and "Kx" in kw and first == 0:
            kw["Kx"] = 3                                              # (Ky = 0 beside Kx = 2: the first rule names both)
        rc, msg = _call(**kw)
        assert rc == -1, (kw, rc, msg)
        for word in RULES[first][1]:
            assert word in msg, (kw, msg)


def test_further_argument_rules_and_the_workspace_query():
    lib = native.lib()
    for kw, word in [(dict(Kx=0), "Kx 0"), (dict(Kx=-1, Ky=1), "Kx -1"), (dict(Kx=4), "Kx 4, Ky 3"), (dict(roi=0), "roi 0 outside"),
                     (dict(roi=256), "roi 256 outside"), (dict(step=-3), "step -3 below 1"), (dict(B=0), "B 0"), (dict(W=31), "smaller than the ROI"),
                     (dict(H=127, roi=128), "smaller than the ROI"), (dict(detrend=-1), "detrend -1"), (dict(flags=-1), "unknown bits"),
                     (dict(x=None), "null"), (dict(y=None), "null"), (dict(radial=None), "null"), (dict(radial_count=None), "null"),
                     (dict(rois_used=None), "null"), (dict(rois_skipped=None), "null"), (dict(workspace=None), "null"), (dict(planes=PL + 4), "8-byte"),
                     (dict(radial_count=CNT + 2), "8-byte"), (dict(rois_skipped=SKIP + 1), "8-byte"), (dict(workspace=WS + 4), "8-byte"),
                     (dict(x=X_ + 2), "4-byte"), (dict(y=Y_ + 1), "4-byte"), (dict(workspace_bytes=0), "too small"),
                     (dict(planes=X_ + 8), "x and planes alias"), (dict(workspace=Y_ + 8), "y and workspace alias"),
                     (dict(radial=PL + 4 * 2 * 32 * 32 * 8 - 8), "planes and radial alias"), (dict(rois_skipped=USED + 8), "rois_used and rois_skipped alias"),
                     (dict(window=[0.5] * 31 + [float("nan")]), "window[31] is not finite")]:
        rc, msg = _call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    # the four planes of the second group end where a buffer of ONE plane per group would: an alias only for the real size
    rc, msg = _call(radial=PL + 2 * 32 * 32 * 8)
    assert rc == -1 and "planes and radial alias" in msg
    ws = lib.mi_cross_spectrum_workspace_bytes
    part = {32: 4 * 32 * 17 + 1, 64: 4 * 64 * 33 + 1, 128: 4 * 128 * 65 + 1}
    assert ws(1, 1, 1, 1, 32, 32, 32, 16) == part[32] * 8                       # one ROI: one chunk
    assert ws(1, 4, 1, 1, 48, 48, 32, 16) == part[32] * 8                       # K = max(Kx, Ky) = 4: 16 ROIs, one chunk
    assert ws(1, 1, 4, 1, 48, 48, 32, 16) == part[32] * 8
    assert ws(1, 1, 1, 1, 32, 288, 32, 16) == 2 * part[32] * 8                  # 17 ROIs: two chunks
    assert ws(2, 3, 3, 2, 70, 83, 32, 16) == 4 * 3 * part[32] * 8               # 36 ROIs per group: three chunks
    assert ws(1, 8, 1, 1, 2500, 2048, 64, 32) == ((8 * 77 * 63 + 15) // 16) * part[64] * 8
    assert ws(1, 2, 2, 1, 128, 200, 128, 64) == part[128] * 8
    for bad in [(0, 1, 1, 1, 64, 64, 32, 16), (1, 2, 3, 1, 64, 64, 32, 16), (1, 0, 1, 1, 64, 64, 32, 16), (1, 1, 1, 1, 64, 64, 33, 16),
                (1, 1, 1, 1, 64, 64, 32, 0), (1, 1, 1, 1, 31, 64, 32, 16), (256, 1, 1, 256, 64, 64, 32, 16)]:
        assert ws(*bad) == 0 and lib.mi_last_error(), bad


def test_x_and_y_may_be_the_same_field():
    """Both are only read: y == x passes every rule up to the window, the last one judged."""
    rc, msg = _call(y=X_, window=[0.5] * 31 + [float("inf")])
    assert rc == -1 and "window[31] is not finite" in msg


# ------------------------------------------------------------------------------ 5. header and bindings
def test_header_and_binding_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in native.SYMBOLS}
    assert NEW <= declared and declared == bound
    for name in NEW:
        assert getattr(native.lib(), name) is not None
    for words in ("THE CROSS SPECTRUM", "Z2 = Z[(R-v)%R][(R-u)%R]", "n1 = x1*x1 + y1*y1", "c  = x1*x2 - y1*y2        s  = x1*y2 + y1*x2",
                  "Sxx = ((n1 + n2) + 2c) / 4        Syy = ((n1 + n2) - 2c) / 4", "Re Sxy = s / 2                    Im Sxy = (n1 - n2) / 4",
                  "ALL R columns", "x OR y holds a NaN or an Inf", "its negation for Im Sxy", "COMBINED energy", "Kx, Ky in {K, 1}"):
        assert words in header, words


# ------------------------------------------------------------------------------ 6. the Python and CLI argument rules
def test_python_surface_without_a_gpu():
    assert midd_amd.CrossSpectrum._fields == ("sxx", "syy", "sxy_re", "sxy_im", "radial_xx", "radial_yy", "radial_xy_re", "radial_xy_im",
                                              "radial_count", "freqs", "rois_used", "rois_skipped", "roi", "step")
    from midd_amd import sampler
    assert sampler.cross_spectrum is midd_amd.cross_spectrum and sampler.CrossSpectrum is midd_amd.CrossSpectrum
    sig = inspect.signature(midd_amd.cross_spectrum).parameters
    assert list(sig) == ["x", "y", "roi", "step", "detrend", "window", "exclude_axes", "return_planes"]
    assert [sig[k].default for k in list(sig)[2:]] == [64, None, "plane", "hann", False, False]
    for method, lead in ((DiffusionDenoiser.spectral_fidelity, ["self", "clean", "noisy", "inference_steps", "members"]),
                         (DiffusionDenoiser.ensemble_frc, ["self", "noisy", "inference_steps", "members"])):
        sig = inspect.signature(method).parameters
        assert list(sig)[:len(lead)] == lead and {"seed", "tile", "overlap", "roi", "step", "detrend", "window", "exclude_axes"} <= set(sig)
        assert (sig["inference_steps"].default, sig["seed"].default, sig["tile"].default, sig["overlap"].default, sig["roi"].default) == (25, None, None, 32, 64)
    assert inspect.signature(DiffusionDenoiser.spectral_fidelity).parameters["members"].default is None
    assert inspect.signature(DiffusionDenoiser.ensemble_frc).parameters["members"].default == 8
    x = torch.zeros(1, 2, 1, 64, 64)
    for kw, word in [(dict(roi=48), "roi must be one of"), (dict(roi=True), "roi must be one of"), (dict(step=0), "step must be"),
                     (dict(detrend="linear"), "detrend must be"), (dict(window="hamming"), "window must be"), (dict(window=[1.0] * 63), "window must be"),
                     (dict(roi=128), "smaller than the ROI")]:
        with pytest.raises(ValueError, match=re.escape(word)):
            midd_amd.cross_spectrum(x, x, **kw)
    for y, word in [(torch.zeros(1, 3, 1, 64, 64), "must have the same shape"), (torch.zeros(1, 1, 64, 32), "B, C, H and W must agree"),
                    (torch.zeros(64, 64), "must have the same shape"), (torch.zeros(3, 64, 64), "y must be a [B, K, C, H, W]")]:
        with pytest.raises(ValueError, match=re.escape(word)):
            midd_amd.cross_spectrum(x, y)
    with pytest.raises(ValueError, match="x must be"):
        midd_amd.cross_spectrum(torch.zeros(3, 64, 64), x)
    for a, b in ((x, x), (x, x[:, 0]), (x[:, 0], x), (x[:, 0], x[:, 0]), (x[0, 0, 0], x[0, 0, 0])):      # valid CPU tensors: never a silent fall-back
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            midd_amd.cross_spectrum(a, b)
    # the compositions: their own rules, then those of the calls they compose
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    img = torch.zeros(1, 1, 64, 64)
    for members in (1, 3, 0):
        with pytest.raises(ValueError, match="even members >= 2|members"):
            d.ensemble_frc(img, inference_steps=2, members=members, seed=1, roi=32)
    with pytest.raises(ValueError, match="even members >= 2"):
        d.ensemble_frc(img, inference_steps=2, members=3, seed=1, roi=32)
    with pytest.raises(ValueError, match="roi must be one of"):
        d.ensemble_frc(img, inference_steps=2, members=2, seed=1, roi=16)
    with pytest.raises(ValueError, match="roi must be one of"):
        d.spectral_fidelity(img, img, inference_steps=2, roi=16)
    with pytest.raises(ValueError, match="clean must be a tensor of the noisy images' shape"):
        d.spectral_fidelity(torch.zeros(1, 1, 64, 32), img, inference_steps=2, roi=32)
    with pytest.raises(TypeError, match="clean must be float32"):
        d.spectral_fidelity(img.double(), img, inference_steps=2, roi=32)
    for kw in (dict(), dict(members=2), dict(tile=32, overlap=8), dict(members=2, tile=32, overlap=8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            d.spectral_fidelity(img, img, inference_steps=2, seed=1, roi=32, **kw)
    for kw in (dict(), dict(tile=32, overlap=8)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            d.ensemble_frc(img, inference_steps=2, members=2, seed=1, roi=32, **kw)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="deterministic sampler has no ensemble"):
        ddim.ensemble_frc(img, inference_steps=2, members=2, seed=1, roi=32)


def test_cli_refusals(capsys):
    from midd_amd import cli
    sig = inspect.signature(cli.denoise_image_diffusion).parameters
    assert sig["fidelity_out"].default is None and sig["fidelity_roi"].default is None and sig["fidelity_step"].default is None
    base = ["--image", "nowhere.png"]
    needs = "--fidelity-out needs --truth PATH"
    for argv, word in [(["--fidelity-roi", "32"], "--fidelity-out PATH.json"), (["--fidelity-step", "8"], "--fidelity-out PATH.json"),
                       (["--fidelity-out", "f.json", "--samples", "2", "--fidelity-roi", "48"], "--fidelity-roi needs one of"),
                       (["--fidelity-out", "f.json", "--samples", "2", "--fidelity-step", "0"], "--fidelity-step needs S >= 1"),
                       (["--fidelity-out", "f.json"], needs), (["--fidelity-out", "f.json", "--samples", "3"], needs),
                       (["--fidelity-out", "f.json", "--members", "2"], needs), (["--fidelity-out", "f.json", "--tile", "64"], needs),
                       (["--fidelity-out", "f.json", "--samples", "2", "--img-size", "48"], "smaller than the ROI")]:
        with pytest.raises(SystemExit):
            cli.main(argv + base)
        assert word in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="need --fidelity-out"):
        cli.denoise_image_diffusion(None, "nowhere.png", fidelity_roi=32)
    with pytest.raises(ValueError, match=re.escape(needs)):
        cli.denoise_image_diffusion(None, "nowhere.png", fidelity_out="f.json")
    with pytest.raises(ValueError, match=re.escape(needs)):
        cli.denoise_image_diffusion(None, "nowhere.png", fidelity_out="f.json", samples=5)
    with pytest.raises(ValueError, match="roi must be one of"):
        cli.denoise_image_diffusion(None, "nowhere.png", fidelity_out="f.json", samples=2, fidelity_roi=48)
    with pytest.raises(ValueError, match="smaller than the ROI"):
        cli.denoise_image_diffusion(None, "nowhere.png", fidelity_out="f.json", samples=2, img_size=32)
    with pytest.raises(RuntimeError, match="only on a ROCm GPU"):
        cli.denoise_image_diffusion(None, "nowhere.png", device_type="cpu", fidelity_out="f.json", samples=2)


# ------------------------------------------------------------------------------ 7. static: the kernels' ISA
def _metadata(text):
    notes = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - ", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_no_cross_spectrum_kernel_touches_scratch():
    """Every instantiation (R in {32, 64, 128} of the ROI, sum and radial kernels) has a private segment of 0 bytes and no spilled
    VGPR -- R = 128 with its four accumulators per entry included: 512 lanes, each under the 256 registers that leaves --; the
    butterflies are plain fp32 multiplications and additions, the sums plain double adds; no atomics on global memory; the ROI
    kernel reads 16-byte words; its LDS is the padded complex plane."""
    text = isa_dump("cross_spectrum.hip")
    meta = _metadata(text)
    seen = set()
    for name, fields in meta.items():
        assert fields["private_segment_fixed_size"] == 0, (name, fields)
        assert fields["vgpr_spill_count"] == 0 and fields["sgpr_spill_count"] == 0, (name, fields)
        start = text.index("\n" + name + ":")
        body = text[start:text.index(".end_amdhsa_kernel", start)]
        assert "scratch_" not in body and "global_atomic" not in body, name
        assert not re.search(r"v_fma\w*_f64|v_pk_fma", body) or "v_div_scale_f64" in body, name      # only inside the divisions
        m = re.search(r"(xs_roi|xs_sum|nps_radial)_kernelILi(\d+)E", name)
        seen.add((m.group(1), int(m.group(2))))
        R = int(m.group(2))
        if m.group(1) == "xs_roi":
            assert "global_load_dwordx4" in body and "v_mul_f32" in body and "v_add_f64" in body and "v_mul_f64" in body, name
            assert not re.search(r"v_(sin|cos)_f32", body) and "v_pk_fma_f32" not in body, name
            assert re.search(r"ds_read2?_b64", body) and re.search(r"ds_write2?_b64", body), name  # (re, im) move as one 8-byte word
            fused = re.findall(r"v_(?:fma|fmac|mad|mac)_f32\w*\s+[^\n]*", body)
            assert all(re.search(r",\s*(0x[0-9a-f]+|-?\d+(\.\d+)?)\b", f) for f in fused), (name, fused)
            plane = 2 * R * (R + 1) * 4
            assert plane <= fields["group_segment_fixed_size"] <= plane + 4 * 2 * R + 4 * 8 * R + 128, (name, fields)
            assert fields["group_segment_fixed_size"] <= 160 * 1024
            assert fields["vgpr_count"] + fields.get("agpr_count", 0) <= (256 if R == 128 else 512), (name, fields)
    assert seen == {(k, R) for k in ("xs_roi", "xs_sum", "nps_radial") for R in SIZES}
