"""CPU-only checks of the noise power spectrum (include/midd.h: THE NOISE POWER SPECTRUM, mi_noise_power_spectrum): the numpy
restatement (tests/nps_reference.py) against float64 numpy.fft within the bound derived from Higham's Theorem 24.2, a known answer
that involves no FFT library, Parseval, the integer radial rule, the argument rules of the C ABI through the library loaded without
a device, the Python and CLI argument rules, and the ISA metadata of the new kernels.  What the device computes is judged in
test_gpu_nps.py."""
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
from tests import nps_reference as ref
from tests.isa_dump import isa_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_noise_power_spectrum", "mi_noise_power_spectrum_workspace_bytes"}
SIZES = (32, 64, 128)


# ------------------------------------------------------------------------------ 1. the restatement against float64 numpy.fft
def _nps64(a, b, R, S, detrend, window):
    """float64 fft2 of the SAME detrended and windowed ROIs, averaged: [B, C, R, R]."""
    f = a if b is None else a - b[:, None]
    sw = float(R * R) if window is None else float((window.astype(np.float64) ** 2).sum() ** 2)
    out = np.empty((a.shape[0], a.shape[2], R, R))
    for bi in range(a.shape[0]):
        for c in range(a.shape[2]):
            d = ref.detrend_window(ref.cut_rois(f[bi, :, c], R, S), detrend, window)
            out[bi, c] = (np.abs(np.fft.fft2(d.astype(np.float64))) ** 2).mean(axis=0) / sw
    return out


def test_the_bound_is_the_derived_one():
    """2 rho + rho^2 recomputed from u = 2^-24: 8.3e-6, 9.9e-6 and 1.15e-5."""
    for R, want in ((32, 8.3e-6), (64, 9.9e-6), (128, 1.15e-5)):
        assert abs(ref.error_bound(R) - want) < 0.05e-6 * 10, (R, ref.error_bound(R))
    assert ref.error_bound(32) < ref.error_bound(64) < ref.error_bound(128)


@pytest.mark.parametrize("R", SIZES)
@pytest.mark.parametrize("ramp,detrend,windowed,with_b", [(0.0, "mean", False, False), (0.3, "mean", True, True), (0.3, "plane", True, False),
                                                         (0.0, "none", False, True)])
def test_restatement_against_float64_fft2(R, ramp, detrend, windowed, with_b):
    """sum|nps - nps64| / sum nps64 <= 2 rho + rho^2 on Philox noise, with and without a ramp."""
    H, W = R + R // 2 + 3, 2 * R + 5
    a = ref.philox_field((1, 2, 1, H, W), seed=R + 1, ramp=ramp)
    b = ref.philox_field((1, 1, H, W), seed=R + 2) if with_b else None
    w = ref.hann(R) if windowed else None
    got = ref.noise_power_spectrum(a, b, R, R // 2, detrend, w)
    want = _nps64(a, b, R, R // 2, detrend, w)
    err = np.abs(got.nps - want).sum() / want.sum()
    print(f"R={R} ramp={ramp} detrend={detrend} window={windowed} b={with_b}: relative L1 error {err:.3e}, bound {ref.error_bound(R):.3e}")
    assert err <= ref.error_bound(R)
    assert err > 0 or detrend == "none"                       # fp32 arithmetic, not a float64 transform in disguise
    assert got.rois_used[0, 0] == 2 * 2 * 3 and got.rois_skipped[0, 0] == 0


def test_white_noise_is_flat_at_its_variance():
    """The normalisation: sigma^2 = 0.0025 at unit pitch, with and without the window (the mean over the plane within 5 %: 48 ROIs)."""
    a = ref.philox_field((1, 3, 1, 96, 96), seed=5)
    for w in (None, ref.hann(32)):
        got = ref.noise_power_spectrum(a, None, 32, 16, "mean", w)
        assert abs(got.nps[0, 0][1:, 1:].mean() / 0.0025 - 1) < 0.05


# ------------------------------------------------------------------------------ 2. a known answer, no FFT library
@pytest.mark.parametrize("R,u0,v0", [(32, 3, 5), (64, 7, 0), (128, 1, 60), (32, 0, 9)])
def test_a_plane_wave_lands_in_its_two_bins(R, u0, v0):
    A = 0.75
    y, x = np.mgrid[0:2 * R, 0:3 * R]
    f = (A * np.cos(2 * np.pi * (u0 * x + v0 * y) / R)).astype(np.float32)
    got = ref.noise_power_spectrum(f[None, None, None], None, R, R, "none", None).nps[0, 0]
    assert got.shape == (R, R)
    peak = A * A * R * R / 4
    bound = ref.error_bound(R)
    # the cosine itself is rounded to fp32 (relative 2^-24 of A per sample: an L2 share of u, inside the 3u of rho)
    for v, u in ((v0, u0), ((R - v0) % R, (R - u0) % R)):
        assert abs(got[v, u] - peak) <= bound * peak, (v, u, got[v, u], peak)
    rest = got.sum() - got[v0, u0] - got[(R - v0) % R, (R - u0) % R]
    assert 0 <= rest <= bound * A * A * R * R / 2, rest


# ------------------------------------------------------------------------------ 3. Parseval
@pytest.mark.parametrize("R", SIZES)
def test_parseval(R):
    a = ref.philox_field((1, 2, 1, R + 7, 2 * R), seed=40 + R, ramp=0.2)
    w = ref.hann(R)
    got = ref.noise_power_spectrum(a, None, R, R // 2, "plane", w)
    d = ref.detrend_window(ref.cut_rois(a[0, :, 0], R, R // 2), "plane", w).astype(np.float64)
    sw = float((w.astype(np.float64) ** 2).sum() ** 2)
    want = (d ** 2).sum(axis=(1, 2)).mean() / sw
    have = got.nps[0, 0].sum() / (R * R)
    print(f"R={R}: Parseval {have!r} vs {want!r}, relative {abs(have - want) / want:.3e}")
    assert abs(have - want) <= ref.error_bound(R) * want


# ------------------------------------------------------------------------------ 4. the radial bins
@pytest.mark.parametrize("R", SIZES)
def test_radial_bins_are_the_rounded_radius_in_integers(R):
    bins, fr = ref.radial_bins(R)
    for v in range(R):
        for u in range(R):
            d2 = int(fr[u]) ** 2 + int(fr[v]) ** 2
            r = math.isqrt(d2)                                  # floor(sqrt(d2) + 1/2) exactly: r or r + 1
            r += 4 * d2 >= (2 * r + 1) ** 2
            assert bins[v, u] == r, (v, u)
    nps = np.arange(R * R, dtype=np.float64).reshape(R, R)
    radial, count = ref.radial_profile(nps, False)
    assert count.sum() == (bins <= R // 2).sum() and count[0] == 1 and radial[0] == 0.0
    assert not np.isnan(radial).any()
    for r in (1, R // 4, R // 2):
        assert radial[r] == nps[bins == r].sum() / count[r]     # integers below 2^53: any order
    radial_x, count_x = ref.radial_profile(nps, True)
    on_axes = (fr[None, :] == 0) | (fr[:, None] == 0)
    assert count_x.sum() == ((bins <= R // 2) & ~on_axes).sum()
    assert count_x[0] == 0 and np.isnan(radial_x[0]) and count[1] == 8 and count_x[1] == 4      # bin 1: (+-1, 0), (0, +-1) and (+-1, +-1)
    assert radial_x[1] == (nps[1, 1] + nps[1, R - 1] + nps[R - 1, 1] + nps[R - 1, R - 1]) / 4


def test_the_summation_order_is_the_specified_one():
    """Chunks of 16 ROIs: P = x^2 >= 2^53 in ROI 0 (a multiple of 64, spacing 2: adding 1 is a tie that falls back to even), P = 1 in
    the 32 ROIs after it.  Chunk 0 loses its fifteen ones one by one, chunk 1 arrives as 16 at once, chunk 2's single 1 is lost."""
    R = 32
    x = np.float32(2.0 ** 26.5)
    while float(x) ** 2 < 2.0 ** 53:
        x = np.nextafter(x, np.float32(np.inf))
    a = np.zeros((1, 33, 1, R, R), np.float32)
    a[0, 0, 0, 0, 0] = x                                        # an impulse: P = x^2 at every frequency
    a[0, 1:, 0, 0, 0] = 1.0                                     # P = 1 at every frequency
    got = ref.noise_power_spectrum(a, None, R, R, "none", None).nps[0, 0]
    big = float(x) ** 2
    assert 2.0 ** 53 <= big < 2.0 ** 54 and big + 1.0 == big and np.all(got == got[0, 0])
    assert got[0, 0] == (1.0 * (big + 16.0)) / (33.0 * 1024.0) != (1.0 * (big + 32.0)) / (33.0 * 1024.0)


# ------------------------------------------------------------------------------ 5. the C ABI: every rule before anything is read
A_, B_, NPS, RAD, CNT, USED, SKIP, WS = (0x10000000 * (i + 1) for i in range(8))      # non-null "device pointers"


def _call(**kw):
    """mi_noise_power_spectrum with fake pointers: every call here must fail before anything reads them."""
    a = dict(a=A_, b=B_, B=2, K=3, C=1, H=70, W=83, roi=32, step=16, detrend=2, window=None, scale=1.0, flags=0, nps=NPS, radial=RAD,
             radial_count=CNT, rois_used=USED, rois_skipped=SKIP, workspace=WS, workspace_bytes=None)
    a.update(kw)
    lib = native.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = 2 * 3 * (32 * 17 + 1) * 8
    w = a["window"]
    if isinstance(w, (list, tuple)):
        w = (C.c_float * len(w))(*w)
    elif isinstance(w, int):
        w = C.cast(w, C.POINTER(C.c_float))
    rc = lib.mi_noise_power_spectrum(a["a"], a["b"], a["B"], a["K"], a["C"], a["H"], a["W"], a["roi"], a["step"], a["detrend"], w, a["scale"],
                                     a["flags"], a["nps"], a["radial"], a["radial_count"], a["rois_used"], a["rois_skipped"], a["workspace"],
                                     a["workspace_bytes"], None)
    return rc, lib.mi_last_error().decode()


FAKE_WINDOW = 0x90000000          # never read: every rule below is judged before the window
RULES = [
    (dict(roi=48), ["roi 48 outside {32, 64, 128}"]),
    (dict(step=0), ["step 0 below 1"]),
    (dict(K=0), ["K 0", "at least 1"]),
    (dict(B=65536), ["65536 groups outside [1, 65535]"]),
    (dict(H=31), ["image 31 x 83 smaller than the ROI 32 x 32"]),
    (dict(detrend=3), ["detrend 3 outside"]),
    (dict(flags=2), ["flags 0x2", "unknown bits"]),
    (dict(scale=float("inf")), ["scale", "not finite"]),
    (dict(nps=None), ["null argument"]),
    (dict(radial=RAD + 4), ["8-byte aligned"]),
    (dict(workspace_bytes=2 * 3 * (32 * 17 + 1) * 8 - 1), ["workspace too small", str(2 * 3 * (32 * 17 + 1) * 8)]),
    (dict(rois_used=NPS + 8), ["nps and rois_used alias"]),
]


@pytest.mark.parametrize("first", range(len(RULES)))
def test_every_argument_rule_in_its_place(first):
    """Rule `first` alone, and rule `first` with every later rule broken as well: its message either way, and the (fake) window,
    the last thing the call looks at, is never read."""
    for broken in (RULES[first:first + 1], RULES[first:]):
        kw = dict(window=FAKE_WINDOW)
        for change, _ in reversed(broken):
            kw.update(change)
        rc, msg = _call(**kw)
        assert rc == -1, (kw, rc, msg)
        for word in RULES[first][1]:
            assert word in msg, (kw, msg)


def test_further_argument_rules_and_the_workspace_query():
    lib = native.lib()
    for kw, word in [(dict(roi=0), "roi 0 outside"), (dict(roi=256), "roi 256 outside"), (dict(step=-3), "step -3 below 1"), (dict(B=0), "B 0"),
                     (dict(C=0), "C 0"), (dict(W=31), "smaller than the ROI"), (dict(H=127, roi=128), "smaller than the ROI"),
                     (dict(detrend=-1), "detrend -1"), (dict(flags=-1), "unknown bits"), (dict(scale=float("nan")), "not finite"),
                     (dict(a=None), "null"), (dict(radial=None), "null"), (dict(radial_count=None), "null"), (dict(rois_used=None), "null"),
                     (dict(rois_skipped=None), "null"), (dict(workspace=None), "null"), (dict(nps=NPS + 4), "8-byte"),
                     (dict(radial_count=CNT + 2), "8-byte"), (dict(rois_skipped=SKIP + 1), "8-byte"), (dict(workspace=WS + 4), "8-byte"),
                     (dict(a=A_ + 2), "4-byte"), (dict(b=B_ + 1), "4-byte"), (dict(workspace_bytes=0), "too small"),
                     (dict(b=A_ + 4 * 70 * 83), "a and b alias"), (dict(nps=A_ + 8), "a and nps alias"), (dict(workspace=B_ + 8), "b and workspace alias"),
                     (dict(radial=NPS + 2 * 32 * 32 * 8 - 8), "nps and radial alias"), (dict(rois_skipped=USED + 8), "rois_used and rois_skipped alias"),
                     (dict(window=[0.5] * 31 + [float("nan")]), "window[31] is not finite")]:
        rc, msg = _call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    ws = lib.mi_noise_power_spectrum_workspace_bytes
    half = {32: 32 * 17 + 1, 64: 64 * 33 + 1, 128: 128 * 65 + 1}
    assert ws(1, 1, 1, 32, 32, 32, 16) == half[32] * 8                       # one ROI: one chunk
    assert ws(1, 4, 1, 48, 48, 32, 16) == half[32] * 8                       # 16 ROIs: one chunk
    assert ws(1, 1, 1, 32, 288, 32, 16) == 2 * half[32] * 8                  # 17 ROIs: two chunks
    assert ws(2, 3, 2, 70, 83, 32, 16) == 4 * 3 * half[32] * 8               # 36 ROIs per group: three chunks
    assert ws(1, 8, 1, 2500, 2048, 64, 32) == ((8 * 77 * 63 + 15) // 16) * half[64] * 8
    assert ws(1, 2, 1, 128, 200, 128, 64) == half[128] * 8
    for bad in [(0, 1, 1, 64, 64, 32, 16), (1, 1, 1, 64, 64, 33, 16), (1, 1, 1, 64, 64, 32, 0), (1, 1, 1, 31, 64, 32, 16), (256, 1, 256, 64, 64, 32, 16)]:
        assert ws(*bad) == 0 and lib.mi_last_error(), bad


# ------------------------------------------------------------------------------ 6. header and bindings
def test_header_and_binding_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in native.SYMBOLS}
    assert NEW <= declared and declared == bound
    for name in NEW:
        assert getattr(native.lib(), name) is not None
    for words in ("THE NOISE POWER SPECTRUM", "tr = wr*X.re - wi*X.im;   ti = wr*X.im + wi*X.re", "chunks of 16", "[bitrev(y)][bitrev(x)]",
                  "P[v][u] = P[(R-v) % R][R-u]", "(2r-1)^2 <= 4*d2 < (2r+1)^2", "nps[g][v][u] = (scale * sum) / ((double)rois_used[g] * S_w)",
                  "d = (float)((double)f - ((m + ax*xc) + ay*yc))", "MI_NPS_EXCLUDE_AXES", "0x7FF8000000000000"):
        assert words in header, words
    assert ref.CHUNK == 16


# ------------------------------------------------------------------------------ 7. the Python and CLI argument rules
def test_python_surface_without_a_gpu():
    assert midd_amd.NoisePowerSpectrum._fields == ("nps", "radial", "radial_count", "freqs", "rois_used", "rois_skipped", "roi", "step")
    sig = inspect.signature(midd_amd.noise_power_spectrum).parameters
    assert list(sig) == ["a", "b", "roi", "step", "detrend", "window", "scale", "exclude_axes"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, 64, None, "plane", "hann", 1.0, False]
    sig = inspect.signature(DiffusionDenoiser.ensemble_nps).parameters
    assert list(sig)[:4] == ["self", "noisy", "inference_steps", "members"] and {"seed", "tile", "overlap", "roi", "step", "detrend", "window"} <= set(sig)
    assert (sig["members"].default, sig["seed"].default, sig["tile"].default, sig["overlap"].default, sig["roi"].default) == (8, None, None, 32, 64)
    x = torch.zeros(1, 2, 1, 64, 64)
    for kw, word in [(dict(roi=48), "roi must be one of"), (dict(roi=True), "roi must be one of"), (dict(step=0), "step must be"),
                     (dict(detrend="linear"), "detrend must be"), (dict(window="hamming"), "window must be"), (dict(window=[1.0] * 63), "window must be"),
                     (dict(scale=float("nan")), "scale must be finite"), (dict(roi=128), "smaller than the ROI"),
                     (dict(b=torch.zeros(1, 2, 1, 64, 64)), "b must be a tensor of shape (1, 1, 64, 64)")]:
        with pytest.raises(ValueError, match=re.escape(word)):
            midd_amd.noise_power_spectrum(x, **kw)
    with pytest.raises(ValueError, match="a must be"):
        midd_amd.noise_power_spectrum(torch.zeros(3, 64, 64))
    for arg in (x, x[:, 0], x[0, 0, 0]):                      # valid arguments, CPU tensors: never a silent fall-back
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            midd_amd.noise_power_spectrum(arg)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.noise_power_spectrum(x, torch.zeros(1, 1, 64, 64), window=None, detrend="none")
    # the Hann table is the restatement's, bit for bit; the result's own arithmetic
    for R in SIZES:
        assert np.array_equal(midd_amd.nps_window("hann", R).numpy().view(np.uint32), ref.hann(R).view(np.uint32))
    sp = midd_amd.NoisePowerSpectrum(torch.full((1, 1, 32, 32), 0.5, dtype=torch.float64), None, None, None, None, None, 32, 16)
    assert sp.variance().tolist() == [[0.5]]
    # ensemble_nps: its own rules, then those of the calls it composes
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    img = torch.zeros(1, 1, 64, 64)
    with pytest.raises(ValueError, match="members >= 2"):
        d.ensemble_nps(img, inference_steps=2, members=1, seed=1)
    with pytest.raises(ValueError, match="roi must be one of"):
        d.ensemble_nps(img, inference_steps=2, members=3, seed=1, roi=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.ensemble_nps(img, inference_steps=2, members=3, seed=1, roi=32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.ensemble_nps(img, inference_steps=2, members=3, seed=1, roi=32, tile=32, overlap=8)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="deterministic sampler has no ensemble"):
        ddim.ensemble_nps(img, inference_steps=2, members=3, seed=1, roi=32)


def test_cli_refusals(capsys, tmp_path):
    from PIL import Image

    from midd_amd import cli
    sig = inspect.signature(cli.denoise_image_diffusion).parameters
    assert sig["nps_out"].default is None and sig["nps_roi"].default is None and sig["nps_step"].default is None
    base = ["--image", "nowhere.png"]
    for argv, word in [(["--nps-roi", "32"], "--nps-out PATH.json"), (["--nps-step", "8"], "--nps-out PATH.json"),
                       (["--nps-out", "n.json", "--nps-roi", "48"], "--nps-roi needs one of"),
                       (["--nps-out", "n.json", "--nps-step", "0"], "--nps-step needs S >= 1"),
                       (["--nps-out", "n.json", "--img-size", "48"], "smaller than the ROI"),
                       (["--nps-out", "n.json", "--img-size", "64", "--nps-roi", "128"], "smaller than the ROI")]:
        with pytest.raises(SystemExit):
            cli.main(argv + base)
        assert word in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="need --nps-out"):
        cli.denoise_image_diffusion(None, "nowhere.png", nps_roi=32)
    with pytest.raises(ValueError, match="roi must be one of"):
        cli.denoise_image_diffusion(None, "nowhere.png", nps_out="n.json", nps_roi=48)
    with pytest.raises(ValueError, match="smaller than the ROI"):
        cli.denoise_image_diffusion(None, "nowhere.png", nps_out="n.json", img_size=32)
    with pytest.raises(RuntimeError, match="only on a ROCm GPU"):
        cli.denoise_image_diffusion(None, "nowhere.png", device_type="cpu", nps_out="n.json")
    small = tmp_path / "small.png"                              # with --tile the image's own size counts
    Image.fromarray(np.zeros((48, 40), np.uint8)).save(small)
    with pytest.raises(ValueError, match=r"the image \(48x40\) is smaller than the ROI \(64x64\)"):
        cli.denoise_image_diffusion(None, str(small), tile=32, overlap=8, nps_out="n.json")


# ------------------------------------------------------------------------------ 8. static: the kernels' ISA
def _metadata(text):
    notes = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - ", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_no_nps_kernel_touches_scratch():
    """Every instantiation (R in {32, 64, 128} of the three kernels) has a private segment of 0 bytes and no spilled VGPR; the
    butterflies are plain fp32 multiplications and additions (no fused multiply-add but inside the integer division of the chunk's
    first ROI index), the sums plain double adds; no atomics on global memory; the ROI kernel reads 16-byte words; its LDS is the two
    padded planes."""
    text = isa_dump("nps.hip")
    meta = _metadata(text)
    seen = set()
    for name, fields in meta.items():
        assert "nps_" in name, name
        assert fields["private_segment_fixed_size"] == 0, (name, fields)
        assert fields["vgpr_spill_count"] == 0, (name, fields)
        start = text.index("\n" + name + ":")
        body = text[start:text.index(".end_amdhsa_kernel", start)]
        assert "scratch_" not in body and "global_atomic" not in body, name
        assert not re.search(r"v_fma\w*_f64|v_pk_fma", body) or "v_div_scale_f64" in body, name      # only inside the divisions
        m = re.search(r"nps_(roi|sum|radial)_kernelILi(\d+)E", name)
        seen.add((m.group(1), int(m.group(2))))
        R = int(m.group(2))
        if m.group(1) == "roi":
            assert "global_load_dwordx4" in body and "v_mul_f32" in body and "v_add_f64" in body and "v_mul_f64" in body, name
            assert not re.search(r"v_(sin|cos)_f32", body) and "v_pk_fma_f32" not in body, name     # twiddles come from the table
            assert re.search(r"ds_read2?_b64", body) and re.search(r"ds_write2?_b64", body), name  # (re, im) move as one 8-byte word
            fused = re.findall(r"v_(?:fma|fmac|mad|mac)_f32\w*\s+[^\n]*", body)
            # (the fused steps of the 64-bit integer division each carry a literal; a fused butterfly would be all registers)
            assert all(re.search(r",\s*(0x[0-9a-f]+|-?\d+(\.\d+)?)\b", f) for f in fused), (name, fused)
            planes = 2 * R * (R + 1) * 4
            assert planes <= fields["group_segment_fixed_size"] <= planes + 4 * 2 * R + 2 * 8 * R + 64, (name, fields)
            assert fields["group_segment_fixed_size"] <= 160 * 1024
        else:      # the sum launch has no LDS, the radial launch holds the group's plane
            assert fields["group_segment_fixed_size"] == (8 * R * R if m.group(1) == "radial" else 0), name
    assert seen == {(k, R) for k in ("roi", "sum", "radial") for R in SIZES}
