"""CPU: the window of the 16-bit path without a GPU (include/midd.h: THE WINDOW) -- the numpy restatement (tests/window_reference.py)
against np.sort / np.percentile, the flat rule, the round trip over whole windows, the argument rules of the five C calls, the CLI and
service switches, and the host recipe on a 12-bit ramp.  Everything here is exact: there is no tolerance."""
import base64
import ctypes as C
import io
import os
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import window_reference as wr  # noqa: E402

PERCENTILES = [0, 0.5, 1, 33.3, 50, 99.5, 100]


def _images():
    rng = np.random.default_rng(21)
    return [rng.integers(0, 4096, (45, 59)).astype(np.uint16), rng.integers(0, 65536, (33, 7)).astype(np.uint16),
            np.array([[9, 9, 3, 9, 70, 9, 65535]], np.uint16), (rng.normal(2000, 300, (64, 64)).clip(0, 65535)).astype(np.uint16)]


def test_levels_are_the_order_statistic_of_np_sort():
    from midd_amd import image16
    for a in _images():
        s = np.sort(a.ravel())
        hist = wr.histogram(a)
        assert hist.dtype == np.uint32 and int(hist.sum()) == a.size
        for p in PERCENTILES:
            r = wr.rank(p, a.size)
            assert 0 <= r <= a.size - 1 and r == int(np.floor(p * (a.size - 1) / 100.0))
            want = int(s[r])
            for q in PERCENTILES:
                if p < q:
                    got = wr.levels(a, p, q)
                    raw = (want, int(s[wr.rank(q, a.size)]))
                    assert got == wr.flat_rule(*raw) and 0 <= got[0] < got[1] <= 65535
                    assert got[0] == want or raw[0] == raw[1] == 65535
                    assert wr.levels_from_histogram(hist, p, q) == got
                    assert image16.window_levels(a, (p, q)) == got
            try:
                lower = np.percentile(a, p, method="lower")
            except TypeError:                                           # an older numpy: np.sort alone is the reference
                continue
            assert int(lower) == want, (p, lower, want)
    assert wr.rank(0, 1) == 0 and wr.rank(100, 1) == 0 and wr.rank(100, 2 ** 32 - 1) == 2 ** 32 - 2


def test_flat_rule():
    from midd_amd import image16
    for v, want in ((0, (0, 1)), (1234, (1234, 1235)), (65535, (65534, 65535))):
        a = np.full((9, 5), v, np.uint16)
        for p in ((0, 100), (0.5, 99.5), (33.3, 33.4)):
            assert wr.levels(a, *p) == want
            assert wr.levels_from_histogram(wr.histogram(a), *p) == want
            assert image16.window_levels(a, p) == want
    a = np.array([[9, 9, 3, 9, 70, 9, 65535]], np.uint16)              # ranks 1 and 2 of 3 9 9 9 9 70 65535: both in bin 9
    assert (wr.rank(33.3, 7), wr.rank(33.4, 7)) == (1, 2)
    assert wr.levels(a, 33.3, 33.4) == (9, 10) == image16.window_levels(a, (33.3, 33.4))
    b = np.array([5] * 50 + [7] * 50, np.uint16)                       # two different ranks inside one bin
    assert wr.rank(10, 100) != wr.rank(20, 100) and wr.levels(b, 10, 20) == (5, 6) == image16.window_levels(b, (10, 20))


def _windows():
    rng = np.random.default_rng(5)
    fixed = [(0, 65535), (0, 1), (65534, 65535), (0, 4095)]
    for _ in range(404):
        lo = int(rng.integers(0, 65535))
        width = int(rng.integers(1, 65536 - lo)) if rng.random() < 0.5 else int(rng.integers(1, min(5000, 65536 - lo)))
        fixed.append((lo, lo + width))
    return fixed


def test_round_trip_is_the_identity_inside_every_window():
    from midd_amd import image16
    mismatches = 0
    for lo, hi in _windows():
        assert 0 <= lo < hi <= 65535
        v = np.arange(lo, hi + 1).astype(np.uint16)
        x = wr.load(v, lo, hi)
        assert x.dtype == np.float32 and x[0] == 0.0 and x[-1] == 1.0
        mismatches += int((wr.store(x, lo, hi) != v).sum())
        assert np.array_equal(image16.unit_float_window(v, (lo, hi)).view(np.uint32), x.view(np.uint32))
        assert np.array_equal(image16.to_u16_window(x, (lo, hi)), v)
    assert mismatches == 0


def test_values_outside_the_window_clip():
    from midd_amd import image16
    v = np.arange(65536).astype(np.uint16)
    for lo, hi in [(1000, 3000), (0, 1), (65534, 65535), (40000, 40001)]:
        back = wr.store(wr.load(v, lo, hi), lo, hi)
        assert np.array_equal(back, np.clip(v, lo, hi))
        assert np.array_equal(image16.to_u16_window(image16.unit_float_window(v, (lo, hi)), (lo, hi)), back)
    x = np.array([np.nan, -np.inf, np.inf, -0.5, 1.5, 0.5], np.float32)
    assert list(wr.store(x, 100, 300)) == [100, 100, 300, 100, 300, 200]
    assert list(image16.to_u16_window(x, (100, 300))) == [100, 100, 300, 100, 300, 200]


def test_window_0_65535_is_the_unwindowed_rule():
    from midd_amd import image16
    v = np.arange(65536).astype(np.uint16)
    f = image16.unit_float(v)
    assert np.array_equal(wr.load(v, 0, 65535).view(np.uint32), f.view(np.uint32))
    assert np.array_equal(image16.unit_float_window(v, (0, 65535)).view(np.uint32), f.view(np.uint32))
    x = np.concatenate([f, np.nextafter(f, np.float32(2)), np.nextafter(f, np.float32(-1)),
                        np.random.default_rng(2).uniform(-0.2, 1.2, 50000).astype(np.float32)])
    assert np.array_equal(wr.store(x, 0, 65535), image16.to_u16(x))
    assert np.array_equal(image16.to_u16_window(x, (0, 65535)), image16.to_u16(x))


# ------------------------------------------------------------------------------ C ABI without a GPU
def test_abi_argument_rules_before_any_gpu_work():
    from midd_amd import native
    lib = native.lib()
    buf = (C.c_char * 8192)()
    al = (C.addressof(buf) + 255) & ~255                               # host memory: every rule is judged before the GPU is touched
    p = C.c_void_p(al)

    def refused(rc, word):
        assert rc == -1 and word in lib.mi_last_error(), (rc, word, lib.mi_last_error())

    refused(lib.mi_histogram_u16(None, 1, 4, p, None), b"null")
    refused(lib.mi_histogram_u16(p, 1, 4, None, None), b"null")
    for n in (0, -1, 65536):
        refused(lib.mi_histogram_u16(p, n, 4, p, None), b"[1, 65535]")
        refused(lib.mi_window_levels(p, n, 0.5, 99.5, p, None), b"[1, 65535]")
        refused(lib.mi_window_u16_to_f32(p, p, n, 4, p, None), b"[1, 65535]")
        refused(lib.mi_window_f32_to_u16(p, p, n, 4, p, None), b"[1, 65535]")
    for count in (0, 1 << 32, 1 << 40):
        refused(lib.mi_histogram_u16(p, 1, count, p, None), b"[1, 2^32)")
        refused(lib.mi_window_u16_to_f32(p, p, 1, count, p, None), b"[1, 2^32)")
        refused(lib.mi_window_f32_to_u16(p, p, 1, count, p, None), b"[1, 2^32)")
    refused(lib.mi_histogram_u16(C.c_void_p(al + 1), 1, 4, p, None), b"2-byte")
    refused(lib.mi_histogram_u16(p, 1, 4, C.c_void_p(al + 4), None), b"16-byte")
    refused(lib.mi_window_levels(None, 1, 0.5, 99.5, p, None), b"null")
    refused(lib.mi_window_levels(p, 1, 0.5, 99.5, None, None), b"null")
    for lo, hi in [(-0.1, 50), (50, 100.1), (60, 40), (50, 50), (0, 0), (100, 100)]:
        refused(lib.mi_window_levels(p, 1, lo, hi, p, None), b"p_lo < p_hi")
    for lo, hi in [(float("nan"), 50), (1, float("nan")), (float("-inf"), 50), (1, float("inf"))]:
        refused(lib.mi_window_levels(p, 1, lo, hi, p, None), b"finite")
    for fn in (lib.mi_window_u16_to_f32, lib.mi_window_f32_to_u16):
        for args in ((None, p, 1, 4, p), (p, None, 1, 4, p), (p, p, 1, 4, None)):
            refused(fn(*args, None), b"null")
    U8, U16, F32 = native.MI_PIX_U8, native.MI_PIX_U16, native.MI_PIX_F32

    def call(src=p, st=U16, n=1, sw=4, sh=4, dst=p, dt=F32, dw=8, dh=8, lv=p, ws=p, nbytes=1 << 20):
        return lib.mi_resize_bicubic_f32_window(src, st, n, sw, sh, dst, dt, dw, dh, 0, lv, ws, nbytes, None)

    for kw, word in [(dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(ws=None), b"null"), (dict(n=0), b"positive"),
                     (dict(sw=0), b"positive"), (dict(st=3), b"source element type"), (dict(dt=U8), b"mi_resize_bicubic_u8"),
                     (dict(dt=7), b"destination element type"), (dict(n=4, sw=32768, sh=32768), b"2^31"),
                     (dict(ws=C.c_void_p(al + 64)), b"aligned"), (dict(nbytes=16), b"too small"),
                     (dict(n=65536, sw=1, sh=1, dw=2, dh=2, nbytes=1 << 40), b"[1, 65535]"),
                     (dict(st=F32, dt=F32), b"neither side"), (dict(st=U8, dt=F32), b"neither side"),
                     # levels == NULL is mi_resize_bicubic_f32 itself: its rules, in its words
                     (dict(lv=None, src=None), b"null"), (dict(lv=None, dt=U8), b"mi_resize_bicubic_u8"), (dict(lv=None, nbytes=16), b"too small")]:
        assert call(**kw) == -1, kw
        assert word in lib.mi_last_error(), (kw, lib.mi_last_error())


def test_python_wrappers_refuse_cpu_tensors_and_bad_types():
    from midd_amd import prepost
    img = torch.zeros((4, 4), dtype=torch.uint16)
    lv = torch.tensor([[0, 10]], dtype=torch.int32)
    with pytest.raises(RuntimeError):
        prepost.histogram_u16(img)                                      # CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        prepost.window_levels(img)
    with pytest.raises(RuntimeError):
        prepost.window_levels(torch.zeros((1, 65536), dtype=torch.uint32))
    with pytest.raises(RuntimeError):
        prepost.window_u16_to_float(img, lv)
    with pytest.raises(RuntimeError):
        prepost.window_to_u16(torch.zeros((4, 4)), lv)
    with pytest.raises(RuntimeError):
        prepost.resize_bicubic_f32(img, (8, 8), levels=lv)


# ------------------------------------------------------------------------------ CLI and service switches
def test_cli_parses_and_refuses_windows(monkeypatch, tmp_path, capsys):
    from midd_amd import cli
    seen = {}

    class _Img:
        def save(self, path, **kw):
            seen["saved"] = path

    def fake(*a, **kw):
        seen.clear()
        seen.update(kw)
        return _Img()

    monkeypatch.setattr(cli, "denoise_image_diffusion", fake)
    base = ["--image", "x.png", "--out", str(tmp_path / "o.png")]
    cli.main(base + ["--bit-depth", "16"])
    assert "window" not in seen and "window_levels" not in seen
    cli.main(base + ["--bit-depth", "16", "--window", "0.5,99.5"])
    assert seen["window"] == (0.5, 99.5) and "window_levels" not in seen and seen["bit_depth"] == 16
    cli.main(base + ["--bit-depth", "16", "--window-levels", "0,4095", "--tile", "32"])
    assert seen["window_levels"] == (0, 4095) and "window" not in seen and seen["tile"] == 32
    for bad in (["--window", "0,100"],                                                       # no --bit-depth 16
                ["--bit-depth", "8", "--window-levels", "0,4095"],
                ["--bit-depth", "16", "--window", "0,100", "--window-levels", "0,4095"],       # both spellings
                ["--bit-depth", "16", "--window", "99,1"],                                    # out of order
                ["--bit-depth", "16", "--window", "0,101"], ["--bit-depth", "16", "--window", "5"],
                ["--bit-depth", "16", "--window", "a,b"], ["--bit-depth", "16", "--window", "nan,50"],
                ["--bit-depth", "16", "--window-levels", "10,10"], ["--bit-depth", "16", "--window-levels", "0,65536"],
                ["--bit-depth", "16", "--window-levels", "1.5,9"]):
        with pytest.raises(SystemExit):
            cli.main(base + bad)
    assert "hi - lo grey levels" in " ".join(_help_text(cli, capsys).split())
    monkeypatch.undo()
    with pytest.raises(ValueError, match="--bit-depth 16"):
        cli.denoise_image_diffusion(None, "x.png", device_type="cpu", window=(0, 100))
    with pytest.raises(ValueError, match="cannot be combined"):
        cli.denoise_image_diffusion(None, "x.png", device_type="cpu", bit_depth=16, window=(0, 100), window_levels=(0, 9))
    with pytest.raises(ValueError, match="p_lo < p_hi"):
        cli.denoise_image_diffusion(None, "x.png", device_type="cpu", bit_depth=16, window=(60, 40))
    with pytest.raises(ValueError, match="lo < hi"):
        cli.denoise_image_diffusion(None, "x.png", device_type="cpu", bit_depth=16, window_levels=(9, 3))


def _help_text(cli, capsys):
    with pytest.raises(SystemExit):
        cli.main(["--help"])
    return capsys.readouterr().out


def test_service_window_switch(monkeypatch):
    from midd_amd.server import DiffusionService
    monkeypatch.delenv("MIDD_BIT_DEPTH", raising=False)
    monkeypatch.delenv("MIDD_WINDOW", raising=False)
    cpu = torch.device("cpu")
    assert DiffusionService(device=cpu).window is None and DiffusionService(device=cpu, bit_depth=16).window is None
    assert DiffusionService(device=cpu, bit_depth=16, window=(1, 99)).window == (1.0, 99.0)
    with pytest.raises(ValueError, match="bit_depth=16"):
        DiffusionService(device=cpu, window=(1, 99))
    with pytest.raises(ValueError, match="p_lo < p_hi"):
        DiffusionService(device=cpu, bit_depth=16, window=(99, 1))
    monkeypatch.setenv("MIDD_WINDOW", "0.5,99.5")
    with pytest.raises(ValueError, match="bit_depth=16"):
        DiffusionService(device=cpu)
    assert DiffusionService(device=cpu, bit_depth=16).window == (0.5, 99.5)
    assert DiffusionService(device=cpu, bit_depth=16, window=(0, 100)).window == (0.0, 100.0)
    monkeypatch.setenv("MIDD_BIT_DEPTH", "16")
    assert DiffusionService(device=cpu).window == (0.5, 99.5)
    monkeypatch.setenv("MIDD_WINDOW", "0.5;99.5")
    with pytest.raises(ValueError, match="MIDD_WINDOW"):
        DiffusionService(device=cpu)
    # with batch_slots > 0 and with update="ddim": only pre and post change
    monkeypatch.setenv("MIDD_WINDOW", "0,100")
    assert DiffusionService(device=cpu, batch_slots=2, session_factory=lambda s: None).window == (0.0, 100.0)
    assert DiffusionService(device=cpu, update="ddim", eta=0.5).window == (0.0, 100.0)


# ------------------------------------------------------------------------------ host recipe on a 12-bit file
def _png16(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr.astype(np.uint16)).save(buf, format="PNG")
    return buf.getvalue()


def _ramp12(h, w):
    return (np.arange(h * w, dtype=np.uint32) * 37 % 4096).astype(np.uint16).reshape(h, w)


def _stand_in_cli(monkeypatch, seen):
    from midd_amd import cli

    class _Denoiser:
        def __init__(self, model, noise_steps):
            pass

        def denoise(self, x, inference_steps):
            seen["x"] = x.clone()
            return x.clone()

        def denoise_tiled(self, x, inference_steps, tile, overlap, seed):
            seen["x"] = x.clone()
            return types.SimpleNamespace(image=x.clone(), origins_y=[0], origins_x=[0], seed=None)

    monkeypatch.setattr(cli, "DiffusionDenoiser", _Denoiser)
    monkeypatch.setattr(cli, "UNetDiffusion", lambda **kw: torch.nn.Identity())
    return cli


def test_cli_host_recipe_with_a_window_on_a_cpu_device(monkeypatch, tmp_path, capsys):
    """A 12-bit ramp in a 16-bit PNG, an identity sampler, no resize (--tile): with a window the sampler sees [0, 1] and the file
    comes back identical; without one it sees at most 4095 / 65535."""
    arr = _ramp12(40, 72)
    assert arr.min() == 0 and arr.max() == 4095
    path = tmp_path / "ramp12.png"
    path.write_bytes(_png16(arr))
    seen = {}
    cli = _stand_in_cli(monkeypatch, seen)
    kw = dict(device_type="cpu", inference_steps=3, variant="ddim", bit_depth=16, tile=32, overlap=8)
    out = cli.denoise_image_diffusion(None, str(path), window=(0, 100), **kw)
    assert out.mode == "I;16" and out.size == (72, 40)
    assert "Window: grey levels 0 .. 4095" in capsys.readouterr().out
    assert float(seen["x"].min()) == 0.0 and float(seen["x"].max()) == 1.0
    assert np.array_equal(seen["x"][0, 0].numpy().view(np.uint32), wr.load(arr, 0, 4095).view(np.uint32))
    assert np.array_equal(np.asarray(out), arr)                         # identical: every value lies inside the window
    unwindowed = cli.denoise_image_diffusion(None, str(path), **kw)
    assert float(seen["x"].max()) == np.float32(4095) / np.float32(65535) and np.array_equal(np.asarray(unwindowed), arr)
    # absolute levels narrower than the data: identical inside, clipped outside
    out = cli.denoise_image_diffusion(None, str(path), window_levels=(1000, 3000), **kw)
    assert np.array_equal(np.asarray(out), np.clip(arr, 1000, 3000))
    assert "Window: grey levels 1000 .. 3000" in capsys.readouterr().out
    # percentiles: the levels of the restatement
    lo, hi = wr.levels(arr, 10, 90)
    out = cli.denoise_image_diffusion(None, str(path), window=(10, 90), **kw)
    assert np.array_equal(np.asarray(out), np.clip(arr, lo, hi))


def test_cli_host_recipe_resizes_under_the_window(monkeypatch, tmp_path):
    from midd_amd import image16
    arr = _ramp12(48, 80)
    path = tmp_path / "ramp12.png"
    path.write_bytes(_png16(arr))
    seen = {}
    cli = _stand_in_cli(monkeypatch, seen)
    out = cli.denoise_image_diffusion(None, str(path), device_type="cpu", img_size=64, inference_steps=3, variant="ddim", bit_depth=16,
                                      window=(0.5, 99.5))
    lo, hi = wr.levels(arr, 0.5, 99.5)
    pre = image16.resize_f(wr.load(arr, lo, hi), (64, 64))
    assert np.array_equal(seen["x"][0, 0].numpy().view(np.uint32), pre.view(np.uint32))
    want = wr.store(image16.resize_f(pre, (48, 80)), lo, hi)
    assert out.mode == "I;16" and out.size == (80, 48) and np.array_equal(np.asarray(out), want)
    assert lo <= np.asarray(out).min() and np.asarray(out).max() <= hi


def test_an_8_bit_file_with_a_window_is_refused_with_its_mode(monkeypatch, tmp_path):
    from PIL import Image
    from midd_amd.server import DiffusionService, create_app
    a8 = np.random.default_rng(3).integers(0, 256, (40, 56), dtype=np.uint8)
    path = tmp_path / "in8.png"
    Image.fromarray(a8).save(path)
    cli = _stand_in_cli(monkeypatch, {})
    for kw in (dict(window=(0, 100)), dict(window_levels=(0, 255))):
        with pytest.raises(ValueError, match="mode 'L'"):
            cli.denoise_image_diffusion(None, str(path), device_type="cpu", img_size=64, inference_steps=3, variant="ddim", bit_depth=16, **kw)
    svc = DiffusionService(device=torch.device("cpu"), denoise_fn=lambda t: t, bit_depth=16, window=(0, 100))
    with pytest.raises(ValueError, match="mode 'L'"):
        svc.denoise_bytes(path.read_bytes())
    from fastapi.testclient import TestClient
    with TestClient(create_app(service=svc)) as client:
        assert client.get("/health").json()["window"] == [0.0, 100.0]
        r = client.post("/denoise", files={"file": ("x.png", path.read_bytes(), "image/png")})
        assert r.status_code == 400 and "mode 'L'" in r.json()["detail"]
        ok = client.post("/denoise", files={"file": ("x.png", _png16(_ramp12(40, 56)), "image/png")})
        assert ok.status_code == 200 and ok.json()["diffusion"] is not None
    plain = DiffusionService(device=torch.device("cpu"), denoise_fn=lambda t: t, bit_depth=16)
    with TestClient(create_app(service=plain)) as client:
        assert client.get("/health").json()["window"] is None
        assert client.post("/denoise", files={"file": ("x.png", path.read_bytes(), "image/png")}).status_code == 200


def test_service_process_path_with_a_window_and_a_stand_in_sampler():
    """The window is per request: two uploads with different ranges each come back at their own levels."""
    from PIL import Image
    from midd_amd import image16
    from midd_amd.server import SERVE_SIZE, DiffusionService
    svc = DiffusionService(device=torch.device("cpu"), denoise_fn=lambda t: t.clone(), bit_depth=16, window=(0, 100))
    for offset, span in ((0, 4096), (20000, 1024)):
        arr = (offset + _ramp12(44, 60) % span).astype(np.uint16)
        img = Image.open(io.BytesIO(base64.b64decode(svc.denoise_bytes(_png16(arr))["diffusion"])))
        assert img.mode == "I;16" and img.size == (60, 44)
        lo, hi = int(arr.min()), int(arr.max())
        x, size = svc.preprocess(_png16(arr))
        assert size == (60, 44, (lo, hi)) and float(x.min()) == 0.0 and float(x.max()) <= 1.0
        pre = image16.resize_f(wr.load(arr, lo, hi), SERVE_SIZE)
        assert np.array_equal(x[0, 0].numpy().view(np.uint32), pre.view(np.uint32))
        got = np.asarray(img)
        assert np.array_equal(got, wr.store(image16.resize_f(pre, (44, 60)), lo, hi))
        assert lo <= got.min() and got.max() <= hi
