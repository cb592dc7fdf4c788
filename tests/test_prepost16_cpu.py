"""CPU: the 16-bit image path without a GPU -- the numpy restatement (tests/resize_f32_reference.py) pinned against Pillow's mode "F"
resample bit for bit, the u16 element rule, the argument rules of the four C calls, the CLI / service switches and the host recipe
on a 16-bit PNG.  Everything here is bit-for-bit: there is no tolerance."""
import base64
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import resize_f32_reference as rr  # noqa: E402

# (source (h, w), destination (h, w)): up, down, mixed, one axis kept, a one-pixel axis, 51 taps
SHAPES = [((37, 53), (48, 64)), ((64, 48), (24, 40)), ((50, 50), (128, 128)), ((97, 31), (40, 24)), ((33, 40), (33, 64)),
          ((1, 7), (5, 9)), ((97, 31), (8, 24))]


def _uniform(h, w, seed):
    return np.random.default_rng(seed).random((h, w), dtype=np.float32)


def _blocks(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx // 3 + yy // 3) % 2).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_is_pillow_mode_f_bit_for_bit(shape):
    Image = pytest.importorskip("PIL.Image")
    (h, w), (oh, ow) = shape
    for name, img in (("uniform", _uniform(h, w, h * 131 + w)), ("blocks", _blocks(h, w))):
        ref = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BICUBIC))
        got = rr.resize_bicubic_f32(img, oh, ow)
        assert ref.dtype == np.float32 and got.shape == ref.shape == (oh, ow)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), f"{name}: {np.abs(got - ref).max()}"


def test_the_unclipped_resample_leaves_the_unit_interval():
    """Otherwise the clamp cases show nothing: the 0/1 block pattern overshoots on both sides."""
    for (h, w), (oh, ow) in SHAPES[:4]:
        out = rr.resize_bicubic_f32(_blocks(h, w), oh, ow)
        assert out.min() < 0.0 and out.max() > 1.0, ((h, w), out.min(), out.max())
        clipped = rr.resize(_blocks(h, w), oh, ow, rr.F32, True)
        assert clipped.min() == 0.0 and clipped.max() == 1.0
        assert np.array_equal(clipped, np.clip(out, 0, 1))


def test_coefficients_are_normalised_and_bounds_stay_inside():
    for in_size, out_size in [(53, 64), (97, 8), (31, 24), (7, 9), (1, 5)]:
        bounds, kk, ksize = rr.coeffs(in_size, out_size)
        assert kk.shape == (out_size, ksize) and kk.dtype == np.float64
        assert np.all(np.abs(kk.sum(axis=1) - 1.0) < 1e-14)
        assert np.all(bounds[:, 0] >= 0) and np.all(bounds[:, 1] >= 1) and np.all(bounds[:, 0] + bounds[:, 1] <= in_size)
        assert np.all(bounds[:, 1] <= ksize)
    assert rr.coeffs(97, 8)[1].shape[1] == 51


def test_u16_round_trip_is_the_identity_for_all_65536_values():
    v = np.arange(65536, dtype=np.uint16)
    f = rr.load(v)
    assert f.dtype == np.float32 and f[0] == 0.0 and f[-1] == 1.0
    np.testing.assert_array_equal(rr.to_u16(f), v)
    from midd_amd import image16
    np.testing.assert_array_equal(image16.unit_float(v), f)
    np.testing.assert_array_equal(image16.to_u16(f), v)


def _u16_rule_in_doubles(v) -> int:
    """The store rule in Python doubles: a product of two float32 values and a sum with .5 are exact in a double, so rounding each to
    float32 once is the fp32 multiply and the fp32 add."""
    v = min(max(float(v), 0.0), 1.0)
    t = float(np.float32(v * 65535.0))
    return int(float(np.float32(t + 0.5)))


def test_u16_rule_rounds_to_nearest_and_clamps():
    h = np.float32(0.5)                                                # 0.5 * 65535 = 32767.5: a .5 boundary, exact in fp32
    x = np.array([-0.1, 1.1, 0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)),
                  np.nextafter(h, np.float32(0)), h, np.nextafter(h, np.float32(1))], np.float32)
    got = rr.to_u16(x)
    assert got.dtype == np.uint16
    assert list(got) == [0, 65535, 0, 65535, 65535, 32767, 32768, 32768]          # the boundary rounds up, the float below it down
    assert list(got) == [_u16_rule_in_doubles(v) for v in x]
    rng = np.random.default_rng(1)
    r = rng.uniform(-0.2, 1.2, 20000).astype(np.float32)
    np.testing.assert_array_equal(rr.to_u16(r), np.array([_u16_rule_in_doubles(v) for v in r], np.uint16))
    assert np.all(np.abs(rr.to_u16(r).astype(np.float64) - np.clip(r.astype(np.float64), 0, 1) * 65535.0) <= 0.5 + 2.0 ** -8)
    from midd_amd import image16
    np.testing.assert_array_equal(image16.to_u16(x), got)
    np.testing.assert_array_equal(image16.to_u16(r), rr.to_u16(r))


# ------------------------------------------------------------------------------ C ABI without a GPU
def test_abi_argument_rules_before_any_gpu_work():
    from midd_amd import native
    lib = native.lib()
    ws_bytes = lib.mi_resize_f32_workspace_bytes
    assert ws_bytes(1, 400, 300, 512, 512) > 300 * 512 * 4
    for bad in [(0, 4, 4, 8, 8), (1, 0, 4, 8, 8), (1, 4, -1, 8, 8), (1, 4, 4, 0, 8), (1, 4, 4, 8, 0), (4, 32768, 32768, 8, 8)]:
        assert ws_bytes(*bad) == 0, bad
    buf = (C.c_char * 8192)()
    al = (C.addressof(buf) + 255) & ~255                               # host memory: every rule is judged before the GPU is touched
    p = C.c_void_p(al)
    U8, U16, F32 = native.MI_PIX_U8, native.MI_PIX_U16, native.MI_PIX_F32

    def call(src=p, st=U16, n=1, sw=4, sh=4, dst=p, dt=F32, dw=8, dh=8, ws=p, nbytes=1 << 20):
        return lib.mi_resize_bicubic_f32(src, st, n, sw, sh, dst, dt, dw, dh, 0, ws, nbytes, None)

    for kw, word in [(dict(src=None), b"null"), (dict(dst=None), b"null"), (dict(ws=None), b"null"),
                     (dict(n=0), b"positive"), (dict(sw=0), b"positive"), (dict(dh=-3), b"positive"),
                     (dict(st=3), b"source element type"), (dict(st=-1), b"source element type"),
                     (dict(dt=U8), b"mi_resize_bicubic_u8"), (dict(dt=7), b"destination element type"),
                     (dict(n=4, sw=32768, sh=32768), b"2^31"),
                     (dict(ws=C.c_void_p(al + 64)), b"aligned"), (dict(nbytes=16), b"too small")]:
        assert call(**kw) == -1, kw
        assert word in lib.mi_last_error(), (kw, lib.mi_last_error())
    for fn in (lib.mi_u16_to_unit_f32, lib.mi_unit_f32_to_u16):
        assert fn(None, p, 4, None) == -1 and b"null" in lib.mi_last_error()
        assert fn(p, None, 4, None) == -1 and b"null" in lib.mi_last_error()
    assert F32 == 2 and U16 == 1 and U8 == 0
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    for name, val in (("MI_PIX_U8", 0), ("MI_PIX_U16", 1), ("MI_PIX_F32", 2)):
        assert f"#define {name}" in header and int(header.split(f"#define {name}")[1].split()[0]) == val


def test_python_wrappers_refuse_cpu_tensors_and_bad_types():
    from midd_amd import prepost
    with pytest.raises(RuntimeError):
        prepost.resize_bicubic_f32(torch.zeros((4, 4)), (8, 8))                               # CPU tensor: no fallback
    with pytest.raises(TypeError):
        prepost.resize_bicubic_f32(torch.zeros((4, 4), dtype=torch.float64), (8, 8))
    with pytest.raises(ValueError):
        prepost.resize_bicubic_f32(torch.zeros((4, 4)), (8, 8), out_dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        prepost.to_u16(torch.zeros(4))
    with pytest.raises(RuntimeError):
        prepost.u16_to_unit_float(torch.zeros(4, dtype=torch.uint16))


# ------------------------------------------------------------------------------ CLI and service switches
def test_cli_parses_bit_depth(monkeypatch, tmp_path):
    from midd_amd import cli
    seen = {}

    class _Img:
        def save(self, path, **kw):
            seen["saved"] = path

    def fake(*a, **kw):
        seen.update(kw)
        return _Img()

    monkeypatch.setattr(cli, "denoise_image_diffusion", fake)
    cli.main(["--image", "x.png", "--out", str(tmp_path / "o.png")])
    assert seen["bit_depth"] == 8
    cli.main(["--image", "x.png", "--out", str(tmp_path / "o.png"), "--bit-depth", "16", "--tile", "32"])
    assert seen["bit_depth"] == 16 and seen["tile"] == 32
    with pytest.raises(SystemExit):
        cli.main(["--image", "x.png", "--bit-depth", "12"])
    monkeypatch.undo()
    with pytest.raises(ValueError, match="bit_depth"):
        cli.denoise_image_diffusion(None, "x.png", device_type="cpu", bit_depth=12)


def test_service_bit_depth_switch(monkeypatch):
    from midd_amd.server import DiffusionService
    monkeypatch.delenv("MIDD_BIT_DEPTH", raising=False)
    assert DiffusionService(device=torch.device("cpu")).bit_depth == 8
    assert DiffusionService(device=torch.device("cpu"), bit_depth=16).bit_depth == 16
    with pytest.raises(ValueError, match="bit_depth"):
        DiffusionService(device=torch.device("cpu"), bit_depth=7)
    monkeypatch.setenv("MIDD_BIT_DEPTH", "16")
    assert DiffusionService(device=torch.device("cpu")).bit_depth == 16
    assert DiffusionService(device=torch.device("cpu"), bit_depth=8).bit_depth == 8
    monkeypatch.setenv("MIDD_BIT_DEPTH", "12")
    with pytest.raises(ValueError, match="bit_depth"):
        DiffusionService(device=torch.device("cpu"))


# ------------------------------------------------------------------------------ host recipe on a 16-bit PNG
def _png16(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr.astype(np.uint16)).save(buf, format="PNG")
    return buf.getvalue()


def test_preprocess16_keeps_the_levels_of_a_12_bit_ramp():
    pytest.importorskip("PIL")
    from midd_amd.server import SERVE_SIZE, preprocess, preprocess16
    arr = (np.arange(SERVE_SIZE[0] * SERVE_SIZE[1], dtype=np.uint32) % 4096 * 16).astype(np.uint16).reshape(SERVE_SIZE)
    data = _png16(arr)
    x, size = preprocess16(data)                                       # identity size: no resample, the pure conversion
    assert size == SERVE_SIZE[::-1] and x.shape == (1, 1) + SERVE_SIZE and x.dtype == torch.float32
    np.testing.assert_array_equal(x[0, 0].numpy(), arr.astype(np.float32) / np.float32(65535))
    assert len(np.unique(x.numpy())) >= 4000
    x8, _ = preprocess(data)
    assert len(np.unique(x8.numpy())) <= 256                           # today's path: the high byte only


def test_preprocess16_resizes_in_float_and_falls_back_to_8_bit_files():
    from PIL import Image
    from midd_amd.server import SERVE_SIZE, preprocess16
    rng = np.random.default_rng(4)
    arr = rng.integers(0, 65536, (40, 56), dtype=np.uint16)
    x, size = preprocess16(_png16(arr))
    assert size == (56, 40)
    want = rr.recipe16_pre(arr, SERVE_SIZE)
    assert np.array_equal(x[0, 0].numpy().view(np.uint32), want.view(np.uint32))
    assert x.min() >= 0.0 and x.max() <= 1.0
    a8 = rng.integers(0, 256, (40, 56), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a8).save(buf, format="PNG")
    x8, _ = preprocess16(buf.getvalue())
    assert np.array_equal(x8[0, 0].numpy().view(np.uint32), rr.recipe16_pre(a8, SERVE_SIZE).view(np.uint32))


def test_tensor_to_base64_16_is_an_i16_png_at_the_requested_size():
    from PIL import Image
    from midd_amd.server import tensor_to_base64_16
    x = torch.from_numpy(_uniform(64, 64, 2) * 1.2 - 0.1)[None, None]
    img = Image.open(io.BytesIO(base64.b64decode(tensor_to_base64_16(x, (50, 30)))))
    assert img.mode == "I;16" and img.size == (50, 30)
    np.testing.assert_array_equal(np.asarray(img), rr.recipe16_post(x[0, 0].numpy(), 30, 50))


def test_service_process_path_at_16_bits_with_a_stand_in_sampler():
    from PIL import Image
    from midd_amd.server import SERVE_SIZE, DiffusionService
    arr = np.random.default_rng(6).integers(0, 65536, (44, 60), dtype=np.uint16)
    svc = DiffusionService(device=torch.device("cpu"), denoise_fn=lambda t: t * 0.5 + 0.25, bit_depth=16)
    out = svc.denoise_bytes(_png16(arr))
    img = Image.open(io.BytesIO(base64.b64decode(out["diffusion"])))
    assert img.mode == "I;16" and img.size == (60, 44)
    mid = rr.recipe16_pre(arr, SERVE_SIZE) * np.float32(0.5) + np.float32(0.25)
    np.testing.assert_array_equal(np.asarray(img), rr.recipe16_post(mid, 44, 60))


def test_cli_host_recipe_on_a_cpu_device(monkeypatch, tmp_path):
    """On a CPU device the host recipe runs around the sampler call (here a stand-in: the CPU has no sampler)."""
    from PIL import Image
    from midd_amd import cli
    arr = np.random.default_rng(8).integers(0, 65536, (48, 80), dtype=np.uint16)
    path = tmp_path / "in16.png"
    path.write_bytes(_png16(arr))
    seen = {}

    class _Denoiser:
        def __init__(self, model, noise_steps):
            pass

        def denoise(self, x, inference_steps):
            seen["x"] = x.clone()
            return (x * 0.75 + 0.125).clamp(0, 1)

    monkeypatch.setattr(cli, "DiffusionDenoiser", _Denoiser)
    monkeypatch.setattr(cli, "UNetDiffusion", lambda **kw: torch.nn.Identity())
    out = cli.denoise_image_diffusion(None, str(path), device_type="cpu", img_size=64, inference_steps=3, variant="ddim", bit_depth=16)
    assert out.mode == "I;16" and out.size == (80, 48)
    pre = rr.recipe16_pre(arr, (64, 64))
    assert np.array_equal(seen["x"][0, 0].numpy().view(np.uint32), pre.view(np.uint32))
    mid = np.clip(pre * np.float32(0.75) + np.float32(0.125), 0, 1)
    np.testing.assert_array_equal(np.asarray(out), rr.recipe16_post(mid, 48, 80))
    out.save(tmp_path / "out16.png")
    assert Image.open(tmp_path / "out16.png").mode == "I;16"
