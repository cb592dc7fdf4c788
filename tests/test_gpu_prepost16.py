"""GPU: the high-bit-depth pre/post-processing kernels (csrc/prepost.hip, through the C ABI and prepost.py) against the numpy
restatement (tests/resize_f32_reference.py, pinned to Pillow on the CPU) and against Pillow's mode "F" resample directly, and the
16-bit CLI / service paths against the recipe spelled out step by step.  Bar: bit for bit everywhere."""
import base64
import io
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import midd_loader  # noqa: E402

midd_loader.load()
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, image16, prepost  # noqa: E402
from midd_amd.native import MiddError  # noqa: E402
from midd_amd.weights import make_state_dict  # noqa: E402
from tests import resize_f32_reference as rr  # noqa: E402

try:
    from PIL import Image
except ImportError:                                                    # the restatement alone is then the reference
    Image = None

pytestmark = pytest.mark.gpu

# (source (h, w), destination (h, w)): up, down, mixed, vertical pass skipped, a one-pixel axis, 51 taps, horizontal pass skipped
SHAPES = [((37, 53), (48, 64)), ((64, 48), (24, 40)), ((50, 50), (128, 128)), ((97, 31), (40, 24)), ((33, 40), (33, 64)),
          ((1, 7), (5, 9)), ((97, 31), (8, 24)), ((40, 33), (64, 33))]
N = 3
_NP = {"f32": np.float32, "u16": np.uint16, "u8": np.uint8}
_REF = {}


def _batch(kind, h, w):
    """N images: uniform noise, a smooth pattern, a 0/1 block pattern (overshoots on both sides)."""
    rng = np.random.default_rng(h * 131 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    unit = np.stack([rng.random((h, w)), np.sin(xx / 7.0) * np.cos(yy / 5.0) * 0.5 + 0.5, (xx // 3 + yy // 3) % 2])
    if kind == "f32":
        return (unit * 2.0 - 0.5).astype(np.float32)                   # values in [-0.5, 1.5]: the clamp has work before the resample too
    top = 65535 if kind == "u16" else 255
    return np.round(unit * top).astype(_NP[kind])


def _reference(kind, shape):
    """The unclamped float32 resample of the batch, computed once and shared (never modified)."""
    key = (kind, shape)
    if key not in _REF:
        (h, w), (oh, ow) = shape
        ref = rr.resize_bicubic_f32(rr.load(_batch(kind, h, w)), oh, ow)
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kind", ["f32", "u16", "u8"])
@pytest.mark.parametrize("shape", SHAPES)
def test_resize_equals_the_restatement_and_pillow_bit_for_bit(shape, kind):
    (h, w), (oh, ow) = shape
    batch = _batch(kind, h, w)
    ref = _reference(kind, shape)
    dev = torch.from_numpy(batch).cuda()
    got = prepost.resize_bicubic_f32(dev, (oh, ow)).cpu().numpy()
    assert got.shape == (N, oh, ow) and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(ref)), np.abs(got - ref).max()
    if Image is not None:
        for i in range(N):
            pil = np.asarray(Image.fromarray(rr.load(batch[i])).resize((ow, oh), Image.BICUBIC))
            assert np.array_equal(_bits(got[i]), _bits(pil)), f"image {i}"
    if kind == "f32":
        assert ref.min() < 0.0 and ref.max() > 1.0                     # the clamp cases below have work to do
    clamped = prepost.resize_bicubic_f32(dev, (oh, ow), clamp=True).cpu().numpy()
    assert np.array_equal(_bits(clamped), _bits(rr.store(ref, rr.F32, True)))
    u16 = prepost.resize_bicubic_f32(dev, (oh, ow), out_dtype=torch.uint16).cpu().numpy()
    assert u16.dtype == np.uint16 and np.array_equal(u16, rr.store(ref, rr.U16, False))
    single = prepost.resize_bicubic_f32(dev[1], (oh, ow)).cpu().numpy()                       # [H,W] form, image stride
    assert np.array_equal(_bits(single), _bits(ref[1]))


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[4], SHAPES[7]])
def test_fused_forms_equal_convert_resize_convert(shape):
    (h, w), (oh, ow) = shape
    for kind, convert in (("u16", prepost.u16_to_unit_float), ("u8", prepost.to_unit_float)):
        dev = torch.from_numpy(_batch(kind, h, w)).cuda()
        fused = prepost.resize_bicubic_f32(dev, (oh, ow), out_dtype=torch.uint16).cpu().numpy()
        steps = prepost.to_u16(prepost.resize_bicubic_f32(convert(dev), (oh, ow))).cpu().numpy()
        assert np.array_equal(fused, steps)
        fused_f = prepost.resize_bicubic_f32(dev, (oh, ow), clamp=True)
        steps_f = prepost.resize_bicubic_f32(convert(dev), (oh, ow)).clamp(0, 1)
        assert torch.equal(fused_f, steps_f)


def test_same_sizes_is_the_pure_conversion():
    h, w = 37, 53
    for kind in ("u16", "u8", "f32"):
        batch = _batch(kind, h, w)
        dev = torch.from_numpy(batch).cuda()
        f = prepost.resize_bicubic_f32(dev, (h, w)).cpu().numpy()
        assert np.array_equal(_bits(f), _bits(rr.load(batch)))
        fc = prepost.resize_bicubic_f32(dev, (h, w), clamp=True).cpu().numpy()
        assert np.array_equal(_bits(fc), _bits(rr.clamp01(rr.load(batch))))
        u = prepost.resize_bicubic_f32(dev, (h, w), out_dtype=torch.uint16).cpu().numpy()
        assert np.array_equal(u, rr.to_u16(rr.load(batch)))
    u16 = _batch("u16", h, w)
    again = prepost.resize_bicubic_f32(torch.from_numpy(u16).cuda(), (h, w), out_dtype=torch.uint16).cpu().numpy()
    assert np.array_equal(again, u16)                                  # u16 -> float -> u16: the identity


def test_served_size_round_trip_equals_the_host_recipe():
    rng = np.random.default_rng(12)
    yy, xx = np.mgrid[0:300, 0:400]
    arr = np.where((xx // 16 + yy // 16) % 2 == 0, rng.integers(0, 65536, (300, 400)), 65535 * ((xx // 5) % 2)).astype(np.uint16)
    x = prepost.resize_bicubic_f32(torch.from_numpy(arr).cuda(), (512, 512), clamp=True)
    want_x = rr.recipe16_pre(arr, (512, 512))
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(want_x))
    back = prepost.resize_bicubic_f32(x, (300, 400), clamp=True, out_dtype=torch.uint16).cpu().numpy()
    assert np.array_equal(back, rr.recipe16_post(want_x, 300, 400))
    if Image is not None:
        host_x = image16.resize_f(image16.unit_float(arr), (512, 512))
        assert np.array_equal(_bits(host_x), _bits(want_x))
        assert np.array_equal(back, image16.to_u16(image16.resize_f(host_x, (300, 400))))


def test_conversions_over_all_65536_values():
    v = np.arange(65536, dtype=np.uint16)
    dev = torch.from_numpy(v).cuda()
    f = prepost.u16_to_unit_float(dev)
    assert np.array_equal(_bits(f.cpu().numpy()), _bits(rr.load(v)))
    assert np.array_equal(prepost.to_u16(f).cpu().numpy(), v)
    h = np.float32(0.5)
    x = np.concatenate([np.random.default_rng(0).uniform(-0.2, 1.2, 100000).astype(np.float32),
                        np.array([-0.1, 1.1, np.nextafter(h, np.float32(0)), h, np.nextafter(h, np.float32(1))], np.float32),
                        np.nextafter(rr.load(v), np.float32(0)), np.nextafter(rr.load(v), np.float32(2)),
                        (v.astype(np.float32) + np.float32(0.5)) / np.float32(65535)])
    got = prepost.to_u16(torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.array_equal(got, rr.to_u16(x))
    shaped = prepost.to_u16(torch.from_numpy(x[:60]).reshape(3, 4, 5).cuda())
    assert shaped.shape == (3, 4, 5) and shaped.dtype == torch.uint16


def test_errors_are_loud():
    z = torch.zeros((4, 4), device="cuda")
    with pytest.raises(RuntimeError):
        prepost.resize_bicubic_f32(torch.zeros((4, 4)), (8, 8))                               # CPU tensor: no fallback
    with pytest.raises(TypeError, match="uint8, uint16 or float32"):
        prepost.resize_bicubic_f32(z.double(), (8, 8))
    with pytest.raises(ValueError, match="out_dtype"):
        prepost.resize_bicubic_f32(z, (8, 8), out_dtype=torch.uint8)
    with pytest.raises(ValueError, match="bad sizes"):
        prepost.resize_bicubic_f32(z, (0, 8))
    with pytest.raises(ValueError, match=r"\[N,H,W\]"):
        prepost.resize_bicubic_f32(z[None, None], (8, 8))
    with pytest.raises(TypeError):
        prepost.to_u16(z.double())
    with pytest.raises(TypeError):
        prepost.u16_to_unit_float(z)
    from midd_amd import native
    lib = native.lib()
    out = torch.empty((8, 8), device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    wptr = (ws.data_ptr() + 255) & ~255
    with pytest.raises(MiddError, match="mi_resize_bicubic_u8"):
        native.check(lib.mi_resize_bicubic_f32(z.data_ptr(), native.MI_PIX_F32, 1, 4, 4, out.data_ptr(), native.MI_PIX_U8, 8, 8, 0,
                                               wptr, 1 << 15, None))
    with pytest.raises(MiddError, match="source element type"):
        native.check(lib.mi_resize_bicubic_f32(z.data_ptr(), 5, 1, 4, 4, out.data_ptr(), native.MI_PIX_F32, 8, 8, 0, wptr, 1 << 15, None))
    with pytest.raises(MiddError, match="too small"):
        native.check(lib.mi_resize_bicubic_f32(z.data_ptr(), native.MI_PIX_F32, 1, 4, 4, out.data_ptr(), native.MI_PIX_F32, 8, 8, 0,
                                               wptr, 64, None))
    with pytest.raises(MiddError, match="aligned"):
        native.check(lib.mi_resize_bicubic_f32(z.data_ptr(), native.MI_PIX_F32, 1, 4, 4, out.data_ptr(), native.MI_PIX_F32, 8, 8, 0,
                                               wptr + 8, 1 << 15, None))


# ------------------------------------------------------------------------------ CLI and service, end to end
SMALL = dict(model_channels=16, time_emb_dim=64)


@pytest.fixture(scope="module")
def small_model():
    cfg = UNetConfig(**SMALL)
    sd = make_state_dict(cfg, seed=5, perturb_norm=True)
    model = UNetDiffusion(**SMALL)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to("cuda:0").eval()


def _png16(path, h, w, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    arr = np.clip((np.sin(xx / 9.0) * np.cos(yy / 6.0) * 0.4 + 0.5) * 65535 + rng.normal(0, 3000, (h, w)), 0, 65535).astype(np.uint16)
    arr[: h // 4, : w // 4] = 65535                                     # a white block on a black one: the resample overshoots
    arr[h // 4: h // 2, : w // 4] = 0
    image16.image_from_u16(arr).save(path)
    return arr


def _cli(monkeypatch, model, path, **kw):
    from midd_amd import cli
    monkeypatch.setattr(cli, "UNetDiffusion", lambda **_: model)       # the CLI's own model is the full-size one
    return cli.denoise_image_diffusion(None, str(path), device_type="cuda", variant="ddim", bit_depth=16, **kw)


def test_cli_end_to_end_at_16_bits(monkeypatch, tmp_path, small_model):
    pytest.importorskip("PIL")
    arr = _png16(tmp_path / "in16.png", 48, 80, seed=3)
    size, steps = 64, 3
    out = _cli(monkeypatch, small_model, tmp_path / "in16.png", img_size=size, inference_steps=steps)
    assert out.mode == "I;16" and out.size == (80, 48)
    got = np.asarray(out)
    assert len(np.unique(got)) > 256                                    # more levels than an 8-bit file holds
    # the stepwise device recipe around the same denoise call
    x = prepost.resize_bicubic_f32(prepost.u16_to_unit_float(torch.from_numpy(arr).cuda()), (size, size)).clamp(0, 1)
    den = DiffusionDenoiser(small_model, noise_steps=50).denoise(x[None, None], inference_steps=steps)
    plane = den.reshape(size, size).float()
    stepwise = prepost.to_u16(prepost.resize_bicubic_f32(plane, (48, 80)).clamp(0, 1)).cpu().numpy()
    assert np.array_equal(got, stepwise)
    # the host Pillow-F recipe around that same tensor
    host_x = image16.resize_f(image16.unit_float(arr), (size, size))
    assert np.array_equal(_bits(host_x), _bits(x.cpu().numpy()))
    assert np.array_equal(got, image16.to_u16(image16.resize_f(plane.cpu().numpy(), (48, 80))))
    assert np.array_equal(got, rr.recipe16_post(plane.cpu().numpy(), 48, 80))
    out.save(tmp_path / "out16.png")
    assert np.array_equal(np.asarray(Image.open(tmp_path / "out16.png")), got)


def test_cli_self_ensemble_mean_at_16_bits(monkeypatch, tmp_path, small_model):
    arr = _png16(tmp_path / "in16.png", 48, 80, seed=4)
    size, steps = 64, 3
    out = _cli(monkeypatch, small_model, tmp_path / "in16.png", img_size=size, inference_steps=steps, self_ensemble="flips")
    x = prepost.resize_bicubic_f32(torch.from_numpy(arr).cuda(), (size, size), clamp=True)
    ens = DiffusionDenoiser(small_model, noise_steps=50).denoise_self_ensemble(x[None, None], inference_steps=steps, views="flips")
    want = prepost.resize_bicubic_f32(ens.mean.reshape(size, size).float(), (48, 80), clamp=True, out_dtype=torch.uint16)
    assert out.mode == "I;16" and np.array_equal(np.asarray(out), want.cpu().numpy())


def test_cli_tiled_at_16_bits_has_no_resize(monkeypatch, tmp_path, small_model):
    arr = _png16(tmp_path / "in16.png", 72, 56, seed=5)
    out = _cli(monkeypatch, small_model, tmp_path / "in16.png", inference_steps=3, tile=32, overlap=8)
    assert out.mode == "I;16" and out.size == (56, 72)
    x = torch.from_numpy(arr.astype(np.float32) / np.float32(65535))[None, None].cuda()
    res = DiffusionDenoiser(small_model, noise_steps=50).denoise_tiled(x, inference_steps=3, tile=32, overlap=8)
    assert np.array_equal(np.asarray(out), prepost.to_u16(res.image[0, 0].float()).cpu().numpy())
    assert np.array_equal(np.asarray(out), rr.to_u16(res.image[0, 0].cpu().numpy()))


def test_service_process_path_at_16_bits(tmp_path, small_model):
    from midd_amd.server import (SERVE_INFERENCE_STEPS, SERVE_SIZE, DiffusionService, preprocess16, preprocess16_device,
                                 tensor_to_base64_16, tensor_to_base64_16_device)
    arr = _png16(tmp_path / "in16.png", 76, 100, seed=6)
    data = (tmp_path / "in16.png").read_bytes()
    svc = DiffusionService(device=torch.device("cuda:0"), bit_depth=16)
    svc.diffusion_model = small_model                                   # the service's own model is the full-size one
    svc.diffusion_denoiser = DiffusionDenoiser(small_model, noise_steps=50)
    result = svc.denoise_bytes(data)["diffusion"]
    img = Image.open(io.BytesIO(base64.b64decode(result)))
    assert img.mode == "I;16" and img.size == (100, 76)
    x_host, size_host = preprocess16(data)
    x_dev, size_dev = preprocess16_device(data, torch.device("cuda:0"))
    assert size_host == size_dev == (100, 76) and torch.equal(x_dev.cpu(), x_host)
    assert np.array_equal(_bits(x_host[0, 0].numpy()), _bits(rr.recipe16_pre(arr, SERVE_SIZE)))
    den = svc.diffusion_denoiser.denoise(x_dev, inference_steps=SERVE_INFERENCE_STEPS).clamp(0, 1)
    assert result == tensor_to_base64_16_device(den, (100, 76)) == tensor_to_base64_16(den.cpu(), (100, 76))
    assert np.array_equal(np.asarray(img), rr.recipe16_post(den[0, 0].cpu().numpy(), 76, 100))
