"""GPU: the window of the 16-bit path (csrc/prepost.hip through the C ABI and prepost.py; include/midd.h: THE WINDOW) against the numpy
restatement (tests/window_reference.py, pinned to np.sort on the CPU), against the separate steps, against the image16 host recipe
(Pillow mode "F"), and the windowed CLI / service paths against the chain of the public pieces.  Bar: bit for bit everywhere."""
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
from midd_amd.weights import make_state_dict  # noqa: E402
from tests import window_reference as wr  # noqa: E402

try:
    from PIL import Image
except ImportError:
    Image = None

pytestmark = pytest.mark.gpu

PAIRS = [(0, 100), (0.5, 99.5), (33.3, 33.4)]
_CASES = {}


def _case(name):
    """uint16 [n][h][w], computed once and shared (never modified)."""
    if not _CASES:
        rng = np.random.default_rng(17)
        odd = rng.integers(0, 65536, (2, 45, 59)).astype(np.uint16)     # count = 2655 is odd: image 1 starts 2-byte aligned
        odd[1, :20] = 777                                               # a flat run in the misaligned image
        tiny = np.array([[[9, 9, 3, 9, 70, 9, 65535]]], np.uint16)      # 1 x 7: shorter than one 16-byte vector
        _CASES.update(odd=odd, tiny=tiny, zeros=np.zeros((1, 300, 300), np.uint16), ones=np.full((1, 300, 300), 65535, np.uint16),
                      noise12=rng.integers(0, 4096, (1, 520, 512)).astype(np.uint16))
        for a in _CASES.values():
            a.setflags(write=False)
    return _CASES[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    """Equality of two integer tensors (uint16 / uint32 have few operators on the device: compared on the host)."""
    return a.dtype == b.dtype and np.array_equal(a.cpu().numpy(), b.cpu().numpy())


def _ref_hist(batch):
    return np.stack([wr.histogram(img) for img in batch])


# ------------------------------------------------------------------------------ histogram
@pytest.mark.parametrize("name", ["odd", "tiny", "zeros", "ones", "noise12"])
def test_histogram_equals_bincount(name):
    batch = _case(name)
    dev = torch.from_numpy(batch.copy()).cuda()
    got = prepost.histogram_u16(dev)
    assert got.shape == (batch.shape[0], 65536) and got.dtype == torch.uint32
    want = _ref_hist(batch)
    assert np.array_equal(got.cpu().numpy(), want)
    assert int(want[0].sum()) == batch[0].size
    again = prepost.histogram_u16(dev)                                  # zeroed by the call itself; integer sums: the same bits
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    if batch.shape[0] == 1:
        assert np.array_equal(prepost.histogram_u16(dev[0]).cpu().numpy(), want)             # [H,W] form


def test_histogram_of_a_misaligned_view_and_many_blocks_per_image():
    """A slice that starts on an odd element (2-byte aligned only) and a 3-image batch large enough for several blocks per image."""
    rng = np.random.default_rng(3)
    flat = rng.integers(0, 300, 3 * 131071 + 1).astype(np.uint16)       # 131071 pixels per image: odd, above two chunks
    dev = torch.from_numpy(flat).cuda()[1:].reshape(3, 131071)
    assert dev.data_ptr() % 4 == 2
    got = prepost.histogram_u16(dev[:, None, :]).cpu().numpy()
    assert np.array_equal(got, _ref_hist(flat[1:].reshape(3, 1, 131071)))


def test_histogram_at_the_largest_block_share_does_not_carry_between_packed_counters():
    """256 images and more: one block per 65528 pixels, the most a block ever counts.  Flat images put all of them into ONE sixteen-bit
    on-chip counter (value 257 i: even and odd halves of a packed pair, 0 and 65535 included); a carry would show in the neighbour."""
    n, count = 256, 66000                                               # 65528 + 472: the second block's share is short
    values = np.arange(n) * 257
    dev = torch.from_numpy(np.repeat(values.astype(np.uint16)[:, None], count, axis=1)).cuda()
    got = prepost.histogram_u16(dev[:, None, :]).view(torch.int32)
    want = torch.zeros((n, 65536), dtype=torch.int32)
    want[torch.arange(n), torch.from_numpy(values)] = count
    assert torch.equal(got.cpu(), want)
    lv = prepost.window_levels(dev[:, None, :], (0, 100)).cpu().numpy()
    assert np.array_equal(lv[:-1, 0], values[:-1]) and np.array_equal(lv[:-1, 1], lv[:-1, 0] + 1)
    assert lv[-1].tolist() == [65534, 65535]


# ------------------------------------------------------------------------------ levels
@pytest.mark.parametrize("name", ["odd", "tiny", "zeros", "ones", "noise12"])
def test_levels_equal_the_restatement(name):
    batch = _case(name)
    dev = torch.from_numpy(batch.copy()).cuda()
    hist = prepost.histogram_u16(dev)
    for p_lo, p_hi in PAIRS:
        want = np.array([wr.levels(img, p_lo, p_hi) for img in batch], np.int32)
        from_images = prepost.window_levels(dev, (p_lo, p_hi))
        from_hist = prepost.window_levels(hist, (p_lo, p_hi))
        assert from_images.dtype == torch.int32 and from_images.is_cuda and tuple(from_images.shape) == (batch.shape[0], 2)
        assert np.array_equal(from_images.cpu().numpy(), want), (name, p_lo, p_hi, from_images.cpu().numpy(), want)
        assert torch.equal(from_hist, from_images)
        assert np.all(want[:, 0] < want[:, 1])
    if name == "tiny":
        assert prepost.window_levels(dev, (33.3, 33.4)).cpu().tolist() == [[9, 10]]           # both ranks in bin 9: the flat rule
    if name == "zeros":
        assert prepost.window_levels(dev).cpu().tolist() == [[0, 1]]
    if name == "ones":
        assert prepost.window_levels(dev).cpu().tolist() == [[65534, 65535]]
    assert torch.equal(prepost.window_levels(dev), prepost.window_levels(dev, (0.5, 99.5)))   # the default


# ------------------------------------------------------------------------------ conversions
def _levels(pairs):
    return torch.tensor(pairs, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("window", [(0, 65535), (1000, 3000), (65534, 65535)])
def test_conversions_over_all_65536_values(window):
    lo, hi = window
    v = np.arange(65536).astype(np.uint16).reshape(256, 256)
    dev = torch.from_numpy(v).cuda()
    lv = _levels([window])
    f = prepost.window_u16_to_float(dev, lv)
    assert f.shape == dev.shape and f.dtype == torch.float32
    assert np.array_equal(_bits(f.cpu().numpy()), _bits(wr.load(v, lo, hi)))
    back = prepost.window_to_u16(f, lv).cpu().numpy()
    assert np.array_equal(back, np.clip(v, lo, hi)) and np.array_equal(back, wr.store(wr.load(v, lo, hi), lo, hi))
    rng = np.random.default_rng(lo)
    x = np.concatenate([rng.uniform(-0.2, 1.2, 60000).astype(np.float32), np.nextafter(wr.load(v, lo, hi).ravel(), np.float32(2)),
                        np.nextafter(wr.load(v, lo, hi).ravel(), np.float32(-1)),
                        np.array([np.nan, -np.inf, np.inf, -0.0], np.float32)]).reshape(2, 1, -1)
    got = prepost.window_to_u16(torch.from_numpy(x).cuda(), _levels([window, window])).cpu().numpy()
    assert np.array_equal(got, wr.store(x, lo, hi))
    assert got[1, 0, -4] == lo and got[1, 0, -3] == lo and got[1, 0, -2] == hi                         # a NaN stores lo
    if window == (0, 65535):                                            # the unwindowed rule, bit for bit, both directions
        assert torch.equal(f, prepost.u16_to_unit_float(dev))
        assert _same(prepost.window_to_u16(torch.from_numpy(x).cuda(), _levels([window, window])), prepost.to_u16(torch.from_numpy(x).cuda()))


def test_conversions_take_the_levels_of_their_image():
    batch = _case("odd")                                                # n = 2, an odd count per image
    pairs = [(100, 40000), (30000, 30001)]
    dev, lv = torch.from_numpy(batch.copy()).cuda(), _levels(pairs)
    f = prepost.window_u16_to_float(dev, lv)
    want = np.stack([wr.load(batch[i], *pairs[i]) for i in range(2)])
    assert np.array_equal(_bits(f.cpu().numpy()), _bits(want))
    back = prepost.window_to_u16(f, lv).cpu().numpy()
    assert np.array_equal(back, np.stack([wr.store(want[i], *pairs[i]) for i in range(2)]))
    assert np.array_equal(back, np.stack([np.clip(batch[i], *pairs[i]) for i in range(2)]))
    assert np.array_equal(_bits(prepost.window_u16_to_float(dev[1], lv[1]).cpu().numpy()), _bits(want[1]))   # [H,W] with levels [2]
    data_levels = prepost.window_levels(dev, (0, 100))                  # the min-max window clips nothing
    assert _same(prepost.window_to_u16(prepost.window_u16_to_float(dev, data_levels), data_levels), dev)


# ------------------------------------------------------------------------------ fused resize
N = 3
RESIZES = [((37, 53), (48, 64)), ((97, 31), (40, 24)), ((37, 53), (37, 53))]
WINDOWS3 = [(0, 4095), (500, 3000), (2047, 2048)]


def _batch12(h, w):
    rng = np.random.default_rng(h * 131 + w)
    yy, xx = np.mgrid[0:h, 0:w]
    unit = np.stack([rng.random((h, w)), np.sin(xx / 7.0) * np.cos(yy / 5.0) * 0.5 + 0.5, (xx // 3 + yy // 3) % 2])
    return np.round(unit * 4095).astype(np.uint16)


@pytest.mark.parametrize("shape", RESIZES)
def test_fused_windowed_resize_equals_the_separate_steps_and_the_host_recipe(shape):
    (h, w), (oh, ow) = shape
    batch = _batch12(h, w)
    dev, lv = torch.from_numpy(batch).cuda(), _levels(WINDOWS3)
    fused = prepost.resize_bicubic_f32(dev, (oh, ow), levels=lv)                              # windowed load -> float
    steps = prepost.resize_bicubic_f32(prepost.window_u16_to_float(dev, lv), (oh, ow))
    assert fused.dtype == torch.float32 and torch.equal(fused, steps)
    fused_c = prepost.resize_bicubic_f32(dev, (oh, ow), clamp=True, levels=lv)
    assert torch.equal(fused_c, steps.clamp(0, 1))
    x = (steps * 1.2 - 0.1).contiguous()                                                      # leaves [0, 1] on both sides
    back = prepost.resize_bicubic_f32(x, (h, w), out_dtype=torch.uint16, levels=lv)           # float -> windowed store
    assert back.dtype == torch.uint16 and _same(back, prepost.window_to_u16(prepost.resize_bicubic_f32(x, (h, w)), lv))
    both = prepost.resize_bicubic_f32(dev, (oh, ow), out_dtype=torch.uint16, levels=lv)       # u16 -> u16, both sides windowed
    assert _same(both, prepost.window_to_u16(steps, lv))
    single = prepost.resize_bicubic_f32(dev[1], (oh, ow), clamp=True, levels=lv[1])           # [H,W] form with levels [2]
    assert torch.equal(single, fused_c[1])
    for i, (lo, hi) in enumerate(WINDOWS3):
        assert back[i].cpu().numpy().min() >= lo and back[i].cpu().numpy().max() <= hi
        if Image is not None:                                                                 # Pillow mode "F" around the host twins
            host = image16.resize_f(image16.unit_float_window(batch[i], (lo, hi)), (oh, ow))
            assert np.array_equal(_bits(host), _bits(fused_c[i].cpu().numpy())), i
            host_back = image16.to_u16_window(image16.resize_f(x[i].cpu().numpy(), (h, w)), (lo, hi))
            assert np.array_equal(host_back, back[i].cpu().numpy()), i
    # levels=None is today's call
    assert torch.equal(prepost.resize_bicubic_f32(dev, (oh, ow), levels=None), prepost.resize_bicubic_f32(dev, (oh, ow)))
    assert _same(prepost.resize_bicubic_f32(x, (h, w), out_dtype=torch.uint16, levels=None),
                       prepost.resize_bicubic_f32(x, (h, w), out_dtype=torch.uint16))
    full = _levels([(0, 65535)] * N)                                    # the window (0, 65535) is the unwindowed call
    assert torch.equal(prepost.resize_bicubic_f32(dev, (oh, ow), levels=full), prepost.resize_bicubic_f32(dev, (oh, ow)))
    assert _same(prepost.resize_bicubic_f32(x, (h, w), out_dtype=torch.uint16, levels=full),
                       prepost.resize_bicubic_f32(x, (h, w), out_dtype=torch.uint16))


# ------------------------------------------------------------------------------ errors
def test_errors_are_loud():
    img = torch.zeros((2, 4, 4), dtype=torch.uint16, device="cuda")
    lv = _levels([(0, 10), (0, 10)])
    img_f = torch.zeros((2, 4, 4), device="cuda")
    with pytest.raises(RuntimeError):
        prepost.histogram_u16(img.cpu())                                # CPU tensors: no fallback
    with pytest.raises(RuntimeError):
        prepost.window_u16_to_float(img, lv.cpu())
    with pytest.raises(RuntimeError):
        prepost.window_to_u16(torch.zeros((2, 4, 4)), lv)
    with pytest.raises(TypeError):
        prepost.histogram_u16(img_f)
    with pytest.raises(TypeError):
        prepost.window_levels(img_f.to(torch.int32))
    with pytest.raises(TypeError):
        prepost.window_u16_to_float(img_f, lv)
    with pytest.raises(TypeError):
        prepost.window_to_u16(img, lv)
    with pytest.raises(TypeError):
        prepost.window_u16_to_float(img, lv.long())
    with pytest.raises(TypeError):
        prepost.window_u16_to_float(img, [(0, 10), (0, 10)])
    for bad in (lv[:1], lv.reshape(4), lv.reshape(1, 4), lv.reshape(2, 2, 1)):
        with pytest.raises(ValueError, match="levels must have shape"):
            prepost.window_u16_to_float(img, bad)
        with pytest.raises(ValueError, match="levels must have shape"):
            prepost.window_to_u16(img_f, bad)
        with pytest.raises(ValueError, match="levels must have shape"):
            prepost.resize_bicubic_f32(img, (8, 8), levels=bad)
    with pytest.raises(ValueError, match="uint16"):
        prepost.resize_bicubic_f32(img_f, (8, 8), levels=lv)                            # no 16-bit side
    with pytest.raises(ValueError, match="65536"):
        prepost.window_levels(torch.zeros((2, 100), dtype=torch.uint32, device="cuda"))
    from midd_amd.native import MiddError
    for p in ((60, 40), (0, 101), (float("nan"), 50)):
        with pytest.raises(MiddError):
            prepost.window_levels(img, p)


# ------------------------------------------------------------------------------ CLI and service, end to end
SMALL = dict(model_channels=16, time_emb_dim=64)


@pytest.fixture(scope="module")
def small_model():
    cfg = UNetConfig(**SMALL)
    sd = make_state_dict(cfg, seed=5, perturb_norm=True)
    model = UNetDiffusion(**SMALL)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to("cuda:0").eval()


def _png12(path, h, w, seed):
    """A 12-bit detector image in a 16-bit PNG: values in [0, 4095], both ends present."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    arr = np.clip((np.sin(xx / 9.0) * np.cos(yy / 6.0) * 0.4 + 0.5) * 4095 + rng.normal(0, 200, (h, w)), 0, 4095).astype(np.uint16)
    arr[: h // 4, : w // 4] = 4095
    arr[h // 4: h // 2, : w // 4] = 0
    image16.image_from_u16(arr).save(path)
    return arr


def _cli(monkeypatch, model, path, **kw):
    from midd_amd import cli
    monkeypatch.setattr(cli, "UNetDiffusion", lambda **_: model)       # the CLI's own model is the full-size one
    return cli.denoise_image_diffusion(None, str(path), device_type="cuda", variant="ddim", bit_depth=16, **kw)


def test_cli_end_to_end_with_a_window_resized(monkeypatch, tmp_path, small_model, capsys):
    pytest.importorskip("PIL")
    arr = _png12(tmp_path / "in12.png", 70, 90, seed=3)
    size, steps = 64, 3
    out = _cli(monkeypatch, small_model, tmp_path / "in12.png", img_size=size, inference_steps=steps, window=(0, 100))
    assert "Window: grey levels 0 .. 4095" in capsys.readouterr().out
    assert out.mode == "I;16" and out.size == (90, 70)
    got = np.asarray(out)
    assert got.min() >= 0 and got.max() <= 4095                         # within the window: the file's own 4096 levels
    # the manual chain of the public pieces around the same denoise call
    dev = torch.from_numpy(arr).cuda()
    lv = prepost.window_levels(dev, (0, 100))
    assert lv.cpu().tolist() == [[0, 4095]]
    x = prepost.resize_bicubic_f32(prepost.window_u16_to_float(dev, lv), (size, size)).clamp(0, 1)
    den = DiffusionDenoiser(small_model, noise_steps=50).denoise(x[None, None], inference_steps=steps)
    plane = den.reshape(size, size).float()
    chain = prepost.window_to_u16(prepost.resize_bicubic_f32(plane, (70, 90)), lv).cpu().numpy()
    assert np.array_equal(got, chain)
    # the host recipe around that same tensor
    host_x = image16.resize_f(image16.unit_float_window(arr, (0, 4095)), (size, size))
    assert np.array_equal(_bits(host_x), _bits(x.cpu().numpy()))
    assert np.array_equal(got, image16.to_u16_window(image16.resize_f(plane.cpu().numpy(), (70, 90)), (0, 4095)))
    # what the sampler saw: [0, 1] under the window, the same picture 4095 / 65535 as bright without it
    plain = prepost.u16_to_unit_float(dev)
    windowed = prepost.window_u16_to_float(dev, lv)
    assert float(windowed.min()) == 0.0 and float(windowed.max()) == 1.0 and float(plain.max()) == np.float32(4095) / np.float32(65535)
    ratio = (plain.double() * 65535.0 / 4095.0 - windowed.double()).abs().max()
    assert float(ratio) <= 2.0 ** -23                                   # two correctly rounded fp32 quotients of the same integers
    # absolute levels: no histogram, the same chain under (1000, 3000)
    out2 = _cli(monkeypatch, small_model, tmp_path / "in12.png", img_size=size, inference_steps=steps, window_levels=(1000, 3000))
    lv2 = _levels([(1000, 3000)])
    x2 = prepost.resize_bicubic_f32(dev, (size, size), clamp=True, levels=lv2)
    den2 = DiffusionDenoiser(small_model, noise_steps=50).denoise(x2[None, None], inference_steps=steps)
    want2 = prepost.resize_bicubic_f32(den2.reshape(size, size).float(), (70, 90), clamp=True, out_dtype=torch.uint16, levels=lv2)
    assert np.array_equal(np.asarray(out2), want2.cpu().numpy()) and np.asarray(out2).min() >= 1000 and np.asarray(out2).max() <= 3000


def test_cli_tiled_with_a_window_has_no_resize(monkeypatch, tmp_path, small_model):
    arr = _png12(tmp_path / "in12.png", 70, 90, seed=5)
    out = _cli(monkeypatch, small_model, tmp_path / "in12.png", inference_steps=3, tile=64, overlap=8, window=(0, 100))
    assert out.mode == "I;16" and out.size == (90, 70)
    dev = torch.from_numpy(arr).cuda()
    lv = prepost.window_levels(dev, (0, 100))
    x = prepost.window_u16_to_float(dev, lv)[None, None]
    res = DiffusionDenoiser(small_model, noise_steps=50).denoise_tiled(x, inference_steps=3, tile=64, overlap=8)
    assert np.array_equal(np.asarray(out), prepost.window_to_u16(res.image[0, 0].float(), lv).cpu().numpy())
    assert np.array_equal(np.asarray(out), wr.store(res.image[0, 0].cpu().numpy(), 0, 4095))
    assert np.asarray(out).max() <= 4095


def test_service_process_path_with_a_window(tmp_path, small_model):
    from midd_amd.server import (SERVE_INFERENCE_STEPS, DiffusionService, preprocess16_window, preprocess16_window_device,
                                 tensor_to_base64_16_window, tensor_to_base64_16_window_device)
    _png12(tmp_path / "in12.png", 70, 90, seed=6)
    data = (tmp_path / "in12.png").read_bytes()
    svc = DiffusionService(device=torch.device("cuda:0"), bit_depth=16, window=(0, 100))
    svc.diffusion_model = small_model                                   # the service's own model is the full-size one
    svc.diffusion_denoiser = DiffusionDenoiser(small_model, noise_steps=50)
    result = svc.denoise_bytes(data)["diffusion"]
    img = Image.open(io.BytesIO(base64.b64decode(result)))
    assert img.mode == "I;16" and img.size == (90, 70) and np.asarray(img).max() <= 4095
    x_host, size_host = preprocess16_window(data, (0, 100))
    x_dev, size_dev = preprocess16_window_device(data, torch.device("cuda:0"), (0, 100))
    assert size_host == (90, 70, (0, 4095)) and size_dev[:2] == (90, 70) and size_dev[2].cpu().tolist() == [[0, 4095]]
    assert torch.equal(x_dev.cpu(), x_host) and float(x_host.max()) == 1.0
    den = svc.diffusion_denoiser.denoise(x_dev, inference_steps=SERVE_INFERENCE_STEPS).clamp(0, 1)
    assert result == tensor_to_base64_16_window_device(den, size_dev) == tensor_to_base64_16_window(den.cpu(), size_host)
