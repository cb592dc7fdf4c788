"""GPU: recipe.py's device side (the prepost kernels) against its host side (image16 / Pillow) on the images and kinds of
tests/image_recipe_cases.py, at a downsizing target, at the image's own size and at an upsizing target -- and the spellings that
cli.py's --tile path had of its own (host / 255 and upload, u16_to_unit_float, window_u16_to_float, to_u16, window_to_u16, the host
x 255 truncation) against the recipe's one.  Bar: bit for bit everywhere; no tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import midd_loader  # noqa: E402

midd_loader.load()
from midd_amd import prepost  # noqa: E402
from midd_amd.recipe import ImageRecipe, Source  # noqa: E402
from tests import image_recipe_cases as rc  # noqa: E402

pytestmark = pytest.mark.gpu

CPU, GPU = torch.device("cpu"), torch.device("cuda:0")
TARGETS = [(32, 24), None, (64, 72)]
IMAGES = rc.images()
CASES = [(n, k) for n in sorted(IMAGES) for k in rc.KINDS if (k[1] is None and k[2] is None) or rc.is_16(IMAGES[n])]


def _recipe(kind):
    return ImageRecipe(kind[0], window=kind[1], window_levels=kind[2])


def _both(name, kind, target):
    """-> recipe, (x, source) on the host, (x, source) on the device."""
    recipe = _recipe(kind)
    return recipe, recipe.load(IMAGES[name], target, CPU), recipe.load(IMAGES[name], target, GPU)


@pytest.mark.parametrize("target", TARGETS, ids=str)
@pytest.mark.parametrize("name,kind", CASES, ids=str)
def test_load_and_store_on_the_device_are_those_of_the_host(name, kind, target):
    recipe, (hx, hsrc), (dx, dsrc) = _both(name, kind, target)
    assert dx.is_cuda and dx.dtype == torch.float32 and tuple(dx.shape) == tuple(hx.shape) == (1, 1) + (target or (rc.H, rc.W))
    assert np.array_equal(rc.bits(dx.cpu().numpy()), rc.bits(hx.numpy()))
    assert dsrc.size == hsrc.size == IMAGES[name].size and dsrc.is_u16 == hsrc.is_u16
    if hsrc.levels is None:
        assert dsrc.levels is None
    else:       # the levels stay on the device
        assert dsrc.levels.is_cuda and dsrc.levels.dtype == torch.int32 and dsrc.levels.cpu().tolist() == [list(hsrc.levels)]
    for y in (hx, torch.clamp(1.03 * hx - 0.01, 0, 1)):      # the identity, and a map that reaches both ends of the clip
        want = recipe.store(y, hsrc)
        got = recipe.store(y.to(GPU), dsrc)
        assert got.dtype == want.dtype and got.shape == want.shape == (rc.H, rc.W) and np.array_equal(got, want)
        assert np.array_equal(want, rc.host_store(y[0, 0].numpy(), kind, hsrc.size, hsrc.levels))


@pytest.mark.parametrize("target", TARGETS, ids=str)
def test_the_counterpart_goes_through_the_other_images_levels(target):
    for kind in [k for k in rc.KINDS if k[1] is not None or k[2] is not None]:
        recipe = _recipe(kind)
        host_levels = recipe.load(IMAGES["I;16"], target, CPU)[1].levels
        levels = recipe.load(IMAGES["I;16"], target, GPU)[1].levels
        x, source = recipe.load(IMAGES["I"], target, GPU, levels=levels)
        assert source.levels is levels and levels.is_cuda
        want = recipe.load(IMAGES["I"], target, CPU, levels=host_levels)[0]
        assert np.array_equal(rc.bits(x.cpu().numpy()), rc.bits(want.numpy()))


def test_the_merged_spellings_agree():
    """At the image's own size the --tile path of cli.py converted by calls of its own; the recipe keeps the service's."""
    from midd_amd import image16
    grey = np.asarray(IMAGES["RGB"].convert("L"), dtype=np.uint8)
    x8, src8 = ImageRecipe(8).load(IMAGES["RGB"], None, GPU)
    assert np.array_equal(rc.bits(x8[0, 0].cpu().numpy()), rc.bits(grey.astype(np.float32) / 255.0))      # host / 255, then upload
    y8 = torch.clamp(1.03 * x8 - 0.01, 0, 1)
    assert np.array_equal(ImageRecipe(8).store(y8, src8), (y8[0, 0].cpu().numpy() * 255).astype(np.uint8))   # download, x 255 truncated
    for name in ("I;16", "I"):
        raw = image16.decode16(IMAGES[name])
        dev = torch.from_numpy(raw).to(GPU)
        x16, src16 = ImageRecipe(16).load(IMAGES[name], None, GPU)
        assert raw.dtype == np.uint16 and np.array_equal(rc.bits(x16[0, 0].cpu().numpy()), rc.bits(prepost.u16_to_unit_float(dev).cpu().numpy()))
        y16 = torch.clamp(1.03 * x16 - 0.01, 0, 1)
        assert np.array_equal(ImageRecipe(16).store(y16, src16), prepost.to_u16(y16[0, 0]).cpu().numpy())
        for kind in rc.KINDS[2:]:
            recipe = _recipe(kind)
            xw, srcw = recipe.load(IMAGES[name], None, GPU)
            assert srcw.levels.is_cuda
            assert np.array_equal(rc.bits(xw[0, 0].cpu().numpy()), rc.bits(prepost.window_u16_to_float(dev, srcw.levels).cpu().numpy()))
            yw = torch.clamp(1.03 * xw - 0.01, 0, 1)
            assert np.array_equal(recipe.store(yw, srcw), prepost.window_to_u16(yw[0, 0], srcw.levels).cpu().numpy())
    raw8 = image16.decode16(IMAGES["L"])      # an 8-bit file under bit_depth 16: / 255
    x, _ = ImageRecipe(16).load(IMAGES["L"], None, GPU)
    assert raw8.dtype == np.uint8 and np.array_equal(rc.bits(x[0, 0].cpu().numpy()), rc.bits(prepost.to_unit_float(torch.from_numpy(raw8).to(GPU)).cpu().numpy()))


def test_the_service_names_keep_their_results_on_the_device(monkeypatch):
    from midd_amd import server
    monkeypatch.setattr(server, "SERVE_SIZE", (32, 24))
    data = rc.png(IMAGES["I;16"])
    for host, dev, back, kind in ((server.preprocess, server.preprocess_device, server.tensor_to_base64_device, rc.KINDS[0]),
                                  (server.preprocess16, server.preprocess16_device, server.tensor_to_base64_16_device, rc.KINDS[1])):
        (hx, hsize), (dx, dsize) = host(data), dev(data, GPU)
        assert dx.is_cuda and hsize == dsize == (rc.W, rc.H) and np.array_equal(rc.bits(dx.cpu().numpy()), rc.bits(hx.numpy()))
        assert back(dx, dsize) == back(hx, hsize)
    (hx, hsize), (dx, dsize) = server.preprocess16_window(data, (10, 90)), server.preprocess16_window_device(data, GPU, (10, 90))
    assert dsize[2].is_cuda and dsize[2].cpu().tolist() == [list(hsize[2])] and Source.of(dsize).levels is dsize[2]
    assert np.array_equal(rc.bits(dx.cpu().numpy()), rc.bits(hx.numpy()))
    assert server.tensor_to_base64_16_window_device(dx, dsize) == server.tensor_to_base64_16_window(hx, hsize)
