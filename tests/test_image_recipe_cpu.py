"""CPU: recipe.py, the one statement of the image recipe (8-bit, 16-bit, 16-bit under a window), on its host side -- against the
image16 / Pillow expressions written out in tests/image_recipe_cases.py, on four kinds of file, at a resize target and at the
image's own size; the way back; the counterpart under another image's levels; and the service's names, which delegate to it.
Everything here is exact: there is no tolerance."""
import base64
import io
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import image_recipe_cases as rc  # noqa: E402

CPU = torch.device("cpu")
TARGETS = [(32, 24), None]
IMAGES = rc.images()


def _recipe(kind):
    from midd_amd.recipe import ImageRecipe
    return ImageRecipe(kind[0], window=kind[1], window_levels=kind[2])


def _refused(name, kind) -> bool:
    return (kind[1] is not None or kind[2] is not None) and not rc.is_16(IMAGES[name])


def test_the_images_are_the_four_kinds_of_file():
    assert {n: im.mode for n, im in IMAGES.items()} == {"L": "L", "RGB": "RGB", "I;16": "I;16", "I": "I"}
    assert all(im.size == (rc.W, rc.H) for im in IMAGES.values())
    ramp = np.asarray(IMAGES["I;16"])
    assert ramp.min() == 0 and ramp.max() == 4095 and np.asarray(IMAGES["I"]).max() > 4095


@pytest.mark.parametrize("target", TARGETS, ids=str)
@pytest.mark.parametrize("kind", rc.KINDS, ids=str)
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_load_is_the_host_recipe_written_out(name, kind, target):
    from midd_amd import image16
    image, recipe = IMAGES[name], _recipe(kind)
    if _refused(name, kind):
        with pytest.raises(image16.WindowInputError, match=repr(image.mode)):
            recipe.load(image, target, CPU)
        return
    x, source = recipe.load(image, target, CPU)
    want, levels = rc.host_load(image, kind, target)
    assert x.dtype == torch.float32 and x.device == CPU and tuple(x.shape) == (1, 1) + (target or (rc.H, rc.W))
    assert np.array_equal(rc.bits(x[0, 0].numpy()), rc.bits(want))
    assert source.size == image.size and source.is_u16 == (kind[0] == 16 and rc.is_16(image)) and source.levels == levels
    assert source.as_tuple() == (image.size if levels is None else image.size + (levels,))
    assert float(x.min()) >= 0.0 and float(x.max()) <= 1.0


@pytest.mark.parametrize("name,kind", [(n, k) for n in sorted(IMAGES) for k in rc.KINDS if not _refused(n, k)], ids=str)
def test_store_of_load_at_the_own_size_returns_the_file(name, kind):
    image, recipe = IMAGES[name], _recipe(kind)
    x, source = recipe.load(image, None, CPU)
    back = recipe.store(x, source)
    arr = rc.file_array(image)
    assert back.shape == (rc.H, rc.W) and np.array_equal(back, rc.host_store(x[0, 0].numpy(), kind, image.size, source.levels))
    if kind[0] == 8:
        grey = np.asarray(image.convert("L"), dtype=np.uint8)
        assert back.dtype == np.uint8 and np.array_equal(back, (grey.astype(np.float32) / 255.0 * 255).astype(np.uint8))
    elif source.levels is not None:
        lo, hi = source.levels
        assert back.dtype == np.uint16 and np.array_equal(back, np.clip(arr, lo, hi))      # the window clips, and nothing else
        if kind[1] == (0, 100):
            assert (lo, hi) == (arr.min(), arr.max()) and np.array_equal(back, arr)
    elif rc.is_16(image):
        assert back.dtype == np.uint16 and np.array_equal(back, arr)
    else:       # an 8-bit file under bit_depth 16: / 255 in, a 16-bit image out
        assert back.dtype == np.uint16 and np.array_equal(back, arr.astype(np.uint16) * 257)


@pytest.mark.parametrize("kind", rc.KINDS, ids=str)
def test_store_resizes_back_to_the_source_size(kind):
    image, recipe = IMAGES["I;16"], _recipe(kind)
    x, source = recipe.load(image, (32, 24), CPU)
    y = torch.clamp(1.03 * x - 0.01, 0, 1)
    back = recipe.store(y, source)
    assert back.shape == (rc.H, rc.W) and np.array_equal(back, rc.host_store(y[0, 0].numpy(), kind, image.size, source.levels))
    assert np.array_equal(recipe.store(y[0, 0], source), back) and np.array_equal(recipe.store(y[0], source), back)      # [.., H, W]


@pytest.mark.parametrize("target", TARGETS, ids=str)
def test_the_counterpart_goes_through_the_other_images_levels(target):
    from midd_amd.recipe import ImageRecipe
    noisy, clean = IMAGES["I;16"], IMAGES["I"]
    for kind in [k for k in rc.KINDS if k[1] is not None or k[2] is not None]:
        recipe = _recipe(kind)
        levels = recipe.load(noisy, target, CPU)[1].levels
        x, source = recipe.load(clean, target, CPU, levels=levels)
        own = recipe.load(clean, target, CPU)[1].levels
        assert source.levels == levels and (kind[2] is not None or own != levels)
        assert np.array_equal(rc.bits(x[0, 0].numpy()), rc.bits(rc.host_load(clean, kind, target, levels=levels)[0]))
    x, source = ImageRecipe(16).load(clean, target, CPU, levels=None)
    assert source.levels is None and np.array_equal(rc.bits(x[0, 0].numpy()), rc.bits(rc.host_load(clean, rc.KINDS[1], target)[0]))


def test_the_recipe_refuses_what_its_callers_refused():
    from midd_amd.recipe import ImageRecipe, Source
    with pytest.raises(ValueError, match="bit_depth must be 8 or 16"):
        ImageRecipe(12)
    with pytest.raises(ValueError, match="cannot be combined"):
        ImageRecipe(16, window=(0, 100), window_levels=(0, 9))
    with pytest.raises(ValueError, match="p_lo < p_hi"):
        ImageRecipe(16, window=(60, 40))
    with pytest.raises(ValueError, match="lo < hi"):
        ImageRecipe(16, window_levels=(9, 3))
    with pytest.raises(ValueError, match="bit_depth=16"):
        ImageRecipe(8, window=(1, 99))
    r = ImageRecipe(16, window=(1, 99))
    assert (r.bit_depth, r.window, r.window_levels, r.windowed) == (16, (1.0, 99.0), None, True) and not ImageRecipe().windowed
    assert Source.of((56, 40)) == Source((56, 40)) and Source.of((56, 40, (3, 9))) == Source((56, 40), None, (3, 9))
    assert Source((56, 40), True, (3, 9)).as_tuple() == (56, 40, (3, 9)) and Source((56, 40), True).as_tuple() == (56, 40)


@pytest.mark.parametrize("kind", [k for k in rc.KINDS if k[2] is None], ids=str)      # (the service takes percentiles only)
def test_the_services_names_and_the_service_are_the_recipe(kind, monkeypatch):
    from midd_amd import server
    monkeypatch.delenv("MIDD_BIT_DEPTH", raising=False)
    monkeypatch.delenv("MIDD_WINDOW", raising=False)
    monkeypatch.delenv("MIDD_TILE", raising=False)
    monkeypatch.setattr(server, "SERVE_SIZE", (32, 24))
    image, recipe = IMAGES["I;16"], _recipe(kind)
    data = rc.png(image)
    load = {8: server.preprocess, 16: server.preprocess16}[kind[0]] if kind[1] is None else \
        (lambda b, tile=None: server.preprocess16_window(b, kind[1], tile=tile))
    store = {8: server.tensor_to_base64, 16: server.tensor_to_base64_16}[kind[0]] if kind[1] is None else server.tensor_to_base64_16_window
    for tile, target in ((None, (32, 24)), ((8, 8), None), ((48, 8), (48, rc.W))):
        x, source = recipe.load(Image.open(io.BytesIO(data)), target, CPU)
        got, size = load(data, tile=tile)
        assert size == source.as_tuple() and np.array_equal(rc.bits(got.numpy()), rc.bits(x.numpy()))
        want = base64.b64encode(rc.png(Image.fromarray(recipe.store(x, source)))).decode()
        assert store(got, size) == want
        svc = server.DiffusionService(denoise_fn=lambda t: t, device=CPU, bit_depth=kind[0], window=kind[1], tile=tile, overlap=0)
        assert svc.preprocess(data)[1] == size and svc.denoise_bytes(data)["diffusion"] == want
        out = np.asarray(Image.open(io.BytesIO(base64.b64decode(want))))
        assert out.shape == (rc.H, rc.W) and out.dtype == (np.uint8 if kind[0] == 8 else np.uint16)
