"""The images and recipe kinds that test_image_recipe_cpu.py and test_gpu_image_recipe.py share, and the host recipe written out
with image16 and Pillow, as cli.py and server.py had it before recipe.py: what ``ImageRecipe.load`` / ``store`` are compared with."""
import io

import numpy as np
from PIL import Image

H, W = 40, 56
# (bit_depth, window percentiles, window levels)
KINDS = [(8, None, None), (16, None, None), (16, (0, 100), None), (16, (10, 90), None), (16, None, (1000, 3000))]


def images() -> dict:
    """name -> PIL image of W x H: an 8-bit "L" file, an RGB file, an "I;16" file holding a 12-bit ramp, an "I" file."""
    n = np.arange(H * W, dtype=np.uint32).reshape(H, W)
    rgb = np.stack([(n * 7) % 256, (n * 11 + 40) % 256, (n * 5 + 90) % 256], axis=-1).astype(np.uint8)
    return {"L": Image.fromarray(((n * 3 + n // W * 17) % 256).astype(np.uint8), mode="L"), "RGB": Image.fromarray(rgb, mode="RGB"),
            "I;16": Image.fromarray((n * 37 % 4096).astype(np.uint16)), "I": Image.fromarray((n * 29 % 60001).astype(np.int32))}


def is_16(image: Image.Image) -> bool:
    return image.mode in ("I;16", "I")


def png(image: Image.Image) -> bytes:
    buf = io.BytesIO()
    image.save(buf, format="PNG")
    return buf.getvalue()


def file_array(image: Image.Image) -> np.ndarray:
    """What the file holds: uint16 for the two 16-bit files, else the uint8 of `convert("L")`."""
    return np.asarray(image).astype(np.uint16) if is_16(image) else np.asarray(image.convert("L"), dtype=np.uint8)


def host_load(image: Image.Image, kind, target, levels=None):
    """-> (float32 [H][W], (lo, hi) or None): the recipe on the host, written out."""
    from midd_amd import image16
    bit_depth, window, window_levels = kind
    if bit_depth == 8:
        grey = image.convert("L")
        if target is not None:
            grey = grey.resize((target[1], target[0]), Image.BICUBIC)
        return np.asarray(grey, dtype=np.uint8).astype(np.float32) / 255.0, None
    raw = image16.decode16(image)
    size = raw.shape if target is None else target
    if window is None and window_levels is None:
        return image16.resize_f(image16.unit_float(raw), size), None
    if levels is None:
        levels = image16.window_levels(raw, window) if window is not None else window_levels
    return image16.resize_f(image16.unit_float_window(raw, levels), size), tuple(levels)


def host_store(x: np.ndarray, kind, size_wh, levels) -> np.ndarray:
    """float32 [H][W] -> the array of the output file at PIL size `size_wh`: the way back on the host, written out."""
    from midd_amd import image16
    if kind[0] == 8:
        return np.asarray(Image.fromarray((x * 255).astype(np.uint8), mode="L").resize(size_wh, Image.BICUBIC))
    back = image16.resize_f(x, (size_wh[1], size_wh[0]))
    return image16.to_u16(back) if levels is None else image16.to_u16_window(back, levels)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
