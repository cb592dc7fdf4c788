"""The 16-bit image recipe either side of the sampler, host side (include/midd.h: THE FLOAT RESIZE AND THE 16-BIT ELEMENT RULES).

Not in the reference, whose every path squeezes an image through 256 grey levels (`convert("L")` in, `(x * 255).astype(uint8)`
out): a 16-bit PNG is decoded to its 65536 levels, scaled to unit float, resampled by Pillow in mode "F" (its 32bpc resample, not
its "I;16" one, which wraps the low byte on overshoot), clipped, and stored back as u16 rounded to nearest.  These functions are the
recipe with Pillow and numpy; `prepost.resize_bicubic_f32` / `u16_to_unit_float` / `to_u16` are the same arithmetic on the GPU, bit
for bit.  cli.py and server.py use whichever side their tensors live on.
"""
import io
from typing import Tuple

import numpy as np
from PIL import Image

_MODES_16 = ("I;16", "I;16L", "I;16B", "I;16N")


def check_bit_depth(bit_depth) -> int:
    if bit_depth not in (8, 16) or isinstance(bit_depth, bool):
        raise ValueError(f"bit_depth must be 8 or 16 (got {bit_depth!r})")
    return int(bit_depth)


def decode16(image: Image.Image) -> np.ndarray:
    """A PIL image -> uint16 [H][W] for the 16-bit greyscale modes (and for "I" with every value in [0, 65535]), else uint8 [H][W]
    through `convert("L")`.  The dtype says which scale applies (/ 65535 or / 255)."""
    if image.mode in _MODES_16:
        return np.ascontiguousarray(np.asarray(image).astype(np.uint16))       # native byte order, whatever the file's
    if image.mode == "I":
        arr = np.asarray(image)
        if arr.size and int(arr.min()) >= 0 and int(arr.max()) <= 65535:
            return np.ascontiguousarray(arr.astype(np.uint16))
    return np.ascontiguousarray(np.asarray(image.convert("L"), dtype=np.uint8))


def unit_float(arr: np.ndarray) -> np.ndarray:
    """decode16's array -> float32 in [0, 1]: one fp32 division by 65535 (uint16) or 255 (uint8)."""
    return arr.astype(np.float32) / np.float32(65535.0 if arr.dtype == np.uint16 else 255.0)


def resize_f(x: np.ndarray, size_hw: Tuple[int, int]) -> np.ndarray:
    """float32 [H][W] -> float32 [size_hw] by Pillow's mode "F" bicubic resample, then clipped to [0, 1]."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.shape != tuple(size_hw):
        x = np.asarray(Image.fromarray(x).resize((size_hw[1], size_hw[0]), Image.BICUBIC), dtype=np.float32)
    return np.clip(x, np.float32(0), np.float32(1))


def to_u16(x: np.ndarray) -> np.ndarray:
    """`(uint16)(clip(x, 0, 1) * 65535.0f + 0.5f)`, the multiply and the add each rounded in fp32."""
    t = np.clip(x.astype(np.float32), np.float32(0), np.float32(1)) * np.float32(65535.0)
    return (t + np.float32(0.5)).astype(np.uint16)


def image_from_u16(arr: np.ndarray) -> Image.Image:
    """uint16 [H][W] -> a PIL image of mode "I;16" (saved as a 16-bit greyscale PNG)."""
    return Image.fromarray(np.ascontiguousarray(arr, dtype=np.uint16))


def png_bytes_u16(arr: np.ndarray) -> bytes:
    buffered = io.BytesIO()
    image_from_u16(arr).save(buffered, format="PNG")
    return buffered.getvalue()
