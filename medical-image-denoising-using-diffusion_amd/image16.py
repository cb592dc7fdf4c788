"""The 16-bit image recipe either side of the sampler, host side (include/midd.h: THE FLOAT RESIZE AND THE 16-BIT ELEMENT RULES).

Not in the reference, whose every path squeezes an image through 256 grey levels (`convert("L")` in, `(x * 255).astype(uint8)`
out): a 16-bit PNG is decoded to its 65536 levels, scaled to unit float, resampled by Pillow in mode "F" (its 32bpc resample, not
its "I;16" one, which wraps the low byte on overshoot), clipped, and stored back as u16 rounded to nearest.  These functions are the
recipe with Pillow and numpy; `prepost.resize_bicubic_f32` / `u16_to_unit_float` / `to_u16` are the same arithmetic on the GPU, bit
for bit.  recipe.py picks the side its tensors live on, for cli.py and server.py alike.

`window_levels` / `unit_float_window` / `to_u16_window` are the host twins of the window (include/midd.h: THE WINDOW;
`prepost.window_levels` / `window_u16_to_float` / `window_to_u16` on the GPU): the grey range [lo, hi] between two percentiles of the
image in the place of [0, 65535].  Values outside the window come back as lo or hi.
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


# ------------------------------------------------------------------------------ the window (include/midd.h: THE WINDOW)
class WindowInputError(ValueError):
    """A window was asked for on a file that is not 16-bit (the service answers 400)."""


def check_percentiles(percentiles) -> Tuple[float, float]:
    """(p_lo, p_hi): finite, 0 <= p_lo < p_hi <= 100."""
    try:
        p_lo, p_hi = (float(p) for p in percentiles)
    except (TypeError, ValueError):
        raise ValueError(f"a window is two percentiles (p_lo, p_hi), got {percentiles!r}") from None
    if not (np.isfinite(p_lo) and np.isfinite(p_hi) and 0.0 <= p_lo < p_hi <= 100.0):
        raise ValueError(f"window percentiles must satisfy 0 <= p_lo < p_hi <= 100 (got {p_lo}, {p_hi})")
    return p_lo, p_hi


def check_levels(levels) -> Tuple[int, int]:
    """(lo, hi): integers with 0 <= lo < hi <= 65535."""
    try:
        lo, hi = levels
        if int(lo) != lo or int(hi) != hi:
            raise ValueError
        lo, hi = int(lo), int(hi)
    except (TypeError, ValueError):
        raise ValueError(f"window levels are two integers (lo, hi), got {levels!r}") from None
    if not 0 <= lo < hi <= 65535:
        raise ValueError(f"window levels must satisfy 0 <= lo < hi <= 65535 (got {lo}, {hi})")
    return lo, hi


def parse_pair(text: str, what: str) -> Tuple[float, float]:
    """"A,B" -> (A, B) as floats, for --window / --window-levels / MIDD_WINDOW."""
    parts = str(text).split(",")
    if len(parts) != 2:
        raise ValueError(f"{what} takes two comma-separated numbers, got {text!r}")
    try:
        return float(parts[0]), float(parts[1])
    except ValueError:
        raise ValueError(f"{what} takes two comma-separated numbers, got {text!r}") from None


def need_u16(arr: np.ndarray, mode: str) -> np.ndarray:
    """decode16's array under a window: it has to be the uint16 one."""
    if arr.dtype != np.uint16:
        raise WindowInputError(f"a window needs a 16-bit greyscale file, this one has mode {mode!r} (decoded to 8 bits); "
                               "leave the window out for such a file")
    return arr


def window_levels(arr: np.ndarray, percentiles=(0.5, 99.5)) -> Tuple[int, int]:
    """uint16 [H][W] -> (lo, hi): the 0-based order statistics at rank floor(p * (N - 1) / 100) of the two percentiles (the multiply
    and the divide in double), from the 65536-bin histogram; hi == lo becomes hi = lo + 1 (lo = hi - 1 at 65535)."""
    p_lo, p_hi = check_percentiles(percentiles)
    if arr.dtype != np.uint16 or arr.size < 1:
        raise ValueError("window_levels: a non-empty uint16 array expected")
    cum = np.cumsum(np.bincount(arr.ravel(), minlength=65536).astype(np.uint64))
    total = int(cum[-1])

    def level(p: float) -> int:
        r = int(np.floor(np.float64(p) * np.float64(total - 1) / np.float64(100.0)))
        return int(np.searchsorted(cum, np.uint64(r), side="right"))       # the smallest k with cum[k] > r

    lo, hi = level(p_lo), level(p_hi)
    if hi == lo:
        if lo < 65535:
            hi = lo + 1
        else:
            lo = hi - 1
    return lo, hi


def unit_float_window(arr: np.ndarray, levels) -> np.ndarray:
    """uint16 -> float32 in [0, 1]: clip((v - lo) / (float)(hi - lo), 0, 1), the difference exact, one fp32 division."""
    lo, hi = check_levels(levels)
    x = (arr.astype(np.int32) - np.int32(lo)).astype(np.float32) / np.float32(hi - lo)
    return np.clip(x, np.float32(0), np.float32(1))


def to_u16_window(x: np.ndarray, levels) -> np.ndarray:
    """`(uint16)(lo + (uint32)(clip(x, 0, 1) * d + 0.5f))`, d = (float)(hi - lo), the multiply and the add each rounded in fp32; a
    NaN stores lo."""
    lo, hi = check_levels(levels)
    x = np.asarray(x, dtype=np.float32)
    x = np.where(x > np.float32(0), np.minimum(x, np.float32(1)), np.float32(0)).astype(np.float32)    # NaN > 0 is false
    t = x * np.float32(hi - lo) + np.float32(0.5)
    return (np.uint32(lo) + t.astype(np.uint32)).astype(np.uint16)


def image_from_u16(arr: np.ndarray) -> Image.Image:
    """uint16 [H][W] -> a PIL image of mode "I;16" (saved as a 16-bit greyscale PNG)."""
    return Image.fromarray(np.ascontiguousarray(arr, dtype=np.uint16))


def png_bytes_u16(arr: np.ndarray) -> bytes:
    buffered = io.BytesIO()
    image_from_u16(arr).save(buffered, format="PNG")
    return buffered.getvalue()
