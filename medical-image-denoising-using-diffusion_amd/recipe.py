"""The image recipe either side of the sampler, once: a decoded file -> the sampler's [1, 1, H, W] float tensor -> a file's array.

Three kinds, chosen by ``ImageRecipe(bit_depth, window / window_levels)``:
  8           the reference's recipe: `convert("L")`, 8-bit bicubic resize, / 255; back: x 255 truncated, 8-bit bicubic resize;
  16          decode16 (/ 65535 for a 16-bit file, `convert("L")` / 255 for any other), float bicubic resize, clip; back: float
              resize, clip, u16 rounded to nearest (include/midd.h: THE FLOAT RESIZE);
  16 + window the same with the grey range [lo, hi] of the file in the place of [0, 65535] (include/midd.h: THE WINDOW).
Each kind has two sides that agree bit for bit: the host (Pillow / numpy, image16.py) and the GPU (the HIP kernels, prepost.py).
``load`` takes the side from the device it is given, ``store`` from the tensor's; cli.py and server.py make no such choice.  A
target of the image's own size resamples nothing: the same calls are then the pure conversions.
"""
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch
from PIL import Image

from . import image16, prepost


class Source(NamedTuple):
    """The way back of a loaded image.  ``levels``: the window's (lo, hi) -- on the GPU an int32 [1, 2] tensor that stays there
    (nothing waits for it), on the host a tuple; None without a window."""
    size: Tuple[int, int]              # PIL order: (width, height)
    is_u16: Optional[bool] = None      # the file decoded to 16 bits (False: to 8, scaled by / 255)
    levels: object = None

    def as_tuple(self) -> tuple:
        """(width, height), or (width, height, levels) under a window: what the service hands from preprocess to the way back."""
        return self.size if self.levels is None else self.size + (self.levels,)

    @classmethod
    def of(cls, size) -> "Source":
        return cls(tuple(size[:2]), None, *size[2:3])


class ImageRecipe:
    def __init__(self, bit_depth: int = 8, window=None, window_levels=None):
        """window: two percentiles (p_lo, p_hi) whose levels are read off each image's histogram; window_levels: the two levels
        themselves.  At most one of the two, and bit_depth 16 with either."""
        self.bit_depth = image16.check_bit_depth(bit_depth)
        if window is not None and window_levels is not None:
            raise ValueError("window and window_levels cannot be combined: percentiles or absolute levels, not both")
        self.window = None if window is None else image16.check_percentiles(window)
        self.window_levels = None if window_levels is None else image16.check_levels(window_levels)
        self.windowed = window is not None or window_levels is not None
        if self.windowed and self.bit_depth != 16:
            raise ValueError("a window needs bit_depth=16 (the window acts on 16-bit uploads)")

    def load(self, image: Image.Image, target: Optional[Tuple[int, int]], device, levels=None) -> Tuple[torch.Tensor, Source]:
        """A decoded image -> (float32 [1, 1, H, W] in [0, 1] on `device`, its Source).  target: (H, W), None for the image's own.
        levels: another image's window levels in the place of this one's (the clean counterpart of a noisy image)."""
        device = torch.device(device)
        raw = image16.decode16(image) if self.bit_depth == 16 else np.asarray(image.convert("L"), dtype=np.uint8).copy()
        if self.windowed:
            raw = image16.need_u16(raw, image.mode)
        size = raw.shape if target is None else (int(target[0]), int(target[1]))
        if device.type == "cuda":
            dev = torch.from_numpy(raw).to(device, non_blocking=True)
            if self.windowed and levels is None:
                levels = (prepost.window_levels(dev, self.window) if self.window is not None
                          else torch.tensor([list(self.window_levels)], dtype=torch.int32, device=device))
            if self.windowed:         # windowed load, float resize, clip: one fused call under the levels on the device
                x = prepost.resize_bicubic_f32(dev, size, clamp=True, levels=levels)
            elif self.bit_depth == 16:      # typed load, float resize, clip: one fused call
                x = prepost.resize_bicubic_f32(dev, size, clamp=True)
            else:
                x = prepost.to_unit_float(prepost.resize_bicubic_u8(dev, size))
        else:
            if self.windowed and levels is None:
                levels = image16.window_levels(raw, self.window) if self.window is not None else self.window_levels
            if self.windowed:
                x = image16.resize_f(image16.unit_float_window(raw, levels), size)
            elif self.bit_depth == 16:
                x = image16.resize_f(image16.unit_float(raw), size)
            else:                     # transforms.Resize on a PIL image, ToTensor
                x = image16.unit_float(raw if size == raw.shape else _resize_u8(raw, size))
            x = torch.from_numpy(x)
        return x[None, None], Source(image.size, raw.dtype == np.uint16, levels if self.windowed else None)

    def store(self, tensor: torch.Tensor, source: Source) -> np.ndarray:
        """[.., H, W] (one plane) in [0, 1] -> uint8 (bit_depth 8) or uint16 [height][width] at the source's size."""
        plane = tensor.reshape(tensor.shape[-2], tensor.shape[-1]).float()
        size = (source.size[1], source.size[0])
        if plane.is_cuda:
            if self.bit_depth == 16:      # float resize back, clip, (windowed) store: one fused call
                return prepost.resize_bicubic_f32(plane, size, clamp=True, out_dtype=torch.uint16, levels=source.levels).cpu().numpy()
            return prepost.resize_bicubic_u8(prepost.to_u8(plane), size).cpu().numpy()
        x = plane.numpy()
        if source.levels is not None:
            return image16.to_u16_window(image16.resize_f(x, size), source.levels)
        if self.bit_depth == 16:
            return image16.to_u16(image16.resize_f(x, size))
        u8 = (x * 255).astype(np.uint8)       # truncation, as the reference; the sampler's output is already in [0, 1]
        return u8 if size == u8.shape else _resize_u8(u8, size)


def _resize_u8(arr: np.ndarray, size_hw: Tuple[int, int]) -> np.ndarray:
    return np.asarray(Image.fromarray(arr, mode="L").resize((size_hw[1], size_hw[0]), Image.BICUBIC), dtype=np.uint8)
