"""TEST INFRASTRUCTURE ONLY: numpy restatement of the high-bit-depth image path (include/midd.h: THE FLOAT RESIZE AND THE
16-BIT ELEMENT RULES).  Imports nothing from the package.

  * resize_bicubic_f32: Pillow's 32bpc resample, `Image.fromarray(a, mode "F").resize((dw, dh), Image.BICUBIC)`: separable,
    horizontal pass first, a pass whose size does not change is skipped, double-precision coefficients normalised by their sum,
    `double ss = 0; ss += (double)pixel * k` in tap order (every operation rounded on its own), float32 between the passes,
    nothing clipped.  PINNED against Pillow itself in tests/test_prepost16_cpu.py.
  * load / store: the element rules (u8 / 255, u16 / 65535 in fp32; u16 store: clamp, fp32 multiply, fp32 add of .5, truncation).
  * recipe16_pre / recipe16_post: the 16-bit recipe either side of the sampler.
"""
import math

import numpy as np

U8, U16, F32 = 0, 1, 2          # MI_PIX_*


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0
    if x < 2.0:
        return (((x - 5.0) * x + 8.0) * x - 4.0) * a
    return 0.0


def coeffs(in_size: int, out_size: int):
    """-> (bounds [out][2] int32 (first tap, tap count), kk [out][ksize] float64, ksize)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    kk = np.zeros((out_size, ksize), np.float64)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            kk[xx, x] = w[x] / ww if ww != 0.0 else w[x]
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize


def _pass(img: np.ndarray, bounds: np.ndarray, kk: np.ndarray) -> np.ndarray:
    """Resamples the LAST axis of a float32 array."""
    assert img.dtype == np.float32
    out = np.empty(img.shape[:-1] + (bounds.shape[0],), np.float32)
    for xx in range(bounds.shape[0]):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        ss = np.zeros(img.shape[:-1], np.float64)
        for x in range(n):                                   # sequential: one rounded multiply, one rounded add per tap
            ss = ss + img[..., x0 + x].astype(np.float64) * kk[xx, x]
        out[..., xx] = ss.astype(np.float32)
    return out


def resize_bicubic_f32(img: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """float32 [..., H, W] -> float32 [..., out_h, out_w]."""
    assert img.dtype == np.float32 and img.ndim >= 2
    h, w = img.shape[-2:]
    cur = img
    if out_w != w:
        b, k, _ = coeffs(w, out_w)
        cur = _pass(cur, b, k)
    if out_h != h:
        b, k, _ = coeffs(h, out_h)
        cur = np.ascontiguousarray(np.swapaxes(_pass(np.ascontiguousarray(np.swapaxes(cur, -1, -2)), b, k), -1, -2))
    return cur


def load(a: np.ndarray) -> np.ndarray:
    """Source element rule: u8 / 255, u16 / 65535 (one fp32 division), f32 as is."""
    if a.dtype == np.uint8:
        return a.astype(np.float32) / np.float32(255.0)
    if a.dtype == np.uint16:
        return a.astype(np.float32) / np.float32(65535.0)
    assert a.dtype == np.float32
    return a


def clamp01(v: np.ndarray) -> np.ndarray:
    return np.minimum(np.maximum(v.astype(np.float32), np.float32(0)), np.float32(1))


def to_u16(v: np.ndarray) -> np.ndarray:
    """Destination u16: clamp, then (uint16)(v * 65535.0f + 0.5f), the multiply and the add each rounded in fp32."""
    t = clamp01(v) * np.float32(65535.0)
    assert t.dtype == np.float32
    return (t + np.float32(0.5)).astype(np.uint16)


def store(v: np.ndarray, dst_type: int, clamp: bool) -> np.ndarray:
    if dst_type == U16:
        return to_u16(v)
    assert dst_type == F32
    return clamp01(v) if clamp else v


def resize(a: np.ndarray, out_h: int, out_w: int, dst_type: int = F32, clamp: bool = False) -> np.ndarray:
    """The fused call, spelled as its separate steps: convert, resize, convert."""
    return store(resize_bicubic_f32(load(a), out_h, out_w), dst_type, clamp)


def recipe16_pre(arr: np.ndarray, size) -> np.ndarray:
    """decoded u16 (or u8) image [H][W] -> float32 [size[0]][size[1]] in [0, 1]."""
    return resize(arr, size[0], size[1], F32, True)


def recipe16_post(x: np.ndarray, out_h: int, out_w: int) -> np.ndarray:
    """sampler output float32 [h][w] -> uint16 [out_h][out_w]."""
    return resize(x.astype(np.float32), out_h, out_w, U16, True)
