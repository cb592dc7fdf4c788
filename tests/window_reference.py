"""The window of the 16-bit path (include/midd.h: THE WINDOW) restated in numpy: the histogram, the levels at two percentiles, and the
two element rules in float32.  The HIP kernels (csrc/prepost.hip) and the host recipe (image16.py) are compared with this file bit for
bit; it shares no code with either."""
import numpy as np

BINS = 65536


def histogram(image: np.ndarray) -> np.ndarray:
    """uint16 array (one image) -> uint32 [65536]: the number of pixels of every value."""
    assert image.dtype == np.uint16
    return np.bincount(image.ravel().astype(np.int64), minlength=BINS).astype(np.uint32)


def rank(p: float, total: int) -> int:
    """floor(p * (double)(N - 1) / 100.0): the multiply and the divide in double, each rounded on its own."""
    t = np.float64(p) * np.float64(total - 1)
    return int(np.floor(t / np.float64(100.0)))


def flat_rule(lo: int, hi: int):
    if hi == lo:
        if lo < BINS - 1:
            hi = lo + 1
        else:
            lo = hi - 1
    return lo, hi


def levels(image: np.ndarray, p_lo: float, p_hi: float):
    """(lo, hi): the 0-based order statistics at the two ranks, on the sorted pixels, then the flat rule."""
    s = np.sort(image.ravel())
    return flat_rule(int(s[rank(p_lo, s.size)]), int(s[rank(p_hi, s.size)]))


def levels_from_histogram(hist: np.ndarray, p_lo: float, p_hi: float):
    """The same levels by the rule as the header words it: the smallest k with h[0] + ... + h[k] > r."""
    total = int(hist.astype(np.uint64).sum())
    out = []
    for p in (p_lo, p_hi):
        r, cum = rank(p, total), 0
        for k in np.flatnonzero(hist):
            cum += int(hist[k])
            if cum > r:
                out.append(int(k))
                break
    return flat_rule(*out)


def load(v: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """x = min(max((float)((int)v - lo) / d, 0), 1), d = (float)(hi - lo): one fp32 division."""
    d = np.float32(hi - lo)
    x = (v.astype(np.int64) - lo).astype(np.float32) / d
    return np.minimum(np.maximum(x, np.float32(0)), np.float32(1)).astype(np.float32)


def store(x: np.ndarray, lo: int, hi: int) -> np.ndarray:
    """v = (uint16)(lo + (uint32)(min(max(x, 0), 1) * d + 0.5f)), the multiply and the add each rounded in fp32; a NaN stores lo."""
    d = np.float32(hi - lo)
    x = np.asarray(x, dtype=np.float32)
    c = np.where(np.isnan(x), np.float32(0), np.minimum(np.maximum(x, np.float32(0)), np.float32(1))).astype(np.float32)
    t = (c * d).astype(np.float32)
    t = (t + np.float32(0.5)).astype(np.float32)
    return (lo + t.astype(np.int64)).astype(np.uint16)
