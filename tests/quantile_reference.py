"""numpy restatement of the quantile maps of an ensemble (include/midd.h: mi_ensemble_quantiles), literally: the total-order key
sort, then the interpolation in double precision with every operation rounded on its own (numpy's float64 element-wise
operations are).  The device kernels are held to this bit for bit (tests/test_gpu_quantiles.py)."""
import numpy as np

QNAN = np.uint32(0x7FC00000)
MAX_MEMBERS, MAX_LEVELS = 64, 8


def keys(x):
    """float32 -> the unsigned key whose integer order is -inf < ... < -0.0 < +0.0 < ... < +inf."""
    bits = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return bits ^ np.where(bits >> np.uint32(31) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkeys(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return (k ^ np.where(k >> np.uint32(31) != 0, np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def sort_members(x, axis=1):
    """The members of every pixel in the specification's total order (ties carry identical bits: the result is unique)."""
    return unkeys(np.sort(keys(x), axis=axis))


def quantiles(x, q, axis=1):
    """x float32 [B, K, ...] -> float32 [B, nq, ...]: the quantiles ``q`` over ``axis`` (1: the members)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert axis == 1 and x.ndim >= 2
    K = x.shape[1]
    levels = [float(v) for v in q]
    assert 1 <= K <= MAX_MEMBERS and 1 <= len(levels) <= MAX_LEVELS and all(0.0 <= v <= 1.0 for v in levels)
    s = sort_members(x, axis=1)
    has_nan = np.isnan(x).any(axis=1)
    out = np.empty((x.shape[0], len(levels)) + x.shape[2:], np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i, level in enumerate(levels):
            pos = np.float64(level) * np.float64(K - 1)
            lo = int(np.floor(pos))
            hi = min(lo + 1, K - 1)
            g = pos - np.float64(lo)
            s_lo, s_hi = s[:, lo].astype(np.float64), s[:, hi].astype(np.float64)
            diff = s_hi - s_lo
            prod = g * diff
            r = (s_lo + prod).astype(np.float32)
            out[:, i] = s[:, 0] if K == 1 else r
    bits = out.view(np.uint32)
    bits[np.isnan(out) | has_nan[:, None]] = QNAN
    return out
