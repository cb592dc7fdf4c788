"""Pure-numpy restatement of the seeded step-noise specification (include/midd.h: mi_denoise_seeded).

Philox4x32-10 as in Random123 (Salmon et al., SC'11), one call per element with the counter
(element index, global sample index, iteration index, 0) and the key (seed low word, seed high word); outputs x0, x1 feed a
Box-Muller cosine branch.  Everything here is float64 / exact integers: it is the yardstick the device's fp32 values are
compared with, not an emulation of them."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # key increments (golden ratio, sqrt(3) - 1)
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two -> four uint64 arrays holding the 32-bit output words."""
    c = [np.asarray(v, np.uint64) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]            # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def normal(seed, sample, iteration, elements):
    """float64 z of the specification for one (seed, global sample index, iteration index) and an array of element indices."""
    e = np.asarray(elements, np.uint64)
    x0, x1, _, _ = philox4x32_10((e, int(sample) & 0xFFFFFFFF, int(iteration) & 0xFFFFFFFF, 0),
                                 (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1 = ((x0 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24          # (0, 1]
    u2 = (x1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24                            # [0, 1)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def step_noise(seed, n_iters, shape, sample_offset=0):
    """float64 [n_iters, B, C, H, W]: 0.5 * z, what midd_amd.step_noise returns in fp32."""
    B, C, H, W = shape
    e = np.arange(C * H * W, dtype=np.uint64)
    out = np.empty((n_iters, B, C * H * W), np.float64)
    for i in range(n_iters):
        for b in range(B):
            out[i, b] = 0.5 * normal(seed, sample_offset + b, i, e)
    return out.reshape(n_iters, B, C, H, W)
