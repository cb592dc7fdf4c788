"""Pure-numpy restatement of the ensemble part of the specification (include/midd.h: mi_denoise_ensemble, mi_ensemble_reduce;
DESIGN.md section 6b): the member-keyed step noise -- tests/step_noise_reference.py with the fourth Philox counter word set to
the member index -- and the fixed double-precision arithmetic of the reduce kernel.  Float64 and exact integers throughout: the
yardstick, not an emulation of the device."""
import numpy as np

from tests.step_noise_reference import philox4x32_10


def normal(seed, sample, iteration, elements, member=0):
    """float64 z for one (seed, global image index, iteration index, member index) and an array of element indices."""
    e = np.asarray(elements, np.uint64)
    x0, x1, _, _ = philox4x32_10((e, int(sample) & 0xFFFFFFFF, int(iteration) & 0xFFFFFFFF, int(member) & 0xFFFFFFFF),
                                 (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    u1 = ((x0 >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24          # (0, 1]
    u2 = (x1 >> np.uint64(8)).astype(np.float64) * 2.0 ** -24                            # [0, 1)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def step_noise(seed, n_iters, shape, sample_offset=0, member=0):
    """float64 [n_iters, B, C, H, W]: 0.5 * z of member `member` of every image, what midd_amd.step_noise(member=) returns in fp32."""
    B, C, H, W = shape
    e = np.arange(C * H * W, dtype=np.uint64)
    out = np.empty((n_iters, B, C * H * W), np.float64)
    for i in range(n_iters):
        for b in range(B):
            out[i, b] = 0.5 * normal(seed, sample_offset + b, i, e, member)
    return out.reshape(n_iters, B, C, H, W)


def reduce(samples):
    """samples float32 [B, K, ...] -> (mean float32 [B, ...], std float32 [B, ...] or None for K == 1) with the kernel's
    arithmetic: members added in index order in float64, one division, deviations from the float64 mean, unbiased."""
    x = np.asarray(samples)
    assert x.dtype == np.float32 and x.ndim >= 3
    K = x.shape[1]
    s = np.zeros((x.shape[0],) + x.shape[2:], np.float64)
    for m in range(K):
        s = s + x[:, m].astype(np.float64)
    mean64 = s / np.float64(K)
    if K < 2:
        return mean64.astype(np.float32), None
    q = np.zeros_like(s)
    for m in range(K):
        d = x[:, m].astype(np.float64) - mean64
        q = q + d * d
    return mean64.astype(np.float32), np.sqrt(q / np.float64(K - 1)).astype(np.float32)
