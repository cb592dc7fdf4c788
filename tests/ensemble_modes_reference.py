"""numpy restatement of the principal modes of an ensemble's spread (include/midd.h: THE ENSEMBLE MODES), literally: the
member-order double mean of tests/ensemble_reference.py, the centred members, the rounded products d_i * d_j and their sums in the
specification's one order (chunks of 4096 elements; 16 rounds of 256, lane l owning elements 256 r + 4 l .. + 3 of round r and
adding its 64 products in element order; the fixed tree over the 64 lanes; the chunk sums one by one), and the projection onto
weight rows with k in index order.  numpy's float64 element-wise operations round every operation on its own.  The device kernels
are held to this bit for bit (tests/test_gpu_ensemble_modes.py); tests/test_ensemble_modes_cpu.py holds this file to float64
matrix products within the recursive-summation bound."""
from typing import NamedTuple

import numpy as np

from tests import ensemble_reference

QNAN = np.uint32(0x7FC00000)
CHUNK, LANES, ROUNDS = 4096, 64, 16
MAX_MEMBERS, MAX_MODES = 64, 8


class Gram(NamedTuple):
    gram: np.ndarray            # float64 [B, K, K], symmetric
    invalid: np.ndarray         # int64 [B]
    d: np.ndarray               # float64 [B, K, chw]: the centred members, 0 where the element is invalid
    valid: np.ndarray           # bool [B, chw]


def centre(samples):
    """float32 [B, K, ...] -> (d float64 [B, K, chw] with zeros at invalid elements, valid bool [B, chw])."""
    x = np.ascontiguousarray(samples, dtype=np.float32)
    B, K = x.shape[:2]
    x = x.reshape(B, K, -1)
    assert 2 <= K <= MAX_MEMBERS
    valid = np.isfinite(x).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros((B, x.shape[2]), np.float64)
        for m in range(K):                                  # mi_ensemble_reduce's mean: members in index order, one division
            s = s + x[:, m].astype(np.float64)
        mean64 = s / np.float64(K)
        d = x.astype(np.float64) - mean64[:, None]
    return np.where(valid[:, None], d, 0.0), valid


def ordered_sum(t):
    """float64 [..., chw] -> [...]: the sum over the last axis in the specification's order.  Absent and invalid elements are zeros
    here: a lane's sum starts at +0.0 and so is never -0.0, hence adding a zero of either sign changes no bit."""
    lead, n = t.shape[:-1], t.shape[-1]
    chunks = (n + CHUNK - 1) // CHUNK
    pad = np.zeros(lead + (chunks * CHUNK,), np.float64)
    pad[..., :n] = t
    own = pad.reshape(lead + (chunks, ROUNDS, LANES, 4))
    v = np.zeros(lead + (chunks, LANES), np.float64)
    for r in range(ROUNDS):                                 # lane l: elements 256 r + 4 l .. + 3, in element order, from 0
        for p in range(4):
            v = v + own[..., r, :, p]
    off = LANES // 2
    while off >= 1:                                         # v[l] += v[l + off] for l < off
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    s = np.zeros(lead, np.float64)
    for c in range(chunks):                                 # chunk sums one by one from 0
        s = s + v[..., c, 0]
    return s


def gram(samples) -> Gram:
    """samples float32 [B, K, ...] -> the Gram matrix of the centred members and the invalid counts."""
    d, valid = centre(samples)
    B, K, _ = d.shape
    g = np.zeros((B, K, K), np.float64)
    for i in range(K):
        row = ordered_sum(d[:, i:i + 1] * d[:, i:])          # the products rounded, then added: [B, K - i]
        g[:, i, i:] = row
        g[:, i:, i] = row
    return Gram(g, (~valid).sum(axis=1).astype(np.int64), d, valid)


def project(samples, weights):
    """samples float32 [B, K, ...], weights float64 [B, M, K] -> float32 [B, M, chw]; 0x7FC00000 at invalid elements."""
    d, valid = centre(samples)
    w = np.asarray(weights, dtype=np.float64)
    B, K, n = d.shape
    M = w.shape[1]
    assert w.shape == (B, M, K) and 1 <= M <= MAX_MODES
    a = np.zeros((B, M, n), np.float64)
    for k in range(K):
        a = a + w[:, :, k, None] * d[:, None, k]
    out = a.astype(np.float32)
    out.view(np.uint32)[np.broadcast_to(~valid[:, None], out.shape)] = QNAN
    return out


def philox_case(B, K, chw, seed=77, nan_at=None, inf_at=None):
    """Seeded members (the Philox normal of tests/ensemble_reference.py): a smooth base in [0, 1] plus a pattern shared by the
    members with a member-dependent amplitude plus independent noise, clipped to [0, 1] as the network's outputs are.  ``nan_at`` /
    ``inf_at``: (image, member, element) of a planted NaN / +inf."""
    e = np.arange(chw, dtype=np.uint64)
    t = np.arange(chw)
    base = 0.5 + 0.4 * np.sin(0.37 * t + 0.1)
    pattern = np.cos(0.011 * t)
    x = np.empty((B, K, chw), np.float32)
    for b in range(B):
        for m in range(K):
            amp = 0.05 * np.sin(1.3 * m + b)
            x[b, m] = np.clip(base + amp * pattern + 0.03 * ensemble_reference.normal(seed, b, 1, e, m), 0.0, 1.0).astype(np.float32)
    if nan_at is not None:
        x[nan_at] = np.nan
    if inf_at is not None:
        x[inf_at] = np.inf
    return x


def planted_case(H=32, W=32, K=16, seed=5):
    """The planted-structure ensemble: members base + a_k P1 + b_k P2 + 1e-3 noise on an H x W image.  P1 and P2 are orthonormal under
    the pixel mean, i.e. of unit RMS (a horizontal and a vertical half-period cosine; with unit SUM of squares a 0.04 amplitude would
    be 0.0018 grey levels a pixel, level with the 1e-3 noise, whose own Gram eigenvalues then shift the 4 : 1 ratio to about 3.6 : 1
    in exact arithmetic); a and b are zero-mean, mutually orthogonal, with sample std 0.04 and 0.02, so the
    two leading modes are 0.04 P1 and 0.02 P2 and their variances stand 4 : 1.  Returns (samples float32 [1, K, 1, H, W], P1, P2)."""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    p1 = np.cos(np.pi * (xx + 0.5) / W)
    p2 = np.cos(np.pi * (yy + 0.5) / H)
    p1, p2 = p1 / np.sqrt((p1 * p1).mean()), p2 / np.sqrt((p2 * p2).mean())      # orthonormal under <f, g> = mean(f g): a_k is in grey levels
    assert abs((p1 * p2).mean()) < 1e-12
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(K)
    a -= a.mean()
    b = rng.standard_normal(K)
    b -= b.mean()
    b -= a * (a @ b) / (a @ a)
    a *= 0.04 / a.std(ddof=1)
    b *= 0.02 / b.std(ddof=1)
    base = 0.5 + 0.2 * np.sin(0.2 * xx) * np.cos(0.15 * yy)
    noise = rng.standard_normal((K, H, W))
    x = base[None] + a[:, None, None] * p1[None] + b[:, None, None] * p2[None] + 1e-3 * noise
    return x.astype(np.float32)[None, :, None], p1, p2
