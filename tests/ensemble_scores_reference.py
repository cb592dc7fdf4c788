"""numpy restatement of the scores of an ensemble against a truth image (include/midd.h: THE ENSEMBLE SCORES), literally: the
member-order mean and variance of tests/ensemble_reference.py, the total-order sort and the quantiles of tests/quantile_reference.py,
the two sorted-order CRPS sums, the integer mid-rank, and the per-image double sums in the specification's one order (chunks of 1024
elements, four consecutive elements a lane, the fixed tree over the 256 lanes, the chunk sums one by one).  numpy's float64
element-wise operations round every operation on its own.  The device kernel is held to this bit for bit
(tests/test_gpu_ensemble_scores.py); tests/test_ensemble_scores_cpu.py holds this file to brute-force definitions."""
from typing import NamedTuple, Optional

import numpy as np

from tests import ensemble_reference
from tests import quantile_reference as qref

QNAN = np.uint32(0x7FC00000)
CHUNK, LANES = 1024, 256
MAX_MEMBERS, MAX_LEVELS = 64, 8


class Scores(NamedTuple):
    sums: np.ndarray            # float64 [B, 4] = (A, G, E, V)
    invalid: np.ndarray         # int64 [B]
    rank_hist: np.ndarray       # int64 [B, 2K+1]
    counts: np.ndarray          # int64 [B, nq, 2] = (y < Q, y <= Q)
    crps_map: np.ndarray        # float32 [B, chw]; 0x7FC00000 where invalid
    pixel: np.ndarray           # float64 [B, 4, chw]: the per-pixel a, g, se, var (0 where invalid) -- what the sums add
    valid: np.ndarray           # bool [B, chw]


def ordered_sum(t):
    """float64 [B, chw] -> [B]: the sum in the specification's order.  Absent and invalid pixels are +0.0 here: a lane's sum starts at
    +0.0 and so is never -0.0, hence adding +0.0 changes no bit."""
    B, n = t.shape
    chunks = (n + CHUNK - 1) // CHUNK
    pad = np.zeros((B, chunks * CHUNK), np.float64)
    pad[:, :n] = t
    lane4 = pad.reshape(B, chunks, LANES, 4)
    v = np.zeros((B, chunks, LANES), np.float64)
    for p in range(4):                                  # lane j: elements 4j .. 4j+3 in that order, from 0
        v = v + lane4[..., p]
    off = LANES // 2
    while off >= 1:                                     # v[j] += v[j + off] for j < off
        v[..., :off] = v[..., :off] + v[..., off:2 * off]
        off //= 2
    s = np.zeros(B, np.float64)
    for c in range(chunks):                             # chunk sums one by one from 0
        s = s + v[:, c, 0]
    return s


def scores(samples, truth, q=()) -> Scores:
    """samples float32 [B, K, ...], truth float32 [B, ...], levels q (0 .. 8 numbers in [0, 1])."""
    x = np.ascontiguousarray(samples, dtype=np.float32)
    B, K = x.shape[:2]
    x = x.reshape(B, K, -1)
    y = np.ascontiguousarray(truth, dtype=np.float32).reshape(B, -1)
    n = y.shape[1]
    levels = [float(v) for v in q]
    assert x.shape[2] == n and 1 <= K <= MAX_MEMBERS and len(levels) <= MAX_LEVELS and all(0.0 <= v <= 1.0 for v in levels)
    valid = np.isfinite(y) & np.isfinite(x).all(axis=1)
    y64 = y.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        # mean and variance: mi_ensemble_reduce's arithmetic in member order
        s = np.zeros((B, n), np.float64)
        for m in range(K):
            s = s + x[:, m].astype(np.float64)
        mean64 = s / np.float64(K)
        v = np.zeros((B, n), np.float64)
        for m in range(K):
            d = x[:, m].astype(np.float64) - mean64
            v = v + d * d
        var = v / np.float64(K - 1) if K > 1 else np.zeros((B, n), np.float64)
        dm = mean64 - y64
        se = dm * dm
        # the CRPS terms in sorted order
        srt = qref.sort_members(x, axis=1)
        a = np.zeros((B, n), np.float64)
        g = np.zeros((B, n), np.float64)
        for i in range(K):
            sv = srt[:, i].astype(np.float64)
            a = a + np.abs(sv - y64)
            g = g + np.float64(2 * i - K + 1) * sv
        c = a / np.float64(K) - g / np.float64(K * K)
        crps_map = c.astype(np.float32)
        crps_map.view(np.uint32)[~valid] = QNAN
        # rank: float comparisons
        lt = (x < y[:, None]).sum(axis=1)
        eq = (x == y[:, None]).sum(axis=1)
        bins = 2 * lt + eq
        rank_hist = np.zeros((B, 2 * K + 1), np.int64)
        for b in range(B):
            rank_hist[b] = np.bincount(bins[b][valid[b]], minlength=2 * K + 1)
        counts = np.zeros((B, len(levels), 2), np.int64)
        if levels:
            Q = qref.quantiles(x, levels)                # float32 [B, nq, n], the bits of mi_ensemble_quantiles
            for i in range(len(levels)):
                counts[:, i, 0] = ((y < Q[:, i]) & valid).sum(axis=1)
                counts[:, i, 1] = ((y <= Q[:, i]) & valid).sum(axis=1)
    pixel = np.stack([np.where(valid, t, 0.0) for t in (a, g, se, var)], axis=1)
    sums = np.stack([ordered_sum(pixel[:, k]) for k in range(4)], axis=1)
    return Scores(sums, (~valid).sum(axis=1).astype(np.int64), rank_hist, counts, crps_map, pixel, valid)


def compose(sums, invalid, K, chw):
    """The host's scalars from the raw outputs, in Python floats: per image (crps, crps_fair, rmse, spread)."""
    out = []
    for (A, G, E, V), inv in zip(np.asarray(sums, np.float64).tolist(), np.asarray(invalid).tolist()):
        N = chw - int(inv)
        nan = float("nan")
        out.append((A / (K * N) - G / (K * K * N) if N else nan,
                    A / (K * N) - G / (K * (K - 1) * N) if N and K > 1 else nan,
                    (E / N) ** 0.5 if N else nan, (V / N) ** 0.5 if N else nan))
    return out


def philox_case(B, K, chw, seed=2024, special: Optional[bool] = True):
    """Seeded inputs (the Philox normal of tests/ensemble_reference.py): truth and members are clip(base + 0.35 n, 0, 1) around a
    smooth base in [0, 1], which ties about a quarter of the pixels with the truth at the clamp.  ``special`` plants, where the image
    is long enough: exact 0 and 1 columns, -0.0 members against a +0.0 truth, a truth equal to one member, a NaN member and an
    infinite truth pixel (the last two only in image 0 and, if there is one, image 1: every image keeps valid pixels)."""
    e = np.arange(chw, dtype=np.uint64)
    base = 0.5 + 0.5 * np.sin(0.37 * np.arange(chw) + 0.1)
    y = np.empty((B, chw), np.float32)
    x = np.empty((B, K, chw), np.float32)
    for b in range(B):
        y[b] = np.clip(base + 0.35 * ensemble_reference.normal(seed, b, 0, e, 0), 0.0, 1.0).astype(np.float32)
        for m in range(K):
            x[b, m] = np.clip(base + 0.35 * ensemble_reference.normal(seed, b, 1, e, m), 0.0, 1.0).astype(np.float32)
    if special:
        if chw > 2:
            x[:, :, 2] = 0.0; y[:, 2] = 0.0                       # all tied at 0
        if chw > 3:
            x[:, :, 3] = 1.0; y[:, 3] = 1.0                       # all tied at 1
        if chw > 4:
            x[:, :, 4] = np.float32(-0.0); y[:, 4] = 0.0          # -0.0 == +0.0 in the rank, -0.0 < +0.0 in the sort
        if chw > 7:
            y[:, 7] = x[:, K // 2, 7]                             # truth equal to a member
        if chw > 9:
            x[0, K - 1, 9] = np.nan                               # an invalid pixel: NaN member
        if chw > 11:
            y[min(1, B - 1), 11] = np.inf                         # an invalid pixel: infinite truth
        if chw > 1030:
            x[0, 0, 1030] = -np.inf                               # one in the second chunk
    return x, y
