"""Time of the ensemble-scores launch next to the two existing launches over the same members, in one process:

    mi_ensemble_scores     (five levels, no crps_map; a second arm with the map)
    mi_ensemble_quantiles  (the same five levels)
    mi_ensemble_reduce     (mean and std)

for one 256x256 image with K = 8 and K = 32 members, a batch of 8 at 256x256 with K = 8, one 2500x2048 image with K = 8, and -- for
the largest sort network -- one 256x256 image with K = 64.  No network runs: truth and members are clip(0.5 + 0.35 n, 0, 1), which
ties a share of the pixels at the clamp as real outputs do (the sort network is data-independent, the rank counters in LDS are
not).  Every launch is the C call with preallocated outputs; `n` launches sit between two events, the arms alternate (reduce,
quantiles, scores, ...) so that clock drift hits all alike, and median [min - max] of at least 5 timed windows is reported, never a
single run.  Beside every time stand the bytes the launch must read and write and, measured in the same windows, a device copy of
as many bytes as the members hold (read once, written once): the rate the memory system gives a plain stream of that size.

    python tools/ensemble_scores_ab.py [--reps 5] [--warmup 2] [--out profiles/ensemble_scores_ab.json]

Writes ONE JSON object (and prints it); `mi_source_hash` names the library build the numbers belong to."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import midd_loader  # noqa: E402

midd_loader.load()
import midd_amd  # noqa: E402
from midd_amd import native  # noqa: E402

LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)
SHAPES = [(1, 256, 256, 8), (1, 256, 256, 32), (8, 256, 256, 8), (1, 2500, 2048, 8), (1, 256, 256, 64)]      # (B, H, W, K)


def windows(arms, n, reps, warmup):
    """arms: name -> launch function; -> name -> us per launch of every timed window, the arms alternating."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = {name: [] for name in arms}
    for rep in range(warmup + reps):
        for name, fn in arms.items():
            ev[0].record()
            for _ in range(n):
                fn()
            ev[1].record()
            ev[1].synchronize()
            if rep >= warmup:
                per[name].append(1e3 * ev[0].elapsed_time(ev[1]) / n)
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed windows per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_scores_ab.json"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_scores_ab.py needs a GPU")
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    q = (C.c_double * len(LEVELS))(*LEVELS)
    nq = len(LEVELS)
    gen = torch.Generator(device="cuda").manual_seed(7)
    rows = []
    for B, H, W, K in SHAPES:
        chw = H * W
        n = 100 if chw * B * K <= (1 << 24) else 20
        samples = (0.5 + 0.35 * torch.randn((B, K, 1, H, W), device="cuda", generator=gen)).clamp_(0, 1)
        truth = (0.5 + 0.35 * torch.randn((B, 1, H, W), device="cuda", generator=gen)).clamp_(0, 1)
        copy_dst = torch.empty_like(samples)
        mean, std, cmap = (torch.empty_like(truth) for _ in range(3))
        maps = torch.empty((B, nq, 1, H, W), device="cuda")
        raw = torch.zeros(B * (4 + 1 + 2 * K + 1 + 2 * nq), dtype=torch.int64, device="cuda")
        base = raw.data_ptr()
        o_inv, o_rank, o_cnt = base + 8 * B * 4, base + 8 * B * 5, base + 8 * B * (5 + 2 * K + 1)
        ws_bytes = lib.mi_ensemble_scores_workspace_bytes(B, K, chw)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")

        def reduce():
            native.check(lib.mi_ensemble_reduce(samples.data_ptr(), B, K, chw, mean.data_ptr(), std.data_ptr(), stream))

        def quantiles():
            native.check(lib.mi_ensemble_quantiles(samples.data_ptr(), B, K, chw, q, nq, maps.data_ptr(), stream))

        def scores(with_map=False):
            native.check(lib.mi_ensemble_scores(samples.data_ptr(), truth.data_ptr(), B, K, chw, q, nq, base, o_inv, o_rank, o_cnt,
                                                cmap.data_ptr() if with_map else None, ws.data_ptr(), ws_bytes, stream))

        def copy():
            copy_dst.copy_(samples)

        plane = B * chw * 4
        nbytes = {"reduce": (K + 2) * plane, "quantiles": (K + nq) * plane, "scores": (K + 1) * plane + ws_bytes,
                  "scores_with_map": (K + 2) * plane + ws_bytes, "copy": 2 * K * plane}
        per = windows({"reduce": reduce, "quantiles": quantiles, "scores": scores, "scores_with_map": lambda: scores(True), "copy": copy},
                      n, a.reps, a.warmup)
        row = {"shape": [B, 1, H, W], "members": K, "levels": list(LEVELS), "launches_per_timed_window": n}
        for name, t in per.items():
            med = statistics.median(t)
            row[name] = {"us_per_launch": {"median": med, "min": min(t), "max": max(t)}, "algorithmic_bytes": nbytes[name],
                         "GB_per_s_at_median": nbytes[name] / (med * 1e-6) / 1e9}
        row["scores_over_quantiles_time"] = row["scores"]["us_per_launch"]["median"] / row["quantiles"]["us_per_launch"]["median"]
        row["scores_over_reduce_time"] = row["scores"]["us_per_launch"]["median"] / row["reduce"]["us_per_launch"]["median"]
        # what the launch answered, composed as the Python call composes it (one image of the batch)
        sc = midd_amd.ensemble_scores(samples, truth, LEVELS)
        row["result_image_0"] = {"crps": float(sc.crps[0]), "crps_fair": float(sc.crps_fair[0]), "rmse": float(sc.rmse[0]),
                                 "spread": float(sc.spread[0]), "coverage_5_95": float(sc.coverage()[0])}
        rows.append(row)
        del samples, truth, copy_dst, maps, ws
    out = {
        "tool": "tools/ensemble_scores_ab.py",
        "metric": "time per launch of mi_ensemble_scores (five levels; the call is three launches: zero the counters, score, add the chunk sums) beside "
                  "mi_ensemble_quantiles (five levels) and mi_ensemble_reduce (mean and std) on the same members, and a device copy of the "
                  "members, alternating in one process; compulsory bytes: every member and the truth once, every output once",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "data": "clip(0.5 + 0.35 n, 0, 1): members and truth tie at the clamp", "rows": rows}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
