"""Time of each quantile launch next to the existing reduce launch on the same tensors, in one process:

    mi_ensemble_quantiles    (three levels: 0.05, 0.5, 0.95)   beside   mi_ensemble_reduce with std      (the base)
    mi_tile_blend_quantiles  (the same three levels)           beside   mi_tile_blend_reduce with std    (the base)

at K = 8 and K = 32 members, for one 256x256 image, a batch of 8 at 256x256, and one 1024x1024 image as 5 x 5 tiles of 256
with overlap 32.  No network runs: the members are uniform random values, which is what a sort network costs the same for as
for real samples (it is data-independent).  Every launch is the C call with preallocated outputs; `n` launches sit between two
events, the arms are interleaved (reduce, quantiles, reduce, ...) so that clock drift hits both alike, and median [min - max] of
at least 5 timed windows is reported, never a single run.  These launches follow seconds of sampling in the calls that use
them: the figures say what the maps cost, not what a user waits for.

    python tools/quantiles_ab.py [--reps 5] [--warmup 2] > profiles/quantiles_ab.json

Prints ONE JSON object; `mi_source_hash` names the library build the numbers belong to."""
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

LEVELS = (0.05, 0.5, 0.95)
T, O = 256, 32
N_LAUNCHES = 100


def windows(arms, reps, warmup):
    """arms: name -> launch function; -> name -> us per launch of every timed window, the arms interleaved."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = {name: [] for name in arms}
    for rep in range(warmup + reps):
        for name, fn in arms.items():
            ev[0].record()
            for _ in range(N_LAUNCHES):
                fn()
            ev[1].record()
            ev[1].synchronize()
            if rep >= warmup:
                per[name].append(1e3 * ev[0].elapsed_time(ev[1]) / N_LAUNCHES)
    return per


def row(what, shape, K, arms, nbytes, reps, warmup):
    per = windows(arms, reps, warmup)
    out = {"case": what, "shape": shape, "members": K, "levels": list(LEVELS), "launches_per_timed_window": N_LAUNCHES}
    for name, t in per.items():
        med = statistics.median(t)
        out[name] = {"us_per_launch": {"median": med, "min": min(t), "max": max(t)}, "algorithmic_bytes": nbytes[name],
                     "GB_per_s_at_median": nbytes[name] / (med * 1e-6) / 1e9}
    out["quantiles_over_reduce_time"] = out["quantiles"]["us_per_launch"]["median"] / out["reduce"]["us_per_launch"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed windows per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("quantiles_ab.py needs a GPU")
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    q = (C.c_double * len(LEVELS))(*LEVELS)
    nq = len(LEVELS)
    rows = []
    same = True
    for K in (8, 32):
        # the plain launches: samples [B, K, 1, S, S]
        for B, S in ((1, 256), (8, 256)):
            chw = S * S
            samples = torch.rand((B, K, 1, S, S), device="cuda")
            mean, std = (torch.empty((B, 1, S, S), device="cuda") for _ in range(2))
            maps = torch.empty((B, nq, 1, S, S), device="cuda")

            def reduce(samples=samples, mean=mean, std=std, B=B, chw=chw):
                native.check(lib.mi_ensemble_reduce(samples.data_ptr(), B, K, chw, mean.data_ptr(), std.data_ptr(), stream))

            def quantiles(samples=samples, maps=maps, B=B, chw=chw):
                native.check(lib.mi_ensemble_quantiles(samples.data_ptr(), B, K, chw, q, nq, maps.data_ptr(), stream))

            plane = B * chw * 4
            rows.append(row("mi_ensemble_quantiles beside mi_ensemble_reduce (mean and std)", [B, 1, S, S], K,
                            {"reduce": reduce, "quantiles": quantiles},
                            {"reduce": (K + 2) * plane, "quantiles": (K + nq) * plane}, a.reps, a.warmup))
            same = same and bool(torch.equal(maps, midd_amd.ensemble_quantiles(samples, LEVELS)))
        # the tiled launches: one 1024 x 1024 image as 25 tiles
        S = 1024
        plan = midd_amd.tile_plan(S, S, T, O)
        tiles_per_image = len(plan.origins_y) * len(plan.origins_x)
        tiles = torch.rand((K, 1, tiles_per_image, 1, T, T), device="cuda")
        mean, std = (torch.empty((1, 1, S, S), device="cuda") for _ in range(2))
        maps = torch.empty((1, nq, 1, S, S), device="cuda")

        def blend_reduce():
            native.check(lib.mi_tile_blend_reduce(tiles.data_ptr(), 1, K, 1, S, S, T, T, O, O, mean.data_ptr(), std.data_ptr(), None, stream))

        def blend_quantiles():
            native.check(lib.mi_tile_blend_quantiles(tiles.data_ptr(), 1, K, 1, S, S, T, T, O, O, q, nq, maps.data_ptr(), stream))

        tile_bytes, plane = tiles.numel() * 4, S * S * 4
        rows.append(row("mi_tile_blend_quantiles beside mi_tile_blend_reduce (mean and std)", [1, 1, S, S, f"{tiles_per_image} tiles of {T}"], K,
                        {"reduce": blend_reduce, "quantiles": blend_quantiles},
                        {"reduce": tile_bytes + 2 * plane, "quantiles": tile_bytes + nq * plane}, a.reps, a.warmup))
        stacked = torch.stack([midd_amd.tile_blend(tiles[m], S, S, O) for m in range(K)], dim=1)
        same = same and bool(torch.equal(maps, midd_amd.ensemble_quantiles(stacked, LEVELS)))
        del tiles, stacked
    print(json.dumps({
        "tool": "tools/quantiles_ab.py",
        "metric": "time per launch of the quantile kernels (three levels) beside the mean / std reduce launch of the parent commit on "
                  "the same tensors, interleaved in one process; compulsory bytes: every member or tile once, every output once",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "data": "uniform random members", "rows": rows,
        "blend_quantiles_equal_blend_then_quantiles_bit_for_bit": same}))


if __name__ == "__main__":
    main()
