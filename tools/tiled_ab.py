"""Same-process, same-box A/B of tiled denoising against the plain batches its tiles amount to:

    A (the base)  the same number of 256x256 tiles as plain denoise() batches of 16 (25 tiles: one batch of 16, one of 9)
    B             one 1024x1024 image, 50 iterations, tile 256, overlap 32, max_batch 16, through denoise_tiled():
                  5 x 5 tiles, passes of 16 and 9, an extract launch per pass, one blend launch

for the DDIM model and for the seeded cddpm model.  The shapes are warmed first, the arms are INTERLEAVED (A B A B ...) so that
clock and thermal drift hits both alike, every timed region is synchronised on both sides, and median [min - max] of at least 5
timed calls is reported, never a single run.  The two kernels are then timed on their own: 200 launches of the C call with
preallocated buffers between two events -- the extract of a pass of 16 tiles (8 bytes per tile pixel) and the blend of the 25
tiles (4 bytes per tile pixel read + 4 per image pixel written).

    python tools/tiled_ab.py [--reps 5] [--warmup 2] > profiles/tiled_ab.json

Prints ONE JSON object; `mi_source_hash` names the library build the numbers belong to."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import midd_loader  # noqa: E402

midd_loader.load()
import midd_amd  # noqa: E402
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

SEED = 0x1234567890ABCDEF
S, T, O, STEPS, MAX_BATCH = 1024, 256, 32, 50, 16


def summary(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "spread_ms": max(t) - min(t), "calls": len(t)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


def ab(arms, reps, warmup):
    times = {name: [] for name in arms}
    for rep in range(warmup + reps):
        for name, fn in arms.items():             # interleaved: A B A B
            ms, out = timed(fn)
            if rep >= warmup:
                times[name].append(ms)
            del out
    row = {name: summary(t) for name, t in times.items()}
    sa, sb = row["A"], row["B"]
    row["B_over_A_time"] = sb["median_ms"] / sa["median_ms"]
    row["B_slower_than_A_beyond_spread_of_A"] = bool(sb["median_ms"] - sa["median_ms"] > sa["spread_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed calls per arm and workload (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("tiled_ab.py needs a GPU")
    image = torch.from_numpy(synthetic_xray(1, S, S, seed=1234)).cuda()
    plan = midd_amd.tile_plan(S, S, T, O)
    K = len(plan.origins_y) * len(plan.origins_x)
    crops = midd_amd.tile_extract(image, T, O).reshape(K, 1, T, T)
    batches = [crops[i:i + MAX_BATCH].contiguous() for i in range(0, K, MAX_BATCH)]
    rows = []
    compute = None
    for variant in ("ddim", "cddpm"):
        m = UNetDiffusion(variant=variant)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state_dict(UNetConfig(variant=variant), seed=42).items()})
        m.check_status = False                    # no host synchronisation inside the timed calls (as a serving loop would run)
        den = DiffusionDenoiser(m.cuda().eval(), noise_steps=50)
        compute = m.compute
        kw = {"seed": SEED} if variant == "cddpm" else {}

        def plain_batches():
            return [den.denoise(b, inference_steps=STEPS, **kw) for b in batches]

        def tiled():
            return den.denoise_tiled(image, inference_steps=STEPS, tile=T, overlap=O, max_batch=MAX_BATCH, **kw)

        row = {"variant": variant, "image": [S, S], "tile": T, "overlap": O, "tiles": K, "iterations": STEPS, "max_batch": MAX_BATCH,
               "A_is": f"{K} tiles of {T}x{T} as plain denoise() batches of {[b.shape[0] for b in batches]} (the base)",
               "B_is": f"denoise_tiled(one {S}x{S} image): {len(batches)} passes + extract per pass + one blend",
               "tiled_workspace_bytes": den.model.tiled_workspace_bytes(1, S, S, T, O, MAX_BATCH)}
        row.update(ab({"A": plain_batches, "B": tiled}, a.reps, a.warmup))
        rows.append(row)
        del den, m

    # the two kernels alone, through the C calls with preallocated buffers, `n` launches back to back between two events
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    tiles = torch.rand((1, K, 1, T, T), device="cuda")
    out = torch.empty_like(image)
    dst = torch.empty((MAX_BATCH, 1, T, T), device="cuda")
    n = 200
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def launch_extract():
        native.check(lib.mi_tile_extract(image.data_ptr(), 1, 1, S, S, T, T, O, O, 0, MAX_BATCH, dst.data_ptr(), stream))

    def launch_blend():
        native.check(lib.mi_tile_blend(tiles.data_ptr(), 1, 1, S, S, T, T, O, O, out.data_ptr(), stream))

    kernels = []
    for name, fn, nbytes in [("tile_extract_kernel<4>: a pass of 16 tiles", launch_extract, MAX_BATCH * T * T * 8),
                             ("tile_blend_kernel: 25 tiles -> 1024x1024", launch_blend, K * T * T * 4 + S * S * 4)]:
        per_launch = []
        for rep in range(a.warmup + a.reps):
            ev[0].record()
            for _ in range(n):
                fn()
            ev[1].record()
            ev[1].synchronize()
            if rep >= a.warmup:
                per_launch.append(1e3 * ev[0].elapsed_time(ev[1]) / n)
        med = statistics.median(per_launch)
        kernels.append({"kernel": name, "bytes_per_launch": nbytes, "launches_per_timed_window": n,
                        "us_per_launch": {"median": med, "min": min(per_launch), "max": max(per_launch)},
                        "GB_per_s_at_median": nbytes / (med * 1e-6) / 1e9,
                        "note": "cache-resident shapes (4-7 MB against a 256 MB last-level cache), as in the tiled call itself"})

    print(json.dumps({
        "tool": "tools/tiled_ab.py",
        "metric": "wall time of 25 tiles x 50 iterations: plain denoise() batches (A, the base) and one denoise_tiled() call (B), interleaved in one process",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "compute": compute, "reps": a.reps, "warmup": a.warmup, "data": "synthetic", "rows": rows, "kernels": kernels}))


if __name__ == "__main__":
    main()
