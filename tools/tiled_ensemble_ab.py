"""Same-process, same-box A/B of an ensemble of tiled runs against the plain seeded batches its tiles amount to:

    A (the base)  the same 8 x 25 = 200 tiles of 256x256 as plain seeded denoise() batches of 16 (12 batches of 16, one of 8)
    B             one 1024x1024 image, 50 iterations, 8 members, tile 256, overlap 32, max_batch 16, through
                  denoise_tiled_ensemble(): members outer, 5 x 5 tiles per member in passes of 16 and 9 (a pass never spans two
                  members), an extract launch per pass, ONE blend-and-reduce launch

for the seeded cddpm model.  The shapes are warmed first, the arms are INTERLEAVED (A B A B ...) so that clock and thermal drift
hits both alike, every timed region is synchronised on both sides, and median [min - max] of at least 5 timed calls is reported,
never a single run.  B packs 16 + 9 tiles per member where A packs 16: B / A is recorded beside A's own spread.

The reduce kernel is then timed on its own -- 200 launches of the C call with preallocated buffers between two events -- beside
what it replaces on the same buffers: 8 blend launches (one per member, each into its slot of the blended members) + one ensemble
reduce launch.

    python tools/tiled_ensemble_ab.py [--reps 5] [--warmup 2] > profiles/tiled_ensemble_ab.json

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
S, T, O, STEPS, MAX_BATCH, MEMBERS = 1024, 256, 32, 50, 16, 8


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
    row["A_spread_over_A_median"] = sa["spread_ms"] / sa["median_ms"]
    row["B_slower_than_A_beyond_spread_of_A"] = bool(sb["median_ms"] - sa["median_ms"] > sa["spread_ms"])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed calls per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("tiled_ensemble_ab.py needs a GPU")
    image = torch.from_numpy(synthetic_xray(1, S, S, seed=1234)).cuda()
    plan = midd_amd.tile_plan(S, S, T, O)
    K = len(plan.origins_y) * len(plan.origins_x)
    crops = midd_amd.tile_extract(image, T, O).reshape(K, 1, T, T)
    every = crops.repeat(MEMBERS, 1, 1, 1)                                     # the 200 tiles of the 8 members, packed
    batches = [every[i:i + MAX_BATCH].contiguous() for i in range(0, MEMBERS * K, MAX_BATCH)]

    m = UNetDiffusion(variant="cddpm")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state_dict(UNetConfig(variant="cddpm"), seed=42).items()})
    m.check_status = False                        # no host synchronisation inside the timed calls (as a serving loop would run)
    den = DiffusionDenoiser(m.cuda().eval(), noise_steps=50)

    def plain_batches():
        return [den.denoise(b, inference_steps=STEPS, seed=SEED) for b in batches]

    def tiled_ensemble():
        return den.denoise_tiled_ensemble(image, inference_steps=STEPS, members=MEMBERS, tile=T, overlap=O, max_batch=MAX_BATCH, seed=SEED)

    passes = [min(MAX_BATCH, K - v) for v in range(0, K, MAX_BATCH)]
    row = {"variant": "cddpm", "image": [S, S], "tile": T, "overlap": O, "tiles_per_member": K, "members": MEMBERS, "iterations": STEPS,
           "max_batch": MAX_BATCH,
           "A_is": f"{MEMBERS * K} tiles of {T}x{T} as plain seeded denoise() batches of {[b.shape[0] for b in batches]} (the base)",
           "B_is": f"denoise_tiled_ensemble(one {S}x{S} image, {MEMBERS} members): per member passes of {passes} + extract per pass; one "
                   "blend-and-reduce launch",
           "tiled_ensemble_workspace_bytes": den.model.tiled_ensemble_workspace_bytes(1, MEMBERS, S, S, T, O, MAX_BATCH),
           "tiled_workspace_bytes": den.model.tiled_workspace_bytes(1, S, S, T, O, MAX_BATCH),
           "tile_storage_bytes": MEMBERS * K * T * T * 4}
    row.update(ab({"A": plain_batches, "B": tiled_ensemble}, a.reps, a.warmup))
    compute = m.compute
    del den, m

    # the reduce kernel alone beside the two kernels it composes, on the same buffers: `n` launches between two events
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    tiles = torch.rand((MEMBERS, 1, K, 1, T, T), device="cuda")
    mean, std = torch.empty_like(image), torch.empty_like(image)
    samples = torch.empty((1, MEMBERS, 1, S, S), device="cuda")
    n = 200
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    member_tiles, plane = K * T * T * 4, S * S * 4

    def fused(with_samples):
        def launch():
            native.check(lib.mi_tile_blend_reduce(tiles.data_ptr(), 1, MEMBERS, 1, S, S, T, T, O, O, mean.data_ptr(), std.data_ptr(),
                                                  samples.data_ptr() if with_samples else None, stream))
        return launch

    def two_kernels():
        for mm in range(MEMBERS):
            native.check(lib.mi_tile_blend(tiles.data_ptr() + mm * member_tiles, 1, 1, S, S, T, T, O, O, samples.data_ptr() + mm * plane, stream))
        native.check(lib.mi_ensemble_reduce(samples.data_ptr(), 1, MEMBERS, S * S, mean.data_ptr(), std.data_ptr(), stream))

    tile_bytes = MEMBERS * member_tiles
    kernels = []
    for name, fn, nbytes in [
            ("tile_blend_reduce_kernel: mean and std, the blended members never stored", fused(False), tile_bytes + 2 * plane),
            ("tile_blend_reduce_kernel: mean, std and samples_out", fused(True), tile_bytes + (2 + MEMBERS) * plane),
            (f"{MEMBERS} x tile_blend_kernel + ensemble_reduce_kernel<4> (what it composes)", two_kernels,
             tile_bytes + MEMBERS * plane + MEMBERS * plane + 2 * plane)]:
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
        kernels.append({"kernel": name, "algorithmic_bytes_per_call": nbytes, "calls_per_timed_window": n,
                        "us_per_call": {"median": med, "min": min(per_launch), "max": max(per_launch)},
                        "GB_per_s_at_median": nbytes / (med * 1e-6) / 1e9,
                        "note": "compulsory bytes: every tile once, every output once (the two-kernel arm also writes and reads the "
                                "blended members); cache-resident shapes (52 MB of tiles against a 256 MB last-level cache), as in the call itself"})
    two_kernels()
    want = (mean.clone(), std.clone())
    fused(False)()
    same = bool(torch.equal(mean, want[0]) and torch.equal(std, want[1]))

    print(json.dumps({
        "tool": "tools/tiled_ensemble_ab.py",
        "metric": f"wall time of {MEMBERS * K} tiles x {STEPS} iterations: plain seeded denoise() batches (A, the base) and one "
                  "denoise_tiled_ensemble() call (B), interleaved in one process",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "compute": compute, "reps": a.reps, "warmup": a.warmup, "data": "synthetic", "rows": [row], "kernels": kernels,
        "fused_equals_two_kernels_bit_for_bit": same}))


if __name__ == "__main__":
    main()
