"""Same-process, same-box A/B of an ensemble of cddpm samples run as a loop of calls (A) and as one mi_denoise_ensemble call (B):

    (a) one 256x256 image, 50 iterations, 8 members
        A  eight denoise(seed=s, member=m) calls at batch 1: the loop over draws a user writes without the ensemble call
        B  one denoise_ensemble(members=8): the 8 (image, member) pairs as one batch of 8, two programs of 4 on two streams
    (b) 8 images x 8 members = 64 virtual samples
        A  four plain seeded denoise calls of batch 16 (64 samples, no ensemble bookkeeping): the executor's price for the samples
        B  denoise_ensemble(members=8, max_batch=16): four passes of 16, the condition broadcast per pass, one reduce launch

The shapes are warmed first, the arms are INTERLEAVED (A B A B ...) so that clock and thermal drift hits both alike, every timed
region is synchronised on both sides, and median [min - max] of at least 5 timed calls is reported, never a single run.  The
reduce kernel is then timed on its own: 200 launches of the C call with preallocated outputs between two events, its
(K + 2) * 4 bytes per pixel against the time per launch, at a cache-resident and at a 512 MiB shape.

    python tools/ensemble_ab.py [--reps 5] [--warmup 2] > profiles/ensemble_ab.json

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
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

SEED = 0x1234567890ABCDEF
S, STEPS, K = 256, 50, 8


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
    row["A_over_B_speedup"] = sa["median_ms"] / sb["median_ms"]
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
        raise SystemExit("ensemble_ab.py needs a GPU")
    cfg = UNetConfig(variant="cddpm")
    m = UNetDiffusion(variant="cddpm")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state_dict(cfg, seed=42).items()})
    m.check_status = False                        # no host synchronisation inside the timed calls (as a serving loop would run)
    den = DiffusionDenoiser(m.cuda().eval(), noise_steps=50)
    rows = []

    # (a) one image, eight draws
    one = torch.from_numpy(synthetic_xray(1, S, S, seed=1234)).cuda()

    def loop_of_members():
        return [den.denoise(one, inference_steps=STEPS, seed=SEED, member=k) for k in range(K)]

    def one_ensemble():
        return den.denoise_ensemble(one, inference_steps=STEPS, members=K, seed=SEED)

    row = {"workload": "(a) 1 image 256x256 x50, 8 members", "images": 1, "members": K, "image": [S, S], "iterations": STEPS,
           "A_is": "8 x denoise(seed, member=m) at batch 1", "B_is": "denoise_ensemble(members=8): one pass of 8"}
    row.update(ab({"A": loop_of_members, "B": one_ensemble}, a.reps, a.warmup))
    rows.append(row)

    # (b) eight images, eight draws each
    eight = torch.from_numpy(synthetic_xray(8, S, S, seed=1234)).cuda()
    sixteen = torch.cat([eight, eight])

    def four_batches_of_16():
        return [den.denoise(sixteen, inference_steps=STEPS, seed=SEED, sample_offset=16 * i) for i in range(4)]

    def ensemble_of_64():
        return den.denoise_ensemble(eight, inference_steps=STEPS, members=K, seed=SEED, max_batch=16)

    row = {"workload": "(b) 8 images 256x256 x50, 8 members", "images": 8, "members": K, "image": [S, S], "iterations": STEPS,
           "A_is": "4 x denoise(seed) at batch 16 (64 samples, no ensemble)", "B_is": "denoise_ensemble(members=8, max_batch=16): 4 passes of 16 + reduce"}
    row.update(ab({"A": four_batches_of_16, "B": ensemble_of_64}, a.reps, a.warmup))
    rows.append(row)

    # The reduce kernel alone, through the C call with preallocated outputs (no allocation, one ctypes call per launch), `n`
    # launches back to back between two events so that the queue stays full: workload (b)'s shape (16.8 MB of samples, which
    # the 256 MB last-level cache holds -- and which the sampler has just written when the ensemble call reduces them) and a
    # shape of 512 MiB that it cannot hold.
    import ctypes as C
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    reduce_rows = []
    for shape in [(8, K, 1, S, S), (64, K, 1, 512, 512)]:
        samples = torch.rand(shape, device="cuda")
        mean = torch.empty((shape[0],) + shape[2:], device="cuda")
        std = torch.empty_like(mean)
        chw = shape[2] * shape[3] * shape[4]
        n = 200
        per_launch = []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for rep in range(a.warmup + a.reps):
            ev[0].record()
            for _ in range(n):
                native.check(lib.mi_ensemble_reduce(samples.data_ptr(), shape[0], K, C.c_int64(chw), mean.data_ptr(), std.data_ptr(), stream))
            ev[1].record()
            ev[1].synchronize()
            if rep >= a.warmup:
                per_launch.append(1e3 * ev[0].elapsed_time(ev[1]) / n)
        bytes_per_launch = shape[0] * chw * (K + 2) * 4
        med = statistics.median(per_launch)
        reduce_rows.append({"shape": list(shape), "samples_bytes": samples.numel() * 4, "bytes_per_launch": bytes_per_launch,
                            "bytes_per_pixel": (K + 2) * 4, "launches_per_timed_window": n,
                            "us_per_launch": {"median": med, "min": min(per_launch), "max": max(per_launch)},
                            "GB_per_s_at_median": bytes_per_launch / (med * 1e-6) / 1e9})
        del samples, mean, std

    print(json.dumps({
        "tool": "tools/ensemble_ab.py",
        "metric": "wall time per ensemble on the cddpm model, a loop of calls (A) and one mi_denoise_ensemble call (B) interleaved in one process",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "compute": m.compute, "reps": a.reps, "warmup": a.warmup, "data": "synthetic", "rows": rows, "ensemble_reduce_kernel": reduce_rows}))


if __name__ == "__main__":
    main()
