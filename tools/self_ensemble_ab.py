"""Same-process, same-box A/B of the geometric self-ensemble of the DDIM sampler run as the loop a user writes today (A) and as
one mi_denoise_self_ensemble call (B):

    (a) one 256x256 image, 50 iterations, 8 views
        A  eight denoise calls at batch 1 on torch.flip / transpose copies, the outputs turned back, stacked, ensemble_reduce
        B  one denoise_self_ensemble(views="d4"): the 8 (image, view) pairs as one batch of 8, two programs of 4 on two streams
    (b) 8 images x 8 views = 64 virtual samples
        A  four plain denoise calls of batch 16 (64 samples, no views, no reduce): the executor's price for the samples
        B  denoise_self_ensemble(views="d4", max_batch=16): four passes of 16, the view fill per pass, one reduce launch
    (c) the kernels alone, on workload (b)'s tensors ([8, 8, 1, 256, 256]): microseconds per launch of dihedral_views (one pass of
        16), dihedral_reduce with the four flips and with all eight views beside ensemble_reduce over as many members, and
        dihedral_quantiles with three levels beside ensemble_quantiles; bytes per launch / time at the median

The shapes are warmed first, the arms are INTERLEAVED (A B A B ...) so that clock and thermal drift hits both alike, every timed
region is synchronised on both sides, and median [min - max] of at least 5 timed calls is reported, never a single run.  The
kernels of (c) run 200 launches of the C call with preallocated outputs between two events.

    python tools/self_ensemble_ab.py [--reps 5] [--warmup 2] > profiles/self_ensemble_ab.json

Prints ONE JSON object; `mi_source_hash` names the library build the numbers belong to."""
import argparse
import ctypes as C
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

S, STEPS = 256, 50
D4, FLIPS = (0, 1, 2, 3, 4, 5, 6, 7), (0, 1, 2, 3)


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
    row["A_spread_over_A_median"] = sa["spread_ms"] / sa["median_ms"]
    row["B_outside_spread_of_A"] = bool(abs(sb["median_ms"] - sa["median_ms"]) > sa["spread_ms"])
    return row


def view_t(x, g):
    u = x.transpose(-1, -2) if g & 4 else x
    if g & 2:
        u = u.flip(-2)
    if g & 1:
        u = u.flip(-1)
    return u.contiguous()


def unview_t(y, g):
    u = y
    if g & 1:
        u = u.flip(-1)
    if g & 2:
        u = u.flip(-2)
    if g & 4:
        u = u.transpose(-1, -2)
    return u.contiguous()


def per_launch(fn, reps, warmup, n=200):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    us = []
    for rep in range(warmup + reps):
        ev[0].record()
        for _ in range(n):
            native.check(fn())
        ev[1].record()
        ev[1].synchronize()
        if rep >= warmup:
            us.append(1e3 * ev[0].elapsed_time(ev[1]) / n)
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed calls per arm and workload (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("self_ensemble_ab.py needs a GPU")
    cfg = UNetConfig()
    m = UNetDiffusion()
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state_dict(cfg, seed=42).items()})
    m.check_status = False                        # no host synchronisation inside the timed calls (as a serving loop would run)
    den = DiffusionDenoiser(m.cuda().eval(), noise_steps=50)
    rows = []

    # (a) one image, eight views
    one = torch.from_numpy(synthetic_xray(1, S, S, seed=1234)).cuda()

    def loop_of_views():
        outs = [unview_t(den.denoise(view_t(one, g), inference_steps=STEPS), g) for g in D4]
        return midd_amd.ensemble_reduce(torch.stack(outs, dim=1))

    def one_call():
        return den.denoise_self_ensemble(one, inference_steps=STEPS, views="d4")

    row = {"workload": "(a) 1 image 256x256 x50, 8 views", "images": 1, "views": 8, "image": [S, S], "iterations": STEPS,
           "A_is": "8 x denoise at batch 1 on torch.flip / transpose copies, unview, stack, ensemble_reduce",
           "B_is": "denoise_self_ensemble(views='d4'): one pass of 8"}
    row.update(ab({"A": loop_of_views, "B": one_call}, a.reps, a.warmup))
    rows.append(row)

    # (b) eight images, eight views each
    eight = torch.from_numpy(synthetic_xray(8, S, S, seed=1234)).cuda()
    sixteen = torch.cat([eight, eight])

    def four_batches_of_16():
        return [den.denoise(sixteen, inference_steps=STEPS) for _ in range(4)]

    def self_ensemble_of_64():
        return den.denoise_self_ensemble(eight, inference_steps=STEPS, views="d4", max_batch=16)

    row = {"workload": "(b) 8 images 256x256 x50, 8 views", "images": 8, "views": 8, "image": [S, S], "iterations": STEPS,
           "A_is": "4 x denoise at batch 16 (64 samples, no views, no reduce)",
           "B_is": "denoise_self_ensemble(views='d4', max_batch=16): 4 passes of 16 (view fill each) + reduce"}
    row.update(ab({"A": four_batches_of_16, "B": self_ensemble_of_64}, a.reps, a.warmup))
    rows.append(row)

    # (c) the kernels alone on workload (b)'s tensors, through the C calls with preallocated outputs
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    B, chw = 8, S * S
    img_bytes = chw * 4
    kernels = []

    def entry(name, us, nbytes, note):
        kernels.append({"kernel": name, "note": note, "bytes_per_launch": nbytes, "us_per_launch": us,
                        "GB_per_s_at_median": nbytes / (us["median"] * 1e-6) / 1e9})

    d4 = (C.c_int32 * 8)(*D4)
    fl = (C.c_int32 * 4)(*FLIPS)
    cond = torch.empty((16, 1, S, S), device="cuda")
    entry("dihedral_views", per_launch(lambda: lib.mi_dihedral_views(eight.data_ptr(), B, 1, S, S, d4, 8, 16, 16, cond.data_ptr(), stream), a.reps, a.warmup),
          2 * 16 * img_bytes, "one pass of 16 virtual samples (2 images x 8 views): 16 planes read + written")
    mean = torch.empty((B, 1, S, S), device="cuda")
    std = torch.empty_like(mean)
    q3 = (C.c_double * 3)(0.05, 0.5, 0.95)
    qout = torch.empty((B, 3, 1, S, S), device="cuda")
    for G, arr, label in ((4, fl, "flips"), (8, d4, "d4")):
        vo = torch.rand((B, G, 1, S, S), device="cuda")
        red_bytes, q_bytes = B * (G + 2) * img_bytes, B * (G + 3) * img_bytes
        entry(f"dihedral_reduce[{label}]", per_launch(lambda: lib.mi_dihedral_reduce(vo.data_ptr(), B, 1, S, S, arr, G, mean.data_ptr(), std.data_ptr(), None, stream), a.reps, a.warmup),
              red_bytes, f"{G} views, mean + std" + (", no LDS" if G == 4 else ", 4 of them staged through LDS"))
        entry(f"ensemble_reduce[{G}]", per_launch(lambda: lib.mi_ensemble_reduce(vo.data_ptr(), B, G, C.c_int64(chw), mean.data_ptr(), std.data_ptr(), stream), a.reps, a.warmup),
              red_bytes, f"{G} members, mean + std (the existing kernel, same tensors)")
        entry(f"dihedral_quantiles[{label}]", per_launch(lambda: lib.mi_dihedral_quantiles(vo.data_ptr(), B, 1, S, S, arr, G, q3, 3, qout.data_ptr(), stream), a.reps, a.warmup),
              q_bytes, f"{G} views, three levels")
        entry(f"ensemble_quantiles[{G}]", per_launch(lambda: lib.mi_ensemble_quantiles(vo.data_ptr(), B, G, C.c_int64(chw), q3, 3, qout.data_ptr(), stream), a.reps, a.warmup),
              q_bytes, f"{G} members, three levels (the existing kernel, same tensors)")
        del vo

    print(json.dumps({
        "tool": "tools/self_ensemble_ab.py",
        "metric": "wall time per self-ensemble on the DDIM model, the loop a user writes (A) and one mi_denoise_self_ensemble call (B) interleaved "
                  "in one process; microseconds per launch of the new kernels beside the existing ones on the same tensors",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "compute": m.compute, "reps": a.reps, "warmup": a.warmup, "data": "synthetic", "rows": rows, "kernels": kernels}))


if __name__ == "__main__":
    main()
