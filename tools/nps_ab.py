"""Time of the noise-power-spectrum call next to the existing reduction over the same members, in one process:

    mi_noise_power_spectrum  (member - mean, R = 64, S = 32, plane detrend, Hann window; three launches)
    mi_ensemble_reduce       (mean and std of the same members)
    a device copy of the members (read once, written once): the rate the memory system gives a plain stream of that size

for one 256x256 image with K = 8 members, a batch of 8 at 256x256 with K = 8, and one 2500x2048 image with K = 8.  No network runs:
the members are clip(0.5 + 0.35 n, 0, 1).  Every launch is the C call with preallocated outputs; `n` launches sit between two
events, the arms alternate so that clock drift hits all alike, and median [min - max] of at least 5 timed windows is reported, never
a single run.  Beside every time stand the bytes the call must read and write (every member and the mean once -- overlapping ROIs
re-read each pixel up to (R/S)^2 = 4 times, which the caches may or may not absorb -- and the workspace once each way), the ROIs per
second, and the fp32 butterflies per second (R^2/2 log2 R for the rows plus (R/2+1) R/2 log2 R for the columns, 10 flops each).

    python tools/nps_ab.py [--reps 5] [--warmup 2] [--out profiles/nps_ab.json]

Writes ONE JSON object (and prints it); `mi_source_hash` names the library build the numbers belong to."""
import argparse
import ctypes as C
import json
import math
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

ROI, STEP = 64, 32
SHAPES = [(1, 256, 256, 8), (8, 256, 256, 8), (1, 2500, 2048, 8)]      # (B, H, W, K)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nps_ab.json"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("nps_ab.py needs a GPU")
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    window = midd_amd.nps_window("hann", ROI)
    warg = (C.c_float * ROI)(*window.tolist())
    bins = ROI // 2 + 1
    rows = []
    for B, H, W, K in SHAPES:
        chw = H * W
        n = 50 if chw * B * K <= (1 << 24) else 10
        samples = (0.5 + 0.35 * torch.randn((B, K, 1, H, W), device="cuda", generator=gen)).clamp_(0, 1)
        copy_dst = torch.empty_like(samples)
        mean, std = (torch.empty((B, 1, H, W), device="cuda") for _ in range(2))
        native.check(lib.mi_ensemble_reduce(samples.data_ptr(), B, K, chw, mean.data_ptr(), std.data_ptr(), stream))
        raw = torch.zeros(B * ROI * ROI + B * bins + bins + 2 * B, dtype=torch.int64, device="cuda")
        base = raw.data_ptr()
        o_rad = base + 8 * B * ROI * ROI
        o_cnt, o_used, o_skip = o_rad + 8 * B * bins, o_rad + 8 * (B * bins + bins), o_rad + 8 * (B * bins + bins + B)
        ws_bytes = lib.mi_noise_power_spectrum_workspace_bytes(B, K, 1, H, W, ROI, STEP)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")

        def reduce():
            native.check(lib.mi_ensemble_reduce(samples.data_ptr(), B, K, chw, mean.data_ptr(), std.data_ptr(), stream))

        def nps():
            native.check(lib.mi_noise_power_spectrum(samples.data_ptr(), mean.data_ptr(), B, K, 1, H, W, ROI, STEP, 2, warg, K / (K - 1), 0,
                                                     base, o_rad, o_cnt, o_used, o_skip, ws.data_ptr(), ws_bytes, stream))

        def copy():
            copy_dst.copy_(samples)

        plane = B * chw * 4
        rois = B * K * ((H - ROI) // STEP + 1) * ((W - ROI) // STEP + 1)
        flies = rois * (ROI * ROI // 2 + bins * ROI // 2) * int(math.log2(ROI))
        nbytes = {"reduce": (K + 2) * plane, "nps": (K + 1) * plane + 2 * ws_bytes + 8 * B * ROI * ROI, "copy": 2 * K * plane}
        per = windows({"reduce": reduce, "nps": nps, "copy": copy}, n, a.reps, a.warmup)
        row = {"shape": [B, 1, H, W], "members": K, "roi": ROI, "step": STEP, "rois": rois, "workspace_bytes": ws_bytes,
               "launches_per_timed_window": n}
        for name, t in per.items():
            med = statistics.median(t)
            row[name] = {"us_per_call": {"median": med, "min": min(t), "max": max(t)}, "algorithmic_bytes": nbytes[name],
                         "GB_per_s_at_median": nbytes[name] / (med * 1e-6) / 1e9}
        med = row["nps"]["us_per_call"]["median"]
        row["nps"]["rois_per_us"] = rois / med
        row["nps"]["butterfly_GFLOP_per_s"] = 10 * flies / (med * 1e-6) / 1e9
        row["nps_over_reduce_time"] = med / row["reduce"]["us_per_call"]["median"]
        row["nps_over_copy_time"] = med / row["copy"]["us_per_call"]["median"]
        sp = midd_amd.noise_power_spectrum(samples, mean, ROI, STEP, scale=K / (K - 1))
        row["result_group_0"] = {"variance": float(sp.variance()[0, 0]), "radial_1": float(sp.radial[0, 0, 1]),
                                 "radial_nyquist": float(sp.radial[0, 0, -1]), "rois_used": int(sp.rois_used[0, 0])}
        rows.append(row)
        del samples, copy_dst, ws
    out = {
        "tool": "tools/nps_ab.py",
        "metric": "time per call of mi_noise_power_spectrum (member - mean, R = 64, S = 32, plane detrend, Hann window; the call is three "
                  "launches: the ROIs, the chunk sums, the radial bins) beside mi_ensemble_reduce on the same members and a device copy of the "
                  "members, alternating in one process; compulsory bytes: every member and the mean once, the workspace written and read once, "
                  "the spectrum once",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "data": "clip(0.5 + 0.35 n, 0, 1)", "rows": rows}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
