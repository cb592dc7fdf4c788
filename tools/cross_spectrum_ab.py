"""Time of the cross-spectrum call next to the existing code that does the nearest equivalent work, in one process:

    mi_cross_spectrum            (x, y: K members each, R = 64, S = 32, plane detrend, Hann window; six launches)
    2 x mi_noise_power_spectrum  (the same two tensors, one call each, b = NULL: two half-plane transforms per ROI pair instead of
                                  one full one, one accumulator per entry instead of four, and no cross term)
    a device copy of both stacks (read once, written once): what moving them costs on the device -- the host path this call
                                  replaces copies both over the bus instead

for one 256x256 image with K = 8 members, a batch of 8 at 256x256 with K = 8, and one 2500x2048 image with K = 8.  No network runs:
x is clip(0.5 + 0.35 n, 0, 1) and y = 0.6 x + 0.4 n'.  Every launch is the C call with preallocated outputs; `n` launches sit between
two events, the arms alternate so that clock drift hits all alike, and median [min - max] of at least 5 timed windows is reported,
never a single run.  The ratio cross / (2 x NPS) stands beside the NPS arm's own spread (max / min of its windows).

    python tools/cross_spectrum_ab.py [--reps 5] [--warmup 2] [--out profiles/cross_spectrum_ab.json]

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_spectrum_ab.json"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("cross_spectrum_ab.py needs a GPU")
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    window = midd_amd.nps_window("hann", ROI)
    warg = (C.c_float * ROI)(*window.tolist())
    bins = ROI // 2 + 1
    rows = []
    for B, H, W, K in SHAPES:
        n = 50 if H * W * B * K <= (1 << 24) else 10
        x = (0.5 + 0.35 * torch.randn((B, K, 1, H, W), device="cuda", generator=gen)).clamp_(0, 1)
        y = 0.6 * x + 0.4 * (0.5 + 0.35 * torch.randn((B, K, 1, H, W), device="cuda", generator=gen)).clamp_(0, 1)
        copy_dst = torch.empty((2,) + tuple(x.shape), device="cuda")
        # the cross-spectrum's outputs [radial 4*B*bins | count | used | skipped | planes 4*B*R*R] and workspace
        o_cnt = 4 * B * bins
        o_used, o_skip, o_pl = o_cnt + bins, o_cnt + bins + B, o_cnt + bins + 2 * B
        raw = torch.zeros(o_pl + 4 * B * ROI * ROI, dtype=torch.int64, device="cuda")
        base = raw.data_ptr()
        xs_bytes = lib.mi_cross_spectrum_workspace_bytes(B, K, K, 1, H, W, ROI, STEP)
        xs_ws = torch.empty(xs_bytes // 8, dtype=torch.float64, device="cuda")
        # the NPS's outputs [nps B*R*R | radial | count | used | skipped], one set per call, and workspace
        nraw = torch.zeros(B * ROI * ROI + B * bins + bins + 2 * B, dtype=torch.int64, device="cuda")
        nbase = nraw.data_ptr()
        n_rad = nbase + 8 * B * ROI * ROI
        n_cnt, n_used, n_skip = n_rad + 8 * B * bins, n_rad + 8 * (B * bins + bins), n_rad + 8 * (B * bins + bins + B)
        nps_bytes = lib.mi_noise_power_spectrum_workspace_bytes(B, K, 1, H, W, ROI, STEP)
        nps_ws = torch.empty(nps_bytes // 8, dtype=torch.float64, device="cuda")

        def cross():
            native.check(lib.mi_cross_spectrum(x.data_ptr(), y.data_ptr(), B, K, K, 1, H, W, ROI, STEP, 2, warg, 0, base + 8 * o_pl, base,
                                               base + 8 * o_cnt, base + 8 * o_used, base + 8 * o_skip, xs_ws.data_ptr(), xs_bytes, stream))

        def nps_twice():
            for t in (x, y):
                native.check(lib.mi_noise_power_spectrum(t.data_ptr(), None, B, K, 1, H, W, ROI, STEP, 2, warg, 1.0, 0, nbase, n_rad, n_cnt,
                                                         n_used, n_skip, nps_ws.data_ptr(), nps_bytes, stream))

        def copy():
            copy_dst[0].copy_(x)
            copy_dst[1].copy_(y)

        plane = B * H * W * 4
        rois = B * K * ((H - ROI) // STEP + 1) * ((W - ROI) // STEP + 1)
        nbytes = {"cross": 2 * K * plane + 2 * xs_bytes + 4 * 8 * B * ROI * ROI, "nps_twice": 2 * (K * plane + 2 * nps_bytes + 8 * B * ROI * ROI),
                  "copy": 4 * K * plane}
        per = windows({"nps_twice": nps_twice, "cross": cross, "copy": copy}, n, a.reps, a.warmup)
        row = {"shape": [B, 1, H, W], "members": K, "roi": ROI, "step": STEP, "roi_pairs": rois, "workspace_bytes": xs_bytes,
               "nps_workspace_bytes": nps_bytes, "launches_per_timed_window": n}
        for name, t in per.items():
            med = statistics.median(t)
            row[name] = {"us_per_call": {"median": med, "min": min(t), "max": max(t)}, "algorithmic_bytes": nbytes[name],
                         "GB_per_s_at_median": nbytes[name] / (med * 1e-6) / 1e9}
        med = row["cross"]["us_per_call"]["median"]
        two = row["nps_twice"]["us_per_call"]
        row["cross"]["roi_pairs_per_us"] = rois / med
        row["cross_over_nps_twice_time"] = med / two["median"]
        row["cross_over_one_nps_time"] = 2.0 * med / two["median"]
        row["nps_twice_spread_max_over_min"] = two["max"] / two["min"]
        row["cross_over_copy_time"] = med / row["copy"]["us_per_call"]["median"]
        sp = midd_amd.cross_spectrum(x, y, ROI, STEP)
        row["result_group_0"] = {"transfer_1": float(sp.transfer()[0, 0, 1]), "frc_1": float(sp.frc()[0, 0, 1]),
                                 "frc_nyquist": float(sp.frc()[0, 0, -1]), "rois_used": int(sp.rois_used[0, 0])}
        rows.append(row)
        del x, y, copy_dst, xs_ws, nps_ws
    out = {
        "tool": "tools/cross_spectrum_ab.py",
        "metric": "time per call of mi_cross_spectrum (x, y with K members each, R = 64, S = 32, plane detrend, Hann window; six launches: "
                  "the ROIs, the chunk sums, the radial bins of four planes) beside two mi_noise_power_spectrum calls on the same two "
                  "tensors and a device copy of both stacks, alternating in one process; there is no pass / fail threshold",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "data": "x = clip(0.5 + 0.35 n, 0, 1), y = 0.6 x + 0.4 clip(0.5 + 0.35 n', 0, 1)", "rows": rows}
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
