"""Time of the windowed 16-bit pre/post-processing next to the unwindowed one, in one process:

    A  u16 image -> resize_bicubic_f32(512 x 512, clamp) -> resize_bicubic_f32(back, clamp, uint16)             (the calls as they were)
    B  u16 image -> histogram_u16 -> window_levels -> resize_bicubic_f32(512 x 512, clamp, levels)
                 -> resize_bicubic_f32(back, clamp, uint16, levels)                                            (the window)

on a 2500 x 2048 image and a 512 x 512 one (at 512 x 512 both arms are the pure conversions), 12-bit data in 16-bit elements.  The arms
are alternated (A, B, A, ...) so that clock drift hits both alike; median [min - max] of 20 timed calls per arm after 3 warm-up calls,
events around the Python calls (allocation and launch overhead included: what a request pays).  The histogram's own time (with its
zeroing memset) is taken on three 2500 x 2048 images -- seeded 12-bit noise, all zero, half zero half noise -- alternated the same
way: a flat image is the worst case for the on-chip counters (every lane of a wave adds to one word), and the flat / noise ratio says
whether the privatisation does its job.  The served sampler call (batch 1, 512 x 512, 9 iterations, full-width DDIM network,
random-init weights) is timed in the same process, so that the share of a request the window takes stands next to it.

    python tools/window16_ab.py [--reps 20] [--warmup 3] [--out profiles/window16_ab.json]

Writes ONE JSON object; `mi_source_hash` names the library build the numbers belong to."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import midd_loader  # noqa: E402

midd_loader.load()
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, prepost  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

SERVE = (512, 512)
SERVE_STEPS = 8            # -> 9 iterations with noise_steps = 50 (server.py)
README_SERVED_MS = 23.1    # README: the served call, batch 1, 512 x 512, 9 iterations
PERCENTILES = (0.5, 99.5)


def arm_a(raw16, hw):
    x = prepost.resize_bicubic_f32(raw16, SERVE, clamp=True)
    return prepost.resize_bicubic_f32(x, hw, clamp=True, out_dtype=torch.uint16)


def arm_b(raw16, hw):
    levels = prepost.window_levels(prepost.histogram_u16(raw16), PERCENTILES)
    x = prepost.resize_bicubic_f32(raw16, SERVE, clamp=True, levels=levels)
    return prepost.resize_bicubic_f32(x, hw, clamp=True, out_dtype=torch.uint16, levels=levels)


def stats(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def timed(calls, reps, warmup):
    """calls: name -> thunk; -> name -> ms of every timed call, the arms alternated."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = {name: [] for name in calls}
    for rep in range(warmup + reps):
        for name, fn in calls.items():
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            if rep >= warmup:
                per[name].append(ev[0].elapsed_time(ev[1]))
    return per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="timed calls per arm")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sampler-reps", type=int, default=5, help="timed served sampler calls")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window16_ab.json"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("window16_ab.py needs a GPU")
    rows = []
    for h, w in ((2500, 2048), (512, 512)):
        arr = np.round(synthetic_xray(1, h, w, seed=h + w)[0, 0].clip(0, 1) * 4095).astype(np.uint16)
        raw16 = torch.from_numpy(arr).cuda()
        per = timed({"A_unwindowed": lambda: arm_a(raw16, (h, w)), "B_windowed": lambda: arm_b(raw16, (h, w))}, a.reps, a.warmup)
        row = {"image": [h, w], "served_size": list(SERVE), "levels": prepost.window_levels(raw16, PERCENTILES).cpu().tolist()[0]}
        for name, t in per.items():
            row[name] = {"ms_per_call": stats(t)}
        row["B_over_A_time"] = row["B_windowed"]["ms_per_call"]["median"] / row["A_unwindowed"]["ms_per_call"]["median"]
        row["B_minus_A_ms"] = row["B_windowed"]["ms_per_call"]["median"] - row["A_unwindowed"]["ms_per_call"]["median"]
        rows.append(row)
    h, w = 2500, 2048
    rng = np.random.default_rng(16)
    noise = rng.integers(0, 4096, (h, w)).astype(np.uint16)
    half = noise.copy()
    half[: h // 2] = 0
    images = {"noise12": torch.from_numpy(noise).cuda(), "zeros": torch.zeros((h, w), dtype=torch.int16, device="cuda").view(torch.uint16),
              "half_zero_half_noise": torch.from_numpy(half).cuda()}
    per = timed({name: (lambda t=t: prepost.histogram_u16(t)) for name, t in images.items()}, a.reps, a.warmup)
    hist = {"image": [h, w], "what": "histogram_u16 alone: the memset of [1][65536] counts, the kernel, the allocation of the result"}
    for name, t in per.items():
        hist[name] = {"ms_per_call": stats(t)}
    hist["zeros_over_noise12_time"] = hist["zeros"]["ms_per_call"]["median"] / hist["noise12"]["ms_per_call"]["median"]
    hist["half_over_noise12_time"] = hist["half_zero_half_noise"]["ms_per_call"]["median"] / hist["noise12"]["ms_per_call"]["median"]
    lev = timed({"levels": lambda: prepost.window_levels(prepost.histogram_u16(images["noise12"]), PERCENTILES)}, a.reps, a.warmup)
    hist["histogram_plus_levels_noise12"] = {"ms_per_call": stats(lev["levels"])}
    model = UNetDiffusion()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(UNetConfig(), seed=42).items()})
    den = DiffusionDenoiser(model.to("cuda").eval(), noise_steps=50)
    x = torch.from_numpy(synthetic_xray(1, SERVE[0], SERVE[1], seed=77)).cuda()
    served = stats(timed({"served": lambda: den.denoise(x, SERVE_STEPS)}, a.sampler_reps, 2)["served"])
    for row in rows:
        for name in ("A_unwindowed", "B_windowed"):
            row[name]["share_of_served_sampler_call"] = row[name]["ms_per_call"]["median"] / served["median"]
            row[name]["share_of_readme_served_call"] = row[name]["ms_per_call"]["median"] / README_SERVED_MS
        row["window_cost_share_of_served_sampler_call"] = row["B_minus_A_ms"] / served["median"]
    result = {
        "tool": "tools/window16_ab.py",
        "metric": "wall time (events around the Python calls) of the pre- plus post-processing of one request at bit depth 16: arm A the "
                  "unwindowed calls, arm B histogram + levels + the windowed calls, alternated in one process; the histogram alone on "
                  "three images; and the served sampler call (batch 1, 512 x 512, 9 iterations) of the same build, whose kernels this "
                  "comparison does not touch",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "percentiles": list(PERCENTILES), "rows": rows, "histogram": hist,
        "served_sampler_call": {"shape": [1, 1, SERVE[0], SERVE[1]], "iterations": SERVE_STEPS + 1, "reps": a.sampler_reps,
                                "weights": "random-init (make_state_dict seed 42)", "ms_per_call": served,
                                "readme_ms": README_SERVED_MS}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(result) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
