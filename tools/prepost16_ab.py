"""Time of the 16-bit pre/post-processing next to the 8-bit one, in one process:

    float  u16 image -> resize_bicubic_f32(512 x 512, clamp) -> resize_bicubic_f32(back, clamp, uint16)        (the new calls)
    u8     the same image's high byte -> to_unit_float(resize_bicubic_u8(512 x 512)) -> resize_bicubic_u8(to_u8(.), back)

on a 2500 x 2048 image and a 512 x 512 one (at 512 x 512 both arms are the pure conversions).  The arms are alternated (float, u8,
float, ...) so that clock drift hits both alike; median [min - max] of 20 timed calls per arm after 3 warm-up calls, events around
the Python calls (workspace allocation and launch overhead included: what a request pays).  The sampler call of a served request
(batch 1, 512 x 512, 9 iterations, full-width DDIM network, random-init weights) is timed in the same process, so that the share of
a request the pre/post-processing takes stands next to it.

    python tools/prepost16_ab.py [--reps 20] [--warmup 3] > profiles/prepost16_ab.json

Prints ONE JSON object; `mi_source_hash` names the library build the numbers belong to."""
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


def arm_float(raw16, hw):
    x = prepost.resize_bicubic_f32(raw16, SERVE, clamp=True)
    return prepost.resize_bicubic_f32(x, hw, clamp=True, out_dtype=torch.uint16)


def arm_u8(raw8, hw):
    x = prepost.to_unit_float(prepost.resize_bicubic_u8(raw8, SERVE))
    return prepost.resize_bicubic_u8(prepost.to_u8(x), hw)


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
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("prepost16_ab.py needs a GPU")
    rows = []
    for h, w in ((2500, 2048), (512, 512)):
        arr = np.round(synthetic_xray(1, h, w, seed=h + w)[0, 0].clip(0, 1) * 65535).astype(np.uint16)
        raw16 = torch.from_numpy(arr).cuda()
        raw8 = torch.from_numpy((arr >> 8).astype(np.uint8)).cuda()
        per = timed({"float": lambda: arm_float(raw16, (h, w)), "u8": lambda: arm_u8(raw8, (h, w))}, a.reps, a.warmup)
        row = {"image": [h, w], "served_size": list(SERVE)}
        for name, t in per.items():
            row[name] = {"ms_per_call": stats(t)}
        row["float_over_u8_time"] = row["float"]["ms_per_call"]["median"] / row["u8"]["ms_per_call"]["median"]
        rows.append(row)
    model = UNetDiffusion()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(UNetConfig(), seed=42).items()})
    den = DiffusionDenoiser(model.to("cuda").eval(), noise_steps=50)
    x = torch.from_numpy(synthetic_xray(1, SERVE[0], SERVE[1], seed=77)).cuda()
    served = stats(timed({"served": lambda: den.denoise(x, SERVE_STEPS)}, a.sampler_reps, 2)["served"])
    for row in rows:
        for name in ("float", "u8"):
            row[name]["share_of_served_sampler_call"] = row[name]["ms_per_call"]["median"] / served["median"]
    print(json.dumps({
        "tool": "tools/prepost16_ab.py",
        "metric": "wall time (events around the Python calls) of the pre- plus post-processing of one request: u16 -> 512 x 512 -> back "
                  "through the float calls beside the same image's high byte through the u8 calls, alternated in one process; and "
                  "the served sampler call (batch 1, 512 x 512, 9 iterations) of the same build, whose kernels this comparison does "
                  "not touch",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "rows": rows,
        "served_sampler_call": {"shape": [1, 1, SERVE[0], SERVE[1]], "iterations": SERVE_STEPS + 1, "reps": a.sampler_reps,
                                "weights": "random-init (make_state_dict seed 42)", "ms_per_call": served}}))


if __name__ == "__main__":
    main()
