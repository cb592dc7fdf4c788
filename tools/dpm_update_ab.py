"""Time of one sampler call under update="dpmpp2m" next to the same call under update="ddim", in one process:

    denoise(x, 50, update="ddim")                      (the base: out_conv_ddim_kernel, eta = 0)
    denoise(x, 50, update="dpmpp2m")                   (out_conv_dpm_kernel: one history slot, read and written in place)
    denoise(x, 50, update="dpmpp2m", return_x0=True)   (B = 8 only: one slot per iteration, the trajectory)

at B = 8 and B = 1, 256 x 256, 50 of 50 timesteps, full-width DDIM-variant network with random-init weights.  The arms are
interleaved (ddim, dpmpp2m, [trajectory,] ddim, ...) so that clock drift hits all alike; median [min - max] of at least 5 timed
calls per arm after 2 warm-ups is reported, never a single run, and the ratio of the medians stands next to the DDIM arm's own
spread.  A second pass brackets every kernel with events (mi_profile_begin) and reports the out-conv kernels' own time per launch.

    python tools/dpm_update_ab.py [--reps 5] [--warmup 2] > profiles/dpm_update_ab.json

Prints ONE JSON object; `mi_source_hash` names the library build the numbers belong to."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import midd_loader  # noqa: E402

midd_loader.load()
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

SIZE, STEPS = 256, 50
ARMS = {"ddim": {"update": "ddim"}, "dpmpp2m": {"update": "dpmpp2m"}, "dpmpp2m_return_x0": {"update": "dpmpp2m", "return_x0": True}}


def timed_calls(den, x, arms, reps, warmup):
    """-> arm -> ms per call of every timed call, the arms interleaved."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = {name: [] for name in arms}
    for rep in range(warmup + reps):
        for name in arms:
            ev[0].record()
            den.denoise(x, STEPS, **ARMS[name])
            ev[1].record()
            ev[1].synchronize()
            if rep >= warmup:
                per[name].append(ev[0].elapsed_time(ev[1]))
    return per


def out_conv_launch_time(den, x, arms):
    """-> arm -> {kernel name: us per launch} of the out-conv kernels of one profiled call."""
    out = {}
    for name in arms:
        den.model.profile_begin()
        den.denoise(x, STEPS, **ARMS[name])
        torch.cuda.synchronize()
        out[name] = {e["name"]: {"us_per_launch": 1e3 * e["total_ms"] / e["launches"], "launches": e["launches"]}
                     for e in den.model.profile_end() if "out_conv" in e["name"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed calls per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("dpm_update_ab.py needs a GPU")
    model = UNetDiffusion()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(UNetConfig(), seed=42).items()})
    den = DiffusionDenoiser(model.to("cuda").eval(), noise_steps=STEPS)
    rows = []
    for B in (8, 1):
        arms = list(ARMS) if B == 8 else ["ddim", "dpmpp2m"]
        x = torch.from_numpy(synthetic_xray(B, SIZE, SIZE, seed=77)).cuda()
        per = timed_calls(den, x, arms, a.reps, a.warmup)
        row = {"shape": [B, 1, SIZE, SIZE], "iterations": STEPS}
        for name, t in per.items():
            row[name] = {"ms_per_call": {"median": statistics.median(t), "min": min(t), "max": max(t)}}
        base = row["ddim"]["ms_per_call"]
        for name in arms[1:]:
            row[name + "_over_ddim_time"] = row[name]["ms_per_call"]["median"] / base["median"]
        row["ddim_spread"] = (base["max"] - base["min"]) / base["median"]
        row["out_conv_kernels"] = out_conv_launch_time(den, x, arms[:2])
        rows.append(row)
    print(json.dumps({
        "tool": "tools/dpm_update_ab.py",
        "metric": "wall time of one sampler call (events around the call) under update='dpmpp2m' beside update='ddim' (eta = 0), "
                  "interleaved in one process; and the out-conv kernels' own time per launch from a profiled call of each arm",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "weights": "random-init (make_state_dict seed 42)", "rows": rows}))


if __name__ == "__main__":
    main()
