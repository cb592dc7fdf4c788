"""Same-process, same-box A/B of the two fp16-MFMA arithmetic modes: compute="f16x3" (the default, parity) against compute="f16"
(one product, autocast precision).  For every workload the two models' `denoise` calls are INTERLEAVED (A B A B ...), so that
clock and thermal drift of the box hits both alike; median and spread of the timed calls are reported, never a single run.
Followed by the per-op table of one forward (B = 8, 256 x 256, one program) in each mode.

    python tools/compute_ab.py [--reps 5] [--warmup 2] > profiles/f16_mode_ab.json

Prints ONE JSON object.  Its `dtype` names the arithmetic that was measured against the base, and `mi_source_hash` the library
build the numbers belong to.  (bench.py cannot time this mode: it labels every run that is not f16x3 as "f32".)"""
import argparse
import json
import os
import statistics
import sys
import time

os.environ["MIDD_PROFILE_PER_OP"] = "1"           # per-op entries from mi_profile_end (read once, when the library first profiles)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import midd_loader  # noqa: E402

midd_loader.load()
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, timestep_list  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

# (name, batch, size, inference_steps): the headline workload, the large batch, the large image, two single-image latencies
WORKLOADS = [("B=8 256x256 x50 (headline)", 8, 256, 50), ("B=32 256x256 x50", 32, 256, 50), ("B=8 512x512 x50", 8, 512, 50),
             ("latency B=1 256x256 x50", 1, 256, 50), ("latency B=1 512x512 x9", 1, 512, 8)]
MODES = ("f16x3", "f16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed denoise calls per mode and workload (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compute_ab.py needs a GPU")
    sd = make_state_dict(UNetConfig(), seed=42)
    models = {}
    for mode in MODES:
        m = UNetDiffusion(compute=mode)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
        m.check_status = False                    # no host synchronisation inside the timed calls (as a serving loop would run)
        models[mode] = DiffusionDenoiser(m.cuda().eval(), noise_steps=50)

    rows = []
    for name, B, S, steps in WORKLOADS:
        noisy = torch.from_numpy(synthetic_xray(B, S, S, seed=1234)).cuda()
        iters = len(timestep_list(50, steps))
        times = {mode: [] for mode in MODES}
        for rep in range(a.warmup + a.reps):
            for mode in MODES:                    # interleaved: A B A B
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = models[mode].denoise(noisy, inference_steps=steps)
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[mode].append(1e3 * (time.perf_counter() - t0))
        assert torch.isfinite(out).all()
        row = {"workload": name, "batch": B, "image": [S, S], "iterations": iters}
        for mode in MODES:
            t = times[mode]
            row[mode] = {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "calls": len(t),
                         "images_per_s": 1e3 * B / statistics.median(t)}
        row["f16_over_f16x3_speedup"] = row["f16x3"]["median_ms"] / row["f16"]["median_ms"]
        rows.append(row)
        del noisy
        for d in models.values():
            d.model._workspaces.clear()
        torch.cuda.empty_cache()

    # per-op table of ONE forward (one program on one stream: the spans are the kernels' own times)
    x = torch.from_numpy(synthetic_xray(8, 256, 256, seed=1234)).cuda()
    t = torch.full((8,), 25, dtype=torch.long)
    per_op = {}
    for mode in MODES:
        m = models[mode].model
        m(x, x, t)
        torch.cuda.synchronize()
        acc = {}
        for _ in range(3):                        # three profiled forwards, the fastest span per op
            m.profile_begin()
            m(x, x, t)
            for p in m.profile_end():
                us = 1e3 * p["total_ms"] / p["launches"]
                op, kernel = p["name"].split(" | ", 1)
                cur = acc.get(op)
                acc[op] = (min(us, cur[0]) if cur else us, kernel, p["flops"])
        per_op[mode] = acc
    table, tot = [], {mode: 0.0 for mode in MODES}
    for op, (us3, k3, fl) in per_op["f16x3"].items():
        us1, k1, _ = per_op["f16"][op]
        tot["f16x3"] += us3
        tot["f16"] += us1
        table.append({"op": op, "f16x3_kernel": k3, "f16_kernel": k1, "f16x3_us": round(us3, 1), "f16_us": round(us1, 1),
                      "ratio": round(us3 / us1, 3), "gflop": round(fl / 1e9, 2)})
    result = {
        "tool": "tools/compute_ab.py", "metric": "denoise() wall time per call, f16x3 and f16 interleaved in one process",
        "dtype": "f16 (every MFMA operand rounded once to fp16, one MFMA per product, fp32 accumulate) vs base f16x3 (split-fp16 x3 MFMA)",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "data": "synthetic", "rows": rows,
        "forward_per_op": {"workload": "one forward, B=8 256x256, one program", "sum_us": {k: round(v, 1) for k, v in tot.items()}, "ops": table},
    }
    print(json.dumps(result))


if __name__ == "__main__":
    main()
