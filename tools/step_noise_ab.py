"""Same-process, same-box A/B of the cddpm sampler's two noise sources:

    A  seed=None   torch.randn of the whole [n_iters,B,C,H,W] tensor up front, read by out_conv_kernel (the behaviour before seeds)
    B  seed=s      drawn inside the fused update by out_conv_seeded_kernel (mi_denoise_seeded); no noise tensor

For every workload the `denoise` calls are INTERLEAVED (A B A B ...), so that clock and thermal drift of the box hits both
alike; median and spread of the timed calls are reported, never a single run.  A's time includes its torch.randn: that is what
a caller of the unseeded path pays.  Then, in a run of its own with the library's event profiler on (it slows the host: these
spans are not end-to-end numbers), the time per launch of the out_conv variants, and of step_noise_fill_kernel over ONE
iteration's [B,C,H,W] -- what a per-iteration fill into a scratch tensor would add to the unseeded kernel.

    python tools/step_noise_ab.py [--reps 5] [--warmup 2] > profiles/step_noise_ab.json

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
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, timestep_list  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

# (name, batch, size, inference_steps): the headline batch, the command-line tool's default size, the large image at batch 8
WORKLOADS = [("B=8 256x256 x50", 8, 256, 50), ("B=1 512x512 x50 (cli default size)", 1, 512, 50), ("B=8 512x512 x50", 8, 512, 50)]
SEED = 0x1234567890ABCDEF
ARMS = {"A_unseeded": {}, "B_seeded": {"seed": SEED}}


def summary(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "spread_ms": max(t) - min(t), "calls": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed denoise calls per arm and workload (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("step_noise_ab.py needs a GPU")
    cfg = UNetConfig(variant="cddpm")
    m = UNetDiffusion(variant="cddpm")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state_dict(cfg, seed=42).items()})
    m.check_status = False                        # no host synchronisation inside the timed calls (as a serving loop would run)
    den = DiffusionDenoiser(m.cuda().eval(), noise_steps=50)

    rows = []
    for name, B, S, steps in WORKLOADS:
        noisy = torch.from_numpy(synthetic_xray(B, S, S, seed=1234)).cuda()
        iters = len(timestep_list(50, steps))
        times = {arm: [] for arm in ARMS}
        for rep in range(a.warmup + a.reps):
            for arm, kw in ARMS.items():          # interleaved: A B A B
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = den.denoise(noisy, inference_steps=steps, **kw)
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[arm].append(1e3 * (time.perf_counter() - t0))
                assert torch.isfinite(out).all()
                del out
        row = {"workload": name, "batch": B, "image": [S, S], "iterations": iters,
               "noise_tensor_bytes_A": iters * B * S * S * 4}
        for arm in ARMS:
            row[arm] = summary(times[arm])
        sa, sb = row["A_unseeded"], row["B_seeded"]
        row["B_over_A_time"] = sb["median_ms"] / sa["median_ms"]
        row["run_to_run_spread_ms"] = max(sa["spread_ms"], sb["spread_ms"])
        row["B_slower_than_A_beyond_spread"] = bool(sb["median_ms"] - sa["median_ms"] > row["run_to_run_spread_ms"])

        # per-symbol spans (MI_NO_SPLIT: one program on one stream, so a span is the kernel's own time), profiler on
        spans = {}
        for arm, kw in ARMS.items():
            noise = None if kw else 0.5 * torch.randn((iters,) + tuple(noisy.shape), device="cuda")
            m.profile_begin()
            m.run_sampler(noisy, timestep_list(50, steps), den.beta, den.alpha, den.alpha_hat, clamp_eps=False,
                          no_split=True, step_noise=noise, **kw)
            for p in m.profile_end():
                if "out_conv" in p["name"]:
                    spans.setdefault(p["name"], {"launches": 0, "total_ms": 0.0})
                    spans[p["name"]]["launches"] += p["launches"]
                    spans[p["name"]]["total_ms"] += p["total_ms"]
            del noise
        for v in spans.values():
            v["us_per_launch"] = 1e3 * v["total_ms"] / v["launches"]
        row["out_conv_spans_no_split"] = spans
        # one iteration's fill, as a scratch-tensor variant would launch it before every unseeded out_conv
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        fills = []
        for rep in range(a.warmup + a.reps):
            ev[0].record()
            midd_amd.step_noise(SEED, 1, noisy.shape, sample_offset=rep)
            ev[1].record()
            ev[1].synchronize()
            if rep >= a.warmup:
                fills.append(1e3 * ev[0].elapsed_time(ev[1]))
        row["step_noise_fill_one_iteration_us"] = {"median": statistics.median(fills), "min": min(fills), "max": max(fills),
                                                   "includes": "torch.empty of the destination and the launch"}
        rows.append(row)
        del noisy
        m._workspaces.clear()
        torch.cuda.empty_cache()

    print(json.dumps({
        "tool": "tools/step_noise_ab.py",
        "metric": "denoise() wall time per call on the cddpm model, unseeded (A, includes its torch.randn) and seeded (B) interleaved in one process",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "compute": m.compute, "reps": a.reps, "warmup": a.warmup, "data": "synthetic", "rows": rows}))


if __name__ == "__main__":
    main()
