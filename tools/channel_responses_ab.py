"""Time of the channel-responses call next to what a caller without it would run, in one process:

    mi_channel_responses   (the call: one launch per 512 locations, preallocated outputs)
    torch                  (the no-kernel alternative on the same device: gather the ROIs to [N L, R^2] with one index, convert to
                            float64 and multiply by U^T; its summation order is whatever the float64 GEMM picks)
    copy                   (a device copy of the planes)

at N = 128 planes of 512 x 512 with R = 64, L = 49 (a 7 x 7 grid of non-overlapping ROIs, half an ROI in from the border), C = 10, and
at N = 16 planes of 256 x 256 with R = 32, L = 64 (the whole non-overlapping grid), C = 6.  No network runs for these: the planes are
clip(0.5 + 0.1 n, 0, 1), the channels Laguerre-Gauss.  `n` launches sit between two events, the arms alternate so that clock drift hits all alike, and median [min - max] of at least 5 timed windows is
reported, never a single run.  Beside the call's time stands the rate of separately rounded double multiply-add pairs it amounts
to, N L C R^2.

Then a complete study (DiffusionDenoiser.detectability, the command-line tool's topology, random weights) beside the same 2 * trials
images as plain denoise passes of the same max_batch: what the study costs over the sampler runs it contains.

    python tools/channel_responses_ab.py [--reps 5] [--warmup 2] [--out profiles/channel_responses_ab.json]

Writes ONE JSON object (and prints it); `mi_source_hash` names the library build the numbers belong to."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import midd_loader  # noqa: E402

midd_loader.load()
import midd_amd  # noqa: E402
from midd_amd import native  # noqa: E402

SHAPES = [(128, 512, 512, 64, 10, 7), (16, 256, 256, 32, 6, 8)]      # (N, H, W, R, C, G); L = G x G non-overlapping ROIs
STUDY = dict(size=256, trials=8, inference_steps=5, max_batch=16, roi=32, n_channels=6)


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


def spread(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def study_row(reps, warmup):
    """The study and its sampler passes alone, alternating, host clock around work that ends in a synchronise."""
    from midd_amd import DiffusionDenoiser, UNetDiffusion
    size, trials = STUDY["size"], STUDY["trials"]
    torch.manual_seed(3)
    model = UNetDiffusion(in_channels=1, model_channels=48, channel_mult=(1, 2, 3, 4), num_res_blocks=2, attention_resolutions=(3,),
                          dropout=0.0, time_emb_dim=192, variant="cddpm").to("cuda").eval()
    d = DiffusionDenoiser(model, noise_steps=50)
    from midd_amd.weights import synthetic_xray
    bg = torch.from_numpy(synthetic_xray(1, size, size, seed=5)[0, 0]).clamp(0.05, 0.9).cuda()
    g = np.arange(13, dtype=np.float64) - 6.0
    blob = np.exp(-(g[:, None] ** 2 + g[None, :] ** 2) / (2.0 * 3.0 ** 2)).astype(np.float32)
    kw = dict(inference_steps=STUDY["inference_steps"], trials=trials, roi=STUDY["roi"], n_channels=STUDY["n_channels"], amplitude=0.05,
              sigma=0.05, seed=11, max_batch=STUDY["max_batch"])
    first = d.detectability(bg, blob, return_images=True, **kw)
    noisy = first.images[0]

    def study():
        d.detectability(bg, blob, **kw)

    def passes():
        for lo in range(0, 2 * trials, STUDY["max_batch"]):
            d.denoise(noisy[lo:lo + STUDY["max_batch"]], STUDY["inference_steps"], seed=11, sample_offset=lo)

    per = {"study": [], "denoise_passes": []}
    for rep in range(warmup + reps):
        for name, fn in (("study", study), ("denoise_passes", passes)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep >= warmup:
                per[name].append(1e3 * (time.perf_counter() - t0))
    return {"what": "DiffusionDenoiser.detectability (cddpm, the command-line topology, random weights) beside its 2 * trials images as "
                    "plain denoise passes; host clock, synchronised, alternating",
            **STUDY, "locations": int(first.centres.shape[0]),
            "ms": {name: spread(t) for name, t in per.items()},
            "study_minus_passes_ms_at_median": statistics.median(per["study"]) - statistics.median(per["denoise_passes"]),
            "dprime": {"noisy": first.noisy.dprime, "denoised": first.denoised.dprime},
            "note": "random-init weights: the d' values say nothing about a trained denoiser"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed windows per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "channel_responses_ab.json"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("channel_responses_ab.py needs a GPU")
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device="cuda").manual_seed(7)
    rows = []
    for N, H, W, R, Cn, G in SHAPES:
        if G == H // R == W // R:
            centres = midd_amd.roi_grid(H, W, R)
        else:                                       # G x G ROIs, half an ROI in from the border
            at = R + R * np.arange(G)
            centres = np.ascontiguousarray(np.stack(np.meshgrid(at, at, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int32))
        L = int(centres.shape[0])
        u = midd_amd.laguerre_gauss_channels(R, Cn)
        x = (0.5 + 0.1 * torch.randn((N, H, W), device="cuda", generator=gen)).clamp_(0, 1)
        ud = torch.from_numpy(u).cuda()
        ut = ud.reshape(Cn, R * R).t().contiguous()
        out = torch.empty((N, L, Cn), dtype=torch.float64, device="cuda")
        flags = torch.empty((N, L), dtype=torch.int32, device="cuda")
        copy_dst = torch.empty_like(x)
        cptr = centres.ctypes.data_as(C.POINTER(C.c_int32))
        yy, xx = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
        flat = ((centres[:, 0, None, None] - R // 2 + yy[None]) * W + (centres[:, 1, None, None] - R // 2 + xx[None])).reshape(L * R * R)
        index = torch.from_numpy(flat.astype(np.int64)).cuda()

        def call():
            native.check(lib.mi_channel_responses(x.data_ptr(), N, H, W, cptr, L, R, ud.data_ptr(), Cn, out.data_ptr(), flags.data_ptr(), stream))

        def torch_arm():
            return (x.reshape(N, H * W)[:, index].reshape(N * L, R * R).double() @ ut).reshape(N, L, Cn)

        def copy():
            copy_dst.copy_(x)

        call()
        alt = torch_arm()
        torch.cuda.synchronize()
        err = float((alt - out).abs().max())
        pairs = N * L * Cn * R * R
        n = 20 if pairs > (1 << 26) else 50
        per = windows({"mi_channel_responses": call, "torch": torch_arm, "copy": copy}, n, a.reps, a.warmup)
        row = {"planes": [N, H, W], "roi": R, "locations": L, "channels": Cn, "launches_per_timed_window": n, "multiply_add_pairs": pairs,
               "max_abs_difference_of_the_two_arms": err}
        for name, t in per.items():
            row[name] = {"us_per_launch": spread(t)}
        t = per["mi_channel_responses"]
        row["mi_channel_responses"]["pairs_per_s"] = {"median": pairs / (statistics.median(t) * 1e-6), "min": pairs / (max(t) * 1e-6),
                                                      "max": pairs / (min(t) * 1e-6)}
        row["mi_channel_responses"]["requested_bytes"] = N * L * R * R * 4 * ((Cn + 7) // 8) + ((N + 7) // 8) * L * Cn * R * R * 8
        row["call_over_torch_time"] = statistics.median(t) / statistics.median(per["torch"])
        row["call_over_copy_time"] = statistics.median(t) / statistics.median(per["copy"])
        rows.append(row)
        del x, out, flags, copy_dst, index, alt
    result = {
        "tool": "tools/channel_responses_ab.py",
        "metric": "time per call of mi_channel_responses beside the torch alternative (gather to [N L, R^2] float64, multiply by U^T) and a "
                  "device copy of the planes, alternating in one process; the call's rate of separately rounded double multiply-add pairs, "
                  "N L C R^2; then a complete detectability study beside its sampler passes alone",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
        "data": "clip(0.5 + 0.1 n, 0, 1) planes, Laguerre-Gauss channels of width R / 4, the non-overlapping ROI grid",
        "requested_bytes": "what the launches ask for -- every ROI once per channel block, every channel block once per workgroup of 8 planes "
                           "-- not what reaches HBM (the caches serve the repeats)",
        "unmeasured": ["HBM and L2 traffic of the kernel (no counter pass was run)", "d' on trained weights: only random-init weights exist"],
        "rows": rows, "study": study_row(a.reps, a.warmup)}
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
