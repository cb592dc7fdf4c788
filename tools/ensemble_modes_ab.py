"""Time of the ensemble-modes launches next to the scores launch over the same members, in one process:

    mi_ensemble_gram       (the call: zero the counter, [K > 8: the mean pre-pass,] the Gram kernel, the chunk sums)
    mi_ensemble_project    (three modes)
    mi_ensemble_scores     (five levels, no crps_map)
    a device copy of the members

for one 256x256 image with K = 8, 32 and 64 members, a batch of 8 at 256x256 with K = 8, and one 2500x2048 image with K = 8.  No
network runs: the members are clip(0.5 + 0.35 n, 0, 1).  Every launch is the C call with preallocated outputs; `n` launches sit
between two events, the arms alternate so that clock drift hits all alike, and median [min - max] of at least 5 timed windows is
reported, never a single run.  Beside the Gram time stands the rate of double multiply-add pairs it amounts to, chw K (K + 1) / 2 an
image, and -- if tools/mb/f64_rate was built (hipcc -O3 --offload-arch=gfx950 tools/mb/f64_rate.hip -o tools/mb/f64_rate) -- what a
register-only loop of such pairs reaches on the same device.

    python tools/ensemble_modes_ab.py [--reps 5] [--warmup 2] [--out profiles/ensemble_modes_ab.json]

Writes ONE JSON object (and prints it); `mi_source_hash` names the library build the numbers belong to."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import midd_loader  # noqa: E402

midd_loader.load()
import midd_amd  # noqa: E402
from midd_amd import native  # noqa: E402
from midd_amd.ensemble import gram_eigen  # noqa: E402

LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)
MODES = 3
SHAPES = [(1, 256, 256, 8), (1, 256, 256, 32), (1, 256, 256, 64), (8, 256, 256, 8), (1, 2500, 2048, 8)]      # (B, H, W, K)


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


def register_rate():
    """The JSON line of tools/mb/f64_rate, or None where the program was not built."""
    exe = os.path.join(ROOT, "tools", "mb", "f64_rate")
    if not os.path.exists(exe):
        return None
    return json.loads(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed windows per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_modes_ab.json"))
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_modes_ab.py needs a GPU")
    peak = register_rate()          # (a child process of its own, before this one opens the device)
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    q = (C.c_double * len(LEVELS))(*LEVELS)
    nq = len(LEVELS)
    gen = torch.Generator(device="cuda").manual_seed(7)
    rows = []
    for B, H, W, K in SHAPES:
        chw = H * W
        n = 50 if chw * B * K <= (1 << 24) else 10
        samples = (0.5 + 0.35 * torch.randn((B, K, 1, H, W), device="cuda", generator=gen)).clamp_(0, 1)
        truth = (0.5 + 0.35 * torch.randn((B, 1, H, W), device="cuda", generator=gen)).clamp_(0, 1)
        copy_dst = torch.empty_like(samples)
        out = torch.empty((B, MODES, 1, H, W), device="cuda")
        graw = torch.zeros(B * (K * K + 1), dtype=torch.int64, device="cuda")
        gws_bytes = lib.mi_ensemble_gram_workspace_bytes(B, K, chw)
        gws = torch.empty(gws_bytes // 8, dtype=torch.float64, device="cuda")
        sraw = torch.zeros(B * (4 + 1 + 2 * K + 1 + 2 * nq), dtype=torch.int64, device="cuda")
        sbase = sraw.data_ptr()
        o_inv, o_rank, o_cnt = sbase + 8 * B * 4, sbase + 8 * B * 5, sbase + 8 * B * (5 + 2 * K + 1)
        sws_bytes = lib.mi_ensemble_scores_workspace_bytes(B, K, chw)
        sws = torch.empty(sws_bytes // 8, dtype=torch.float64, device="cuda")

        def gram():
            native.check(lib.mi_ensemble_gram(samples.data_ptr(), B, K, chw, graw.data_ptr(), graw.data_ptr() + 8 * B * K * K, gws.data_ptr(), gws_bytes, stream))

        gram()
        torch.cuda.synchronize()
        _, _, weights = gram_eigen(graw[:B * K * K].cpu().view(torch.float64).reshape(B, K, K).numpy(), MODES)
        wd = torch.from_numpy(weights).cuda()

        def project():
            native.check(lib.mi_ensemble_project(samples.data_ptr(), B, K, chw, wd.data_ptr(), MODES, out.data_ptr(), stream))

        def scores():
            native.check(lib.mi_ensemble_scores(samples.data_ptr(), truth.data_ptr(), B, K, chw, q, nq, sbase, o_inv, o_rank, o_cnt, None,
                                                sws.data_ptr(), sws_bytes, stream))

        def copy():
            copy_dst.copy_(samples)

        plane = B * chw * 4
        mean_bytes = 2 * plane if K > 8 else 0                       # K > 8: the double means, 8 bytes an element
        nb = (K + 7) // 8
        # K <= 8: every member once.  K > 8: the pre-pass reads every member and writes the means; pair (bi, bj) reads its 16 (8)
        # members and the means: over all pairs every member nb times, the means nb (nb + 1) / 2 times -- what the launches ask
        # for, not what reaches HBM (the caches serve the repeats)
        gram_bytes = K * plane if K <= 8 else K * plane + mean_bytes + nb * K * plane + nb * (nb + 1) // 2 * mean_bytes
        part_bytes = gws_bytes - mean_bytes                          # the chunk sums: written once, read once by the last launch
        nbytes = {"gram": gram_bytes + 2 * part_bytes, "project": (2 * K + MODES) * plane,
                  "scores": (K + 1) * plane + sws_bytes, "copy": 2 * K * plane}
        per = windows({"gram": gram, "project": project, "scores": scores, "copy": copy}, n, a.reps, a.warmup)
        row = {"shape": [B, 1, H, W], "members": K, "modes": MODES, "launches_per_timed_window": n}
        for name, t in per.items():
            med = statistics.median(t)
            row[name] = {"us_per_launch": {"median": med, "min": min(t), "max": max(t)}, "requested_bytes": nbytes[name],
                         "GB_per_s_at_median": nbytes[name] / (med * 1e-6) / 1e9}
        pairs = B * chw * K * (K + 1) // 2
        t = per["gram"]
        row["gram"]["multiply_add_pairs"] = pairs
        row["gram"]["pairs_per_s"] = {"median": pairs / (statistics.median(t) * 1e-6), "min": pairs / (max(t) * 1e-6), "max": pairs / (min(t) * 1e-6)}
        if peak is not None:
            row["gram"]["share_of_register_only_rate"] = row["gram"]["pairs_per_s"]["median"] / peak["pairs_per_s"]["median"]
        row["gram_over_scores_time"] = row["gram"]["us_per_launch"]["median"] / row["scores"]["us_per_launch"]["median"]
        row["gram_over_copy_time"] = row["gram"]["us_per_launch"]["median"] / row["copy"]["us_per_launch"]["median"]
        pm = midd_amd.ensemble_modes(samples, MODES)
        row["result_image_0"] = {"variance": pm.variance[0].tolist(), "explained": pm.explained[0].tolist(), "total_variance": float(pm.total_variance[0])}
        rows.append(row)
        del samples, truth, copy_dst, out, gws, sws
    result = {
        "tool": "tools/ensemble_modes_ab.py",
        "metric": "time per call of mi_ensemble_gram and of mi_ensemble_project (three modes) beside mi_ensemble_scores (five levels) on the same "
                  "members and a device copy of the members, alternating in one process; the Gram call's rate of separately rounded double "
                  "multiply-add pairs, chw K (K + 1) / 2 an image, beside a register-only loop of such pairs (tools/mb/f64_rate.hip)",
        "register_only_pairs": peak if peak is not None else "unmeasured: tools/mb/f64_rate was not built",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "data": "clip(0.5 + 0.35 n, 0, 1), independent members: a flat spectrum, no leading mode",
        "unmeasured": ["HBM traffic of the pair kernel (no counter pass was run)", "the modes of a trained model: only random-init weights exist"],
        "rows": rows}
    text = json.dumps(result, indent=1)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
