"""Same-process, same-box A/B of fused tiled denoising (denoise_tiled_fused: the overlapping tiles agree after every step) against
the unfused call and against the launches its consensus kernel replaces:

  (a) the whole call.  One 1024 x 1024 and one 1024 x 768 image, 9 iterations, tile 256, overlap 32, max_batch 16, DDIM, f16x3.
        A (the base)  denoise_tiled(): every tile runs the whole loop alone, one blend at the end
        B             denoise_tiled_fused(): the steps are the outer loop, one consensus launch per step
      No bar is set: B joins its side streams once per (step, pass) instead of once per pass and adds one launch per step.  The
      ratio is reported beside A's own spread, with the share of the difference that the consensus launches of (b) explain.
      A is this build's denoise_tiled; `--parent-dump` (a file written by `--dump-tiled` under the parent commit's tree and
      library, `--root`) shows that it gives the parent's bits, so that it may stand in for the parent.
  (b) the consensus launch alone, on the tiles of those calls: `n` launches between two events.
        A (the base)  tile_blend + tile_extract, the pair it replaces        B  tile_consensus (with image_out)
        C             a device-to-device copy of the tiles (the stream rate the shape allows)
  (c) the disagreement the feature removes: max and rms, over the pixels under more than one tile, of the spread (max - min over
      the covering tiles) of denoise_tiled's tiles before the blend.  A fact about RANDOM-INIT weights, the only weights there
      are; image quality on trained weights is not measured here.

The shapes are warmed first, the arms ALTERNATE (A B A B ...) so that clock and thermal drift hits both alike, every timed region
is synchronised on both sides, and median [min - max] of at least 5 timed windows is reported, never a single run.

    python tools/tiled_fused_ab.py [--reps 5] [--warmup 2] [--parent-dump parent.npz] > profiles/tiled_fused_ab.json
    python tools/tiled_fused_ab.py --root PARENT_TREE --dump-tiled parent.npz

Prints ONE JSON object; `mi_source_hash` names the library build the numbers belong to."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                           # whose package and library are loaded (default: this tree's)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import midd_loader  # noqa: E402

midd_loader.load()
import midd_amd  # noqa: E402
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, timestep_list  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

SHAPES, T, O, INFERENCE_STEPS, MAX_BATCH = ((1024, 1024), (1024, 768)), 256, 32, 8, 16      # timestep_list(50, 8): 9 iterations


def summary(t, unit="ms"):
    return {f"median_{unit}": statistics.median(t), f"min_{unit}": min(t), f"max_{unit}": max(t), f"spread_{unit}": max(t) - min(t), "windows": len(t)}


def verdict(sa, sb, unit):
    m, s = f"median_{unit}", f"spread_{unit}"
    return {"B_over_A_time": sb[m] / sa[m], "A_spread_over_A_median": sa[s] / sa[m],
            "B_faster_than_A_beyond_spread_of_A": bool(sa[m] - sb[m] > sa[s]),
            "B_slower_than_A_beyond_spread_of_A": bool(sb[m] - sa[m] > sa[s])}


def image_of(shape):
    return torch.from_numpy(synthetic_xray(1, shape[0], shape[1], seed=1234)).cuda()


def disagreement(tiles, plan, H, W):
    """(max, rms, pixels) of max - min over the covering tiles, over the pixels of one image that lie under more than one tile."""
    hi = torch.full((H, W), -float("inf"), device=tiles.device)
    lo = torch.full((H, W), float("inf"), device=tiles.device)
    cover = torch.zeros((H, W), device=tiles.device)
    nx = len(plan.origins_x)
    for ky, y0 in enumerate(plan.origins_y):
        for kx, x0 in enumerate(plan.origins_x):
            t = tiles[0, ky * nx + kx, 0]
            hi[y0:y0 + T, x0:x0 + T] = torch.maximum(hi[y0:y0 + T, x0:x0 + T], t)
            lo[y0:y0 + T, x0:x0 + T] = torch.minimum(lo[y0:y0 + T, x0:x0 + T], t)
            cover[y0:y0 + T, x0:x0 + T] += 1
    d = (hi - lo)[cover > 1].double()
    return float(d.max()), float(d.pow(2).mean().sqrt()), int(d.numel())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed windows per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--root", default=None, help="the tree whose package and library run (default: this one)")
    ap.add_argument("--dump-tiled", default=None, metavar="OUT.npz", help="write denoise_tiled's images of the two shapes and exit")
    ap.add_argument("--parent-dump", default=None, metavar="IN.npz", help="a --dump-tiled file of the parent commit: compared bit for bit")
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("tiled_fused_ab.py needs a GPU")
    m = UNetDiffusion(variant="ddim")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state_dict(UNetConfig(variant="ddim"), seed=42).items()})
    m.check_status = False                        # no host synchronisation inside the timed calls (as a serving loop would run)
    den = DiffusionDenoiser(m.cuda().eval(), noise_steps=50)
    kw = dict(inference_steps=INFERENCE_STEPS, tile=T, overlap=O, max_batch=MAX_BATCH)
    iterations = len(timestep_list(50, INFERENCE_STEPS))
    if a.dump_tiled:
        out = {f"{h}x{w}": den.denoise_tiled(image_of((h, w)), **kw).image.cpu().numpy() for h, w in SHAPES}
        np.savez(a.dump_tiled, mi_source_hash=native.kernel_source_hash(), **out)
        print(json.dumps({"dumped": a.dump_tiled, "mi_source_hash": native.kernel_source_hash()}))
        return
    parent = np.load(a.parent_dump) if a.parent_dump else None
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    calls, launches, gaps = [], [], []
    for H, W in SHAPES:
        image = image_of((H, W))
        plan = midd_amd.tile_plan(H, W, T, O)
        K = len(plan.origins_y) * len(plan.origins_x)
        arms = {"A": lambda: den.denoise_tiled(image, return_tiles=True, **kw), "B": lambda: den.denoise_tiled_fused(image, return_tiles=True, **kw)}
        times = {name: [] for name in arms}
        outs = {}
        for rep in range(a.warmup + a.reps):
            for name, fn in arms.items():         # alternating: A B A B
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[name] = fn()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    times[name].append(1e3 * (time.perf_counter() - t0))
        key = f"{H}x{W}"
        call = {"variant": "ddim", "image": [H, W], "tile": T, "overlap": O, "tiles": K, "iterations": iterations, "max_batch": MAX_BATCH,
                "passes_per_step": -(-K // MAX_BATCH),
                "A_is": "denoise_tiled(): every tile runs the whole loop alone, one blend at the end (the base)",
                "B_is": "denoise_tiled_fused(): steps outer, one tile_consensus launch per step",
                "A": summary(times["A"]), "B": summary(times["B"]),
                "A_gives_the_parent_librarys_bits": None if parent is None else bool(np.array_equal(parent[key].view(np.int32),
                                                                                                    outs["A"].image.cpu().numpy().view(np.int32))),
                "parent_mi_source_hash": None if parent is None else str(parent["mi_source_hash"]),
                "fused_tiles_equal_extract_of_the_image": bool(torch.equal(outs["B"].tiles, midd_amd.tile_extract(outs["B"].image, T, O))),
                "max_abs_fused_minus_unfused": float((outs["A"].image - outs["B"].image).abs().max()),
                "tiled_fused_workspace_bytes": den.model.tiled_fused_workspace_bytes(1, H, W, T, O, MAX_BATCH, tiles_external=True),
                "tiled_workspace_bytes": den.model.tiled_workspace_bytes(1, H, W, T, O, MAX_BATCH, tiles_external=True)}
        call.update(verdict(call["A"], call["B"], "ms"))

        # (c) what the unfused tiles disagree about, before the blend hides it
        mx, rms, pixels = disagreement(outs["A"].tiles, plan, H, W)
        fmx, _, _ = disagreement(outs["B"].tiles, plan, H, W)
        gaps.append({"image": [H, W], "shared_pixels": pixels, "unfused_max": mx, "unfused_rms": rms, "fused_max": fmx,
                     "is": "max - min over the covering tiles of denoise_tiled's tiles (before the blend), over the pixels under more than one "
                           "tile; random-init weights; image quality on trained weights is not measured"})

        # (b) the consensus launch alone beside the launches it replaces, on the tiles of the call
        src = outs["A"].tiles.clone()
        work, blended, copy = src.clone(), torch.empty_like(image), torch.empty_like(src)
        n = 500

        def pair():
            native.check(lib.mi_tile_blend(work.data_ptr(), 1, 1, H, W, T, T, O, O, blended.data_ptr(), stream))
            native.check(lib.mi_tile_extract(blended.data_ptr(), 1, 1, H, W, T, T, O, O, 0, K, work.data_ptr(), stream))

        def consensus():
            native.check(lib.mi_tile_consensus(work.data_ptr(), 1, 1, H, W, T, T, O, O, blended.data_ptr(), stream))

        variants = {"A": pair, "B": consensus, "C": lambda: copy.copy_(work)}
        per = {name: [] for name in variants}
        for rep in range(a.warmup + a.reps):
            for name, fn in variants.items():     # alternating windows
                ev[0].record()
                for _ in range(n):
                    fn()
                ev[1].record()
                ev[1].synchronize()
                if rep >= a.warmup:
                    per[name].append(1e3 * ev[0].elapsed_time(ev[1]) / n)
        work.copy_(src)
        pair()
        want = (work.clone(), blended.clone())
        work.copy_(src)
        consensus()
        same = bool(torch.equal(work.view(torch.int32), want[0].view(torch.int32)) and torch.equal(blended.view(torch.int32), want[1].view(torch.int32)))
        tile_bytes, plane = K * T * T * 4, H * W * 4
        shared = float(np.mean(np.outer(np.bincount(np.concatenate([np.arange(o, o + T) for o in plan.origins_y]), minlength=H) > 1,
                                        np.ones(W, bool)) |
                               np.outer(np.ones(H, bool), np.bincount(np.concatenate([np.arange(o, o + T) for o in plan.origins_x]), minlength=W) > 1)))
        row = {"image": [H, W], "tiles": K, "launches_per_timed_window": n,
               "A_is": "tile_blend_kernel + tile_extract_kernel, the pair the consensus replaces (the base)",
               "B_is": "tile_consensus_kernel, in place, with image_out", "C_is": "a device-to-device copy of the tiles (torch copy_)",
               "A": summary(per["A"], "us"), "B": summary(per["B"], "us"), "C": summary(per["C"], "us"),
               "algorithmic_bytes": {"A": 2 * tile_bytes + 2 * plane, "B": 2 * tile_bytes + plane, "C": 2 * tile_bytes},
               "share_of_pixels_under_more_than_one_tile": shared,
               "consensus_equals_the_pair_bit_for_bit": same,
               "note": "cache-resident shapes (the tiles are 5 - 7 MB against a 256 MB last-level cache), as in the call itself"}
        row["GB_per_s_at_median"] = {k: row["algorithmic_bytes"][k] / (row[k]["median_us"] * 1e-6) / 1e9 for k in ("A", "B", "C")}
        row.update(verdict(row["A"], row["B"], "us"))
        launches.append(row)
        extra = call["B"]["median_ms"] - call["A"]["median_ms"]
        call["B_minus_A_ms"] = extra
        call["consensus_launches_ms"] = iterations * row["B"]["median_us"] * 1e-3
        call["share_of_B_minus_A_explained_by_the_consensus_launches"] = None if extra <= 0 else call["consensus_launches_ms"] / extra
        call["joins"] = {"A": -(-K // MAX_BATCH), "B": iterations * -(-K // MAX_BATCH)}
        calls.append(call)

    print(json.dumps({
        "tool": "tools/tiled_fused_ab.py",
        "metric": "(a) wall time of one image as denoise_tiled() (A, the base) and as denoise_tiled_fused() (B); (b) device time per launch: "
                  "blend + extract (A), the consensus kernel (B), a copy of the tiles (C); (c) the spread of the unfused tiles over shared "
                  "pixels; arms alternate in one process",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "compute": m.compute, "reps": a.reps, "warmup": a.warmup, "data": "synthetic", "weights": "random-init (seed 42)",
        "call": calls, "consensus_launch": launches, "disagreement": gaps}))


if __name__ == "__main__":
    main()
