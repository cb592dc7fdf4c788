"""Same-process, same-box A/B of the tiled self-ensemble against the public calls it composes:

  (a) the whole call.  One 1024 x 768 image, 9 iterations, all 8 views, tile 256, overlap 32, max_batch 16, DDIM.
        A (the base)  eight denoise_tiled() calls on torch-viewed copies + the torch un-view of every image + ensemble_reduce()
        B             one denoise_tiled_self_ensemble() call: views outer, a view copy per round, ONE blend-unview-reduce launch
  (b) the final launch alone, on the same tile tensors, for the flips and for d4: `n` launches between two events.
        A (the base)  tile_blend x views (each in its view's frame), the un-view copies, ensemble_reduce -- the parent's kernels
        B             tile_blend_unview_reduce, with and without samples_out

The shapes are warmed first, the arms ALTERNATE (A B A B ...) so that clock and thermal drift hits both alike, every timed region
is synchronised on both sides, and median [min - max] of at least 5 timed windows is reported, never a single run.

    python tools/tiled_self_ensemble_ab.py [--reps 5] [--warmup 2] > profiles/tiled_self_ensemble_ab.json

Prints ONE JSON object; `mi_source_hash` names the library build the numbers belong to."""
import argparse
import ctypes
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
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

H, W, T, O, STEPS, MAX_BATCH = 1024, 768, 256, 32, 9, 16
D4, FLIPS = tuple(range(8)), (0, 1, 2, 3)


def tview(x, g):
    u = x.transpose(-1, -2) if g & 4 else x
    if g & 2:
        u = u.flip(-2)
    if g & 1:
        u = u.flip(-1)
    return u.contiguous()


def tunview(v, g):
    u = v
    if g & 1:
        u = u.flip(-1)
    if g & 2:
        u = u.flip(-2)
    if g & 4:
        u = u.transpose(-1, -2)
    return u.contiguous()


def summary(t, unit="ms"):
    return {f"median_{unit}": statistics.median(t), f"min_{unit}": min(t), f"max_{unit}": max(t), f"spread_{unit}": max(t) - min(t), "windows": len(t)}


def verdict(sa, sb, unit):
    m, s = f"median_{unit}", f"spread_{unit}"
    return {"B_over_A_time": sb[m] / sa[m], "A_spread_over_A_median": sa[s] / sa[m],
            "B_faster_than_A_beyond_spread_of_A": bool(sa[m] - sb[m] > sa[s]),
            "B_slower_than_A_beyond_spread_of_A": bool(sb[m] - sa[m] > sa[s])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed windows per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("tiled_self_ensemble_ab.py needs a GPU")
    image = torch.from_numpy(synthetic_xray(1, H, W, seed=1234)).cuda()
    m = UNetDiffusion(variant="ddim")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state_dict(UNetConfig(variant="ddim"), seed=42).items()})
    m.check_status = False                        # no host synchronisation inside the timed calls (as a serving loop would run)
    den = DiffusionDenoiser(m.cuda().eval(), noise_steps=50)
    kw = dict(inference_steps=STEPS, tile=T, overlap=O, max_batch=MAX_BATCH)

    def composed():
        members = torch.stack([tunview(den.denoise_tiled(tview(image, g), **kw).image, g) for g in D4], dim=1)
        return midd_amd.ensemble_reduce(members)

    def one_call():
        r = den.denoise_tiled_self_ensemble(image, views="d4", **kw)
        return r.mean, r.std

    arms = {"A": composed, "B": one_call}
    times = {name: [] for name in arms}
    outs = {}
    for rep in range(a.warmup + a.reps):
        for name, fn in arms.items():             # alternating: A B A B
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = fn()
            torch.cuda.synchronize()
            if rep >= a.warmup:
                times[name].append(1e3 * (time.perf_counter() - t0))
    plan = midd_amd.tile_plan(H, W, T, O)
    K = len(plan.origins_y) * len(plan.origins_x)
    call = {"variant": "ddim", "image": [H, W], "tile": T, "overlap": O, "tiles_per_view": K, "views": list(D4), "iterations": STEPS,
            "max_batch": MAX_BATCH,
            "A_is": "8 x denoise_tiled(torch view of the image) + torch un-view of every image + ensemble_reduce (the base)",
            "B_is": "one denoise_tiled_self_ensemble(views='d4') call",
            "A": summary(times["A"]), "B": summary(times["B"]),
            "same_bits": bool(torch.equal(outs["A"][0], outs["B"][0]) and torch.equal(outs["A"][1], outs["B"][1])),
            "tiled_self_ensemble_workspace_bytes": den.model.tiled_self_ensemble_workspace_bytes(1, 8, H, W, T, O, MAX_BATCH),
            "tiled_workspace_bytes": den.model.tiled_workspace_bytes(1, H, W, T, O, MAX_BATCH)}
    call.update(verdict(call["A"], call["B"], "ms"))
    compute = m.compute
    del den, m, outs

    # (b) the final launch alone beside the launches it replaces, on the same tensors
    lib = native.lib()
    stream = torch.cuda.current_stream().cuda_stream
    n = 1000                                      # 30 - 170 ms per timed window
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    plane, view_tiles = H * W * 4, K * T * T * 4
    kernels = []
    for codes in (FLIPS, D4):
        G = len(codes)
        tiles = torch.rand((G, 1, K, 1, T, T), device="cuda")
        mean, std = torch.empty_like(image), torch.empty_like(image)
        samples = torch.empty((1, G, 1, H, W), device="cuda")
        blended = [torch.empty((1, 1, W, H) if g & 4 else (1, 1, H, W), device="cuda") for g in codes]
        code_arg = (ctypes.c_int32 * G)(*codes)

        def fused(with_samples):
            def launch():
                native.check(lib.mi_tile_blend_unview_reduce(tiles.data_ptr(), 1, 1, H, W, T, T, O, O, code_arg, G, mean.data_ptr(), std.data_ptr(),
                                                             samples.data_ptr() if with_samples else None, stream))
            return launch

        def composition():
            for k, g in enumerate(codes):
                Hv, Wv = (W, H) if g & 4 else (H, W)
                native.check(lib.mi_tile_blend(tiles.data_ptr() + k * view_tiles, 1, 1, Hv, Wv, T, T, O, O, blended[k].data_ptr(), stream))
                dims = [d for d, bit in ((-1, 1), (-2, 2)) if g & bit]               # the un-view with the fewest torch kernels: one flip
                u = blended[k].flip(dims) if dims else blended[k]                  # copy, the transpose as a stride view, and the
                samples[:, k].copy_(u.transpose(-1, -2) if g & 4 else u)           # copy into the member's slot
            native.check(lib.mi_ensemble_reduce(samples.data_ptr(), 1, G, H * W, mean.data_ptr(), std.data_ptr(), stream))

        variants = {"A": composition, "B": fused(False), "B_with_samples": fused(True)}
        per = {name: [] for name in variants}
        for rep in range(a.warmup + a.reps):
            for name, fn in variants.items():      # alternating windows
                ev[0].record()
                for _ in range(n):
                    fn()
                ev[1].record()
                ev[1].synchronize()
                if rep >= a.warmup:
                    per[name].append(1e3 * ev[0].elapsed_time(ev[1]) / n)
        composition()
        want = (mean.clone(), std.clone(), samples.clone())
        fused(True)()
        same = bool(torch.equal(mean, want[0]) and torch.equal(std, want[1]) and torch.equal(samples, want[2]))
        tile_bytes = G * view_tiles
        row = {"views": list(codes), "launches_per_timed_window": n,
               "A_is": f"{G} x tile_blend_kernel + the torch un-view and copy of every image + ensemble_reduce_kernel (the parent's kernels)",
               "B_is": "tile_blend_unview_reduce_kernel: mean and std, the aligned members never stored",
               "A": summary(per["A"], "us"), "B": summary(per["B"], "us"), "B_with_samples": summary(per["B_with_samples"], "us"),
               "algorithmic_bytes": {"A": tile_bytes + G * plane + 2 * G * plane + G * plane + 2 * plane, "B": tile_bytes + 2 * plane,
                                     "B_with_samples": tile_bytes + (2 + G) * plane},
               "fused_equals_composition_bit_for_bit": same,
               "note": "cache-resident shapes (the tiles of 8 views are 25 MB against a 256 MB last-level cache), as in the call itself; A's "
                       "un-view runs as torch kernels (flip / transpose copies), identity views as one copy"}
        row["GB_per_s_at_median"] = {k: row["algorithmic_bytes"][k] / (row[k]["median_us"] * 1e-6) / 1e9 for k in ("A", "B", "B_with_samples")}
        row.update(verdict(row["A"], row["B"], "us"))
        kernels.append(row)

    print(json.dumps({
        "tool": "tools/tiled_self_ensemble_ab.py",
        "metric": "(a) wall time of 8 views x tiles x iterations as eight denoise_tiled() calls + un-view + ensemble_reduce (A, the base) and as "
                  "one denoise_tiled_self_ensemble() call (B); (b) device time per final launch, composition (A) against the fused kernel (B); "
                  "arms alternate in one process",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "compute": compute, "reps": a.reps, "warmup": a.warmup, "data": "synthetic", "call": call, "final_launch": kernels}))


if __name__ == "__main__":
    main()
