"""Same-box measurements of slots as virtual samples and of tiled tickets (mi_denoise_slots_virtual, SamplerSession.submit_tiled)
-> profiles/slot_tickets_ab.json.

    uniform   what the wider slot record costs: run_slots with every column equal to the timestep list, on the PARENT commit's
              library (--parent-library, a build of the commit before the feature: 32-byte records) and on this tree's (48-byte
              records, the same call with both tables absent), at B = 8, 256x256, 50 iterations and B = 1, 512x512, 9 iterations.
              A library is fixed per process (MIDD_LIBRARY), so the arms are separate worker processes, ALTERNATED (parent new
              parent new); every worker warms its shapes, then times whole calls between synchronisations.  The parent's own
              run-to-run spread (its workers, all calls) is recorded beside the ratio.
    tiled     one 1024x1024 image, 9 iterations, tile 256, overlap 32 (25 tiles): a tiled ticket in a 16-slot session against
              denoise_tiled(max_batch=16).  Arms alternate in one process.
    mixed     four uploads of different sizes submitted together -- 512x512, 768x1024, 1024x1024, 2048x2500: 9 + 20 + 25 + 108 tiles
              -- through one 16-slot session against serial denoise_tiled calls in submission order: total time and per-request
              latency (submission -> result on the host side of a synchronisation).  Arms alternate in one process.
    merge     the part files -> one JSON object on stdout.

Each part is a GPU step of its own; run them under their own time limits, chained so that nothing starts after a failure:

    timeout -k 10 500 python tools/slot_tickets_ab.py uniform --parent-library libmidd_parent.so --out out/st_uniform.json \\
     && timeout -k 10 200 python tools/slot_tickets_ab.py tiled --out out/st_tiled.json \\
     && timeout -k 10 400 python tools/slot_tickets_ab.py mixed --out out/st_mixed.json \\
     && python tools/slot_tickets_ab.py merge out/st_uniform.json out/st_tiled.json out/st_mixed.json > profiles/slot_tickets_ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x1234567890ABCDEF
UNIFORM_SHAPES = [(8, 256, 50), (1, 512, 9)]          # (B, side, iterations)
STEPS = 8                                             # inference_steps=8 -> 9 iterations (the server's call)
TILE, OVERLAP, SLOTS = 256, 32, 16
MIXED = [(512, 512), (768, 1024), (1024, 1024), (2048, 2500)]


def summary(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "spread_ms": max(t) - min(t), "calls": len(t)}


def _setup(parent: bool = False):
    import torch
    import midd_loader
    midd_loader.load()
    from midd_amd import native
    if parent:                                        # the parent's library has every symbol but the new one
        native.SYMBOLS[:] = [s for s in native.SYMBOLS if s[0] != "mi_denoise_slots_virtual"]
    from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion
    from midd_amd.weights import make_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("slot_tickets_ab.py needs a GPU")
    m = UNetDiffusion(variant="cddpm")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in make_state_dict(UNetConfig(variant="cddpm"), seed=42).items()})
    m.check_status = False                            # no host synchronisation inside the timed calls
    return torch, native, DiffusionDenoiser(m.cuda().eval(), noise_steps=50)


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), out


# ------------------------------------------------------------------------------ uniform: one worker = one library
def worker_uniform(a):
    torch, native, den = _setup(a.parent)
    from midd_amd import timestep_list
    from midd_amd.weights import synthetic_xray
    out = {"library": native.LIB_PATH, "mi_source_hash": native.kernel_source_hash(), "shapes": []}
    for B, S, iters in UNIFORM_SHAPES:
        x = torch.from_numpy(synthetic_xray(B, S, S, seed=1234)).cuda()
        t_list = timestep_list(50, iters if iters == 50 else iters - 1)
        assert len(t_list) == iters
        rows = [[t] * B for t in t_list]
        times, digest = [], None
        for rep in range(a.warmup + a.reps):
            ms, o = timed(torch, lambda: den.model.run_slots(x, x.clone(), rows, den.beta, den.alpha, den.alpha_hat, clamp_eps=False, seed=SEED))
            if rep >= a.warmup:
                times.append(ms)
            digest = float(o.double().sum())
        out["shapes"].append({"B": B, "side": S, "iterations": iters, "times_ms": times, "sum": digest})
    print("RESULT " + json.dumps(out))


def part_uniform(a):
    lib = os.path.abspath(a.parent_library)
    if not os.path.exists(lib):
        raise SystemExit(f"{lib} not found: build the parent commit's library first")
    runs = []
    for rnd in range(a.rounds):
        for parent in (True, False):                  # alternated: parent new parent new
            env = dict(os.environ)
            if parent:
                env["MIDD_LIBRARY"] = lib
            else:
                env.pop("MIDD_LIBRARY", None)
            cmd = [sys.executable, os.path.abspath(__file__), "worker-uniform", "--reps", str(a.reps), "--warmup", str(a.warmup)] + (["--parent"] if parent else [])
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.worker_timeout)
            if r.returncode != 0:                     # nothing more is started on the GPU after a failure
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"worker (parent={parent}) failed with status {r.returncode}")
            line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1]
            runs.append({"parent": parent, "round": rnd, **json.loads(line[7:])})
    shapes = []
    for i, (B, S, iters) in enumerate(UNIFORM_SHAPES):
        pool = lambda parent: [t for r in runs if r["parent"] == parent for t in r["shapes"][i]["times_ms"]]      # noqa: E731
        base, new = summary(pool(True)), summary(pool(False))
        shapes.append({
            "B": B, "side": S, "iterations": iters, "parent_run_slots": base, "new_run_slots": new,
            "parent_worker_medians_ms": [statistics.median(r["shapes"][i]["times_ms"]) for r in runs if r["parent"]],
            "new_worker_medians_ms": [statistics.median(r["shapes"][i]["times_ms"]) for r in runs if not r["parent"]],
            "new_over_parent": new["median_ms"] / base["median_ms"],
            "parent_spread_over_median": base["spread_ms"] / base["median_ms"],
            "new_median_outside_parent_spread": bool(not (base["min_ms"] <= new["median_ms"] <= base["max_ms"])),
            "same_result": len({r["shapes"][i]["sum"] for r in runs}) == 1,
        })
    _write(a.out, {"part": "uniform", "variant": "cddpm, seeded", "rounds": a.rounds, "reps_per_worker": a.reps, "warmup": a.warmup,
                   "parent_library_hash": next(r["mi_source_hash"] for r in runs if r["parent"]),
                   "new_library_hash": next(r["mi_source_hash"] for r in runs if not r["parent"]), "shapes": shapes})


# ------------------------------------------------------------------------------ tiled and mixed: arms alternate in one process
def _drain(torch, s, tickets, t0):
    """Steps the session until it is empty -> ms from t0 to every ticket's result (host side of a synchronisation per step)."""
    done = {}
    while s.pending():
        finished = s.step()
        if finished:
            torch.cuda.synchronize()
            now = time.perf_counter()
            for t, _ in finished:
                done[t.number] = 1e3 * (now - t0)
    torch.cuda.synchronize()
    return [done[t.number] for t in tickets]


def _alternate(torch, arms, reps, warmup):
    rows = {n: [] for n in arms}
    for rep in range(warmup + reps):
        for n, fn in arms.items():                    # session, serial, session, serial, ...
            torch.cuda.synchronize()
            r = fn()
            if rep >= warmup:
                rows[n].append(r)
    return rows


def _arm_summary(rows):
    """rows: per repeat, the latency of every request in submission order"""
    return {"total": summary([max(r) for r in rows]),
            "per_request_latency": [summary([r[i] for r in rows]) for i in range(len(rows[0]))]}


def _tiled_parts(a, sizes, part):
    torch, native, den = _setup()
    from midd_amd import SamplerSession
    from midd_amd.weights import synthetic_xray
    imgs = [torch.from_numpy(synthetic_xray(1, h, w, seed=99 + i)).cuda() for i, (h, w) in enumerate(sizes)]
    session = SamplerSession(den, TILE, TILE, slots=SLOTS, seed=SEED)

    def run_session():
        t0 = time.perf_counter()
        tickets = [session.submit_tiled(x, STEPS, overlap=OVERLAP, index=i) for i, x in enumerate(imgs)]
        return _drain(torch, session, tickets, t0)

    def run_serial():
        t0, lat = time.perf_counter(), []
        for i, x in enumerate(imgs):
            den.denoise_tiled(x, inference_steps=STEPS, tile=TILE, overlap=OVERLAP, max_batch=SLOTS, seed=SEED, sample_offset=i)
            torch.cuda.synchronize()
            lat.append(1e3 * (time.perf_counter() - t0))
        return lat

    rows = _alternate(torch, {"session": run_session, "denoise_tiled": run_serial}, a.reps, a.warmup)
    session.close()
    from midd_amd import tile_plan
    tiles = [len(p.origins_y) * len(p.origins_x) for p in (tile_plan(h, w, TILE, OVERLAP) for h, w in sizes)]
    ses, ser = _arm_summary(rows["session"]), _arm_summary(rows["denoise_tiled"])
    _write(a.out, {"part": part, "images": [list(s) for s in sizes], "tiles": tiles, "tile": TILE, "overlap": OVERLAP, "slots": SLOTS,
                   "max_batch": SLOTS, "inference_steps": STEPS, "iterations": 9, "variant": "cddpm, seeded", "batch_invariant": False,
                   "compute": den.model.compute, "repeats": a.reps, "warmup": a.warmup, "mi_source_hash": native.kernel_source_hash(),
                   "device": torch.cuda.get_device_name(0), "session_submit_tiled": ses, "serial_denoise_tiled": ser,
                   "session_total_over_serial_total": ses["total"]["median_ms"] / ser["total"]["median_ms"]})


def _write(path, obj):
    text = json.dumps(obj, indent=1)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")
    print(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    u = sub.add_parser("uniform")
    u.add_argument("--parent-library", required=True)
    u.add_argument("--rounds", type=int, default=2)
    u.add_argument("--worker-timeout", type=int, default=200)
    w = sub.add_parser("worker-uniform")
    w.add_argument("--parent", action="store_true")
    td, mx = sub.add_parser("tiled"), sub.add_parser("mixed")
    for p in (u, w, td, mx):
        p.add_argument("--reps", type=int, default=5, help="timed calls per arm")
        p.add_argument("--warmup", type=int, default=1)
    for p in (u, td, mx):
        p.add_argument("--out", default=None)
    mg = sub.add_parser("merge")
    mg.add_argument("parts", nargs="+")
    a = ap.parse_args()
    if a.cmd != "merge" and a.reps < 3:
        raise SystemExit("--reps must be at least 3")
    if a.cmd == "uniform":
        part_uniform(a)
    elif a.cmd == "worker-uniform":
        worker_uniform(a)
    elif a.cmd == "tiled":
        _tiled_parts(a, [(1024, 1024)], "tiled")
    elif a.cmd == "mixed":
        _tiled_parts(a, MIXED, "mixed")
    else:
        parts = [json.load(open(p)) for p in a.parts]
        print(json.dumps({"tool": "tools/slot_tickets_ab.py", "data": "synthetic", "parts": parts}, indent=1))


if __name__ == "__main__":
    main()
