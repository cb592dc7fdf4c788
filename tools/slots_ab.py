"""Same-box measurements of the per-slot sampler loop (mi_denoise_slots, SamplerSession) -> profiles/slots_ab.json.

    uniform   cost of the slot path when nothing is ragged: run_slots with every column equal to the timestep list against
              denoise() of the PARENT commit's library (--parent-library, a build of the commit before the feature), at B = 8,
              256x256, 50 iterations and B = 1, 512x512, 9 iterations.  A library is fixed per process (MIDD_LIBRARY), so the
              arms are separate worker processes, ALTERNATED (parent new parent new); every worker warms its shapes, then
              times whole calls between synchronisations.  The parent's own run-to-run spread (its two workers, all calls) is
              recorded beside the ratio; the new library's denoise() is timed too (the refactored loop's uniform case).
    load      what the feature buys: 8 requests of 512x512, 9 iterations (the served configuration) arrive one every d ms,
              d in {0, 10, 40}; they run through a SamplerSession(slots=8) with max_rows in {None, 1, 2, 4}, and as serial
              batch-1 denoise() calls.  Throughput and per-request latency (arrival -> result on the host side of a
              synchronisation), median and worst, medians over the repeats.  Every configuration runs once untimed first.
    merge     the part files -> one JSON object on stdout.

Each part is a GPU step of its own; run them under their own time limits, chained so that nothing starts after a failure:

    timeout -k 10 600 python tools/slots_ab.py uniform --parent-library libmidd_parent.so --out out/slots_uniform.json \\
     && timeout -k 10 600 python tools/slots_ab.py load --out out/slots_load.json \\
     && python tools/slots_ab.py merge out/slots_uniform.json out/slots_load.json > profiles/slots_ab.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEED = 0x1234567890ABCDEF
UNIFORM_SHAPES = [(8, 256, 50), (1, 512, 9)]          # (B, side, iterations)
LOAD_N, LOAD_SIDE, LOAD_STEPS = 8, 512, 8             # inference_steps=8 -> 9 iterations (the server's call)


def summary(t):
    return {"median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "spread_ms": max(t) - min(t), "calls": len(t)}


def _setup(parent: bool):
    import torch
    import midd_loader
    midd_loader.load()
    from midd_amd import native
    if parent:                                        # the parent's library has every symbol but the new one
        native.SYMBOLS[:] = [s for s in native.SYMBOLS if s[0] != "mi_denoise_slots"]
    from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion
    from midd_amd.weights import make_state_dict
    if not torch.cuda.is_available():
        raise SystemExit("slots_ab.py needs a GPU")
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
        k = iters if iters == 50 else iters - 1                   # inference_steps that give `iters` iterations at noise_steps = 50
        t_list = timestep_list(50, k)
        assert len(t_list) == iters, (k, len(t_list))
        arms = {"denoise": lambda: den.denoise(x, inference_steps=k, seed=SEED)}
        if not a.parent:
            rows = [[t] * B for t in t_list]
            arms["run_slots"] = lambda: den.model.run_slots(x, x.clone(), rows, den.beta, den.alpha, den.alpha_hat, clamp_eps=False, seed=SEED)
        times = {n: [] for n in arms}
        outs = {}
        for rep in range(a.warmup + a.reps):
            for n, fn in arms.items():
                ms, o = timed(torch, fn)
                if rep >= a.warmup:
                    times[n].append(ms)
                outs[n] = o
        row = {"B": B, "side": S, "iterations": iters, "times_ms": times}
        if "run_slots" in outs:
            row["run_slots_equals_denoise"] = bool(torch.equal(outs["run_slots"], outs["denoise"]))
        out["shapes"].append(row)
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
        pool = lambda parent, arm: [t for r in runs if r["parent"] == parent for t in r["shapes"][i]["times_ms"].get(arm, [])]      # noqa: E731
        base, slots, new_denoise = summary(pool(True, "denoise")), summary(pool(False, "run_slots")), summary(pool(False, "denoise"))
        per_worker = [statistics.median(r["shapes"][i]["times_ms"]["denoise"]) for r in runs if r["parent"]]
        shapes.append({
            "B": B, "side": S, "iterations": iters,
            "parent_denoise": base, "new_run_slots_uniform": slots, "new_denoise": new_denoise,
            "parent_worker_medians_ms": per_worker,
            "run_slots_over_parent_denoise": slots["median_ms"] / base["median_ms"],
            "new_denoise_over_parent_denoise": new_denoise["median_ms"] / base["median_ms"],
            "parent_spread_over_median": base["spread_ms"] / base["median_ms"],
            "run_slots_outside_parent_spread": bool(not (base["min_ms"] <= slots["median_ms"] <= base["max_ms"])),
            "new_denoise_outside_parent_spread": bool(not (base["min_ms"] <= new_denoise["median_ms"] <= base["max_ms"])),
            "run_slots_equals_denoise_bitwise": all(r["shapes"][i].get("run_slots_equals_denoise", True) for r in runs if not r["parent"]),
        })
    res = {"part": "uniform", "variant": "cddpm, seeded", "rounds": a.rounds, "reps_per_worker": a.reps, "warmup": a.warmup,
           "parent_library_hash": next(r["mi_source_hash"] for r in runs if r["parent"]),
           "new_library_hash": next(r["mi_source_hash"] for r in runs if not r["parent"]), "shapes": shapes}
    _write(a.out, res)


# ------------------------------------------------------------------------------ load: arrivals every d ms
def _arrivals(n, d_ms, submit):
    """Calls submit(i) at t0 + i * d from a thread of its own -> (thread, list of arrival times)."""
    times = [None] * n
    t0 = time.perf_counter()

    def run():
        for i in range(n):
            wait = t0 + i * d_ms * 1e-3 - time.perf_counter()
            if wait > 0:
                time.sleep(wait)
            times[i] = time.perf_counter()
            submit(i)
    th = threading.Thread(target=run)
    th.start()
    return th, times


def part_load(a):
    torch, native, den = _setup(False)
    from midd_amd import SamplerSession
    from midd_amd.weights import synthetic_xray
    imgs = torch.from_numpy(synthetic_xray(LOAD_N, LOAD_SIDE, LOAD_SIDE, seed=99)).cuda()

    def run_session(d_ms, max_rows):
        s = SamplerSession(den, LOAD_SIDE, LOAD_SIDE, slots=LOAD_N, seed=SEED, max_rows=max_rows)
        tickets, done, calls = [None] * LOAD_N, {}, 0
        th, arrive = _arrivals(LOAD_N, d_ms, lambda i: tickets.__setitem__(i, s.submit(imgs[i:i + 1], LOAD_STEPS, index=i)))
        while len(done) < LOAD_N:
            if s.pending():
                finished = s.step()
                calls += 1
                torch.cuda.synchronize()
                now = time.perf_counter()
                for t, _ in finished:
                    done[t.index] = now
            else:
                time.sleep(0.0002)
        th.join()
        s.close()
        return arrive, [done[i] for i in range(LOAD_N)], calls

    def run_serial(d_ms):
        queue, done = [], {}
        lock = threading.Lock()

        def submit(i):
            with lock:
                queue.append(i)
        th, arrive = _arrivals(LOAD_N, d_ms, submit)
        while len(done) < LOAD_N:
            with lock:
                i = queue.pop(0) if queue else None
            if i is None:
                time.sleep(0.0002)
                continue
            den.denoise(imgs[i:i + 1], inference_steps=LOAD_STEPS, seed=SEED, sample_offset=i)
            torch.cuda.synchronize()
            done[i] = time.perf_counter()
        th.join()
        return arrive, [done[i] for i in range(LOAD_N)], LOAD_N

    def measure(fn):
        fn()                                          # untimed: plans, workspaces and code objects of every batch it meets
        thr, med, worst, calls = [], [], [], []
        for _ in range(a.reps):
            arrive, done, n_calls = fn()
            lat = [1e3 * (d - t) for d, t in zip(done, arrive)]
            thr.append(LOAD_N / (max(done) - min(arrive)))
            med.append(statistics.median(lat)); worst.append(max(lat)); calls.append(n_calls)
        return {"images_per_s": {"median": statistics.median(thr), "min": min(thr), "max": max(thr)},
                "latency_ms_median": {"median": statistics.median(med), "min": min(med), "max": max(med)},
                "latency_ms_worst": {"median": statistics.median(worst), "min": min(worst), "max": max(worst)},
                "native_calls": statistics.median(calls), "repeats": a.reps}

    rows = []
    for d in (0, 10, 40):
        row = {"arrival_interval_ms": d, "serial_batch1_denoise": measure(lambda: run_serial(d))}
        for mr in (None, 1, 2, 4):
            row[f"session_slots8_max_rows_{mr}"] = measure(lambda: run_session(d, mr))
        rows.append(row)
    _write(a.out, {"part": "load", "requests": LOAD_N, "image": [LOAD_SIDE, LOAD_SIDE], "inference_steps": LOAD_STEPS, "iterations": 9,
                   "variant": "cddpm, seeded", "batch_invariant": False, "compute": den.model.compute,
                   "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0), "rows": rows})


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
    u.add_argument("--worker-timeout", type=int, default=280)
    w = sub.add_parser("worker-uniform")
    w.add_argument("--parent", action="store_true")
    ld = sub.add_parser("load")
    for p in (u, w, ld):
        p.add_argument("--reps", type=int, default=5, help="timed calls per arm (>= 5)")
        p.add_argument("--warmup", type=int, default=2)
    for p in (u, ld):
        p.add_argument("--out", default=None)
    mg = sub.add_parser("merge")
    mg.add_argument("parts", nargs="+")
    a = ap.parse_args()
    if a.cmd != "merge" and a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if a.cmd == "uniform":
        part_uniform(a)
    elif a.cmd == "worker-uniform":
        worker_uniform(a)
    elif a.cmd == "load":
        part_load(a)
    else:
        parts = [json.load(open(p)) for p in a.parts]
        print(json.dumps({"tool": "tools/slots_ab.py", "data": "synthetic", "parts": parts}, indent=1))


if __name__ == "__main__":
    main()
