"""Time of the slot path under an update rule (mi_denoise_slots_rule) next to the uniform calls of the same build, in one process:

  pair 1, per rule ("ddim" at eta = 0, "dpmpp2m"):
    denoise(x, K, update=rule)                              (the base: out_conv_ddim_kernel / out_conv_dpm_kernel)
    run_slots_rule(x, x.clone(), uniform table, rule)       (out_conv_slots_rule_kernel: the same programs, every scalar of the
                                                             update from the slot's 64-byte record, one small fill launch per row)
  at B = 8, 256 x 256, 50 of 50 timesteps and at B = 1, 512 x 512, 9 of 50 (the served list);
  pair 2, per rule: a 16-slot SamplerSession(rule=) at 256 x 256 fed 12 plain tickets (9-entry lists) and one tiled 512 x 384
    ticket, drained, against the same tickets as serial denoise / denoise_tiled calls.

Full-width DDIM-variant network, random-init weights.  The arms of a pair are interleaved so that clock drift hits both alike;
median [min - max] of at least 5 timed runs per arm after the warm-ups is reported, never a single run, and the ratio of the medians
stands next to the base arm's own spread.  A profiled call of each arm of pair 1 gives the out-conv kernels' own time per launch.

    python tools/slots_rule_ab.py [--reps 5] [--warmup 2] > profiles/slots_rule_ab.json

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
from midd_amd import DiffusionDenoiser, SamplerRule, SamplerSession, UNetConfig, UNetDiffusion, native, timestep_list  # noqa: E402
from midd_amd.weights import make_state_dict, synthetic_xray  # noqa: E402

NOISE_STEPS = 50
RULES = {"ddim": SamplerRule("ddim"), "dpmpp2m": SamplerRule("dpmpp2m")}


def timed(arms, reps, warmup):
    """arms: name -> callable.  -> name -> ms of every timed run, the arms interleaved."""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = {name: [] for name in arms}
    for rep in range(warmup + reps):
        for name, fn in arms.items():
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            if rep >= warmup:
                per[name].append(ev[0].elapsed_time(ev[1]))
    return per


def stats(t):
    return {"median": statistics.median(t), "min": min(t), "max": max(t)}


def pair_row(per, base, other):
    b, o = stats(per[base]), stats(per[other])
    return {base: {"ms": b}, other: {"ms": o}, other + "_over_" + base + "_time": o["median"] / b["median"],
            base + "_spread": (b["max"] - b["min"]) / b["median"]}


def out_conv_time(model, fn):
    model.profile_begin()
    fn()
    torch.cuda.synchronize()
    return {e["name"]: {"us_per_launch": 1e3 * e["total_ms"] / e["launches"], "launches": e["launches"]}
            for e in model.profile_end() if "out_conv" in e["name"] or "slot" in e["name"]}


def uniform_pair(den, rule, B, size, K, reps, warmup):
    x = torch.from_numpy(synthetic_xray(B, size, size, seed=77)).cuda()
    t_list = timestep_list(NOISE_STEPS, K)
    rows = [[t] * B for t in t_list]
    x0 = torch.empty_like(x) if rule.update == "dpmpp2m" else None

    def uniform():
        return den.denoise(x, K, **rule.kwargs())

    def slots():
        return den.model.run_slots_rule(x, x.clone(), rows, den.beta, den.alpha, den.alpha_hat, clamp_eps=True, rule=rule, x0=x0)

    same = bool(torch.equal(uniform(), slots()))
    row = {"rule": rule.update, "shape": [B, 1, size, size], "iterations": len(t_list), "same_bits": same}
    row.update(pair_row(timed({"denoise": uniform, "run_slots_rule": slots}, reps, warmup), "denoise", "run_slots_rule"))
    row["kernels"] = {"denoise": out_conv_time(den.model, uniform), "run_slots_rule": out_conv_time(den.model, slots)}
    return row


def session_pair(den, rule, reps, warmup):
    plain = torch.from_numpy(synthetic_xray(12, 256, 256, seed=5)).cuda()
    big = torch.from_numpy(synthetic_xray(1, 512, 384, seed=6)).cuda()

    def session():
        with SamplerSession(den, 256, 256, slots=16, rule=rule) as s:
            tickets = [s.submit(plain[i:i + 1], 8) for i in range(12)] + [s.submit_tiled(big, 8, overlap=32)]
            s.drain()
            return [t.result() for t in tickets]

    def serial():
        return [den.denoise(plain[i:i + 1], 8, **rule.kwargs()) for i in range(12)] + \
               [den.denoise_tiled(big, 8, tile=256, overlap=32, **rule.kwargs()).image]

    row = {"rule": rule.update, "tickets": "12 x [1,1,256,256] + one tiled [1,1,512,384] (tile 256, overlap 32), 9 of 50 timesteps", "slots": 16}
    row.update(pair_row(timed({"serial_calls": serial, "session": session}, reps, warmup), "serial_calls", "session"))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="timed runs per arm (>= 5)")
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.reps < 5:
        raise SystemExit("--reps must be at least 5")
    if not torch.cuda.is_available():
        raise SystemExit("slots_rule_ab.py needs a GPU")
    model = UNetDiffusion()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(UNetConfig(), seed=42).items()})
    den = DiffusionDenoiser(model.to("cuda").eval(), noise_steps=NOISE_STEPS)
    uniform = [uniform_pair(den, rule, B, size, K, a.reps, a.warmup) for rule in RULES.values() for B, size, K in ((8, 256, 50), (1, 512, 8))]
    sessions = [session_pair(den, rule, a.reps, a.warmup) for rule in RULES.values()]
    print(json.dumps({
        "tool": "tools/slots_rule_ab.py",
        "metric": "wall time (events around the run) of run_slots_rule on a uniform table beside denoise(update=...), and of a 16-slot "
                  "rule session beside the same tickets as serial calls; arms interleaved in one process; and the out-conv / record-fill "
                  "kernels' own time per launch from a profiled call of each arm",
        "mi_source_hash": native.kernel_source_hash(), "device": torch.cuda.get_device_name(0),
        "reps": a.reps, "warmup": a.warmup, "weights": "random-init (make_state_dict seed 42)",
        "uniform_table": uniform, "session": sessions}))


if __name__ == "__main__":
    main()
