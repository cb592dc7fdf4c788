#!/usr/bin/env python3
"""Records what the stand-alone analysis entries of the C ABI refuse as JSON: tests/golden/analysis_refusals.json, which
tests/test_analysis_refusals_cpu.py replays against the built library.  CPU only: every device pointer is a fixed fake address, and every
recorded call is refused before anything is read through one or launched, so no message depends on the run.

    python tools/dump_analysis_refusals.py [OUT.json]        # default: tests/golden/analysis_refusals.json

The seven calls -- mi_ensemble_reduce, mi_ensemble_quantiles, mi_ensemble_scores, mi_ensemble_gram, mi_ensemble_project,
mi_noise_power_spectrum, mi_cross_spectrum -- each have a table of valid arguments (``base``) and the list of their rules in the order
in which the call judges them (include/midd.h), each with one change of arguments that breaks it.  Per rule two cases: the rule
broken "alone", and "with later", i.e. together with every rule after it (the call names the first of its order).  Then "further"
cases: other ways to break a rule.  Recorded per case: the return code and the whole text of ``mi_last_error()``.  The four workspace
queries are recorded as (arguments, size, and the message where the size is 0).

A float that JSON cannot spell travels as a string ("nan", "inf").  The file is a record of the commit it was generated at
(``generated_at``); it is never regenerated from code it is meant to judge.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "analysis_refusals.json")
P1, P2, P3, P4, P5, P6, P7, P8, P9 = (0x10000000 * (i + 1) for i in range(9))      # non-null "device pointers", never read
NAN, INF = "nan", "inf"
# the window of every spectrum case is a real host table whose last entry is not finite: the last rule of the two calls, so that a
# call that passed every other rule would still be refused and launch nothing
WINDOW = [0.5] * 31 + [NAN]


def load():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import midd_loader
    midd_loader.load()
    from midd_amd import native
    return native


def _ensemble(query, **more):
    return dict(query=query, query_args=("B", "members", "chw"), **more)


_SPECTRUM_OUT = dict(radial=P4, radial_count=P5, rois_used=P6, rois_skipped=P7, workspace=P8, workspace_bytes="NEED")
_SPECTRUM_RULES = [
    ("roi outside {32, 64, 128}", dict(roi=48)),
    ("step < 1", dict(step=0)),
    ("B, K or C < 1", dict(C=0)),
    ("B*C > 65535", dict(B=65536)),
    ("H < roi or W < roi", dict(H=31)),
    ("ROIs per member or chunks >= 2^31", dict(H=70000, W=70000, step=1)),
    ("detrend outside {0, 1, 2}", dict(detrend=3)),
    ("unknown flags", dict(flags=2)),
]
_SPECTRUM_FURTHER = [dict(roi=0), dict(roi=256), dict(step=-3), dict(B=0), dict(W=31), dict(H=127, roi=128), dict(detrend=-1), dict(flags=-1),
                     dict(radial=None), dict(radial_count=None), dict(rois_used=None), dict(rois_skipped=None), dict(workspace=None),
                     dict(radial_count=P5 + 2), dict(rois_skipped=P7 + 1), dict(workspace=P8 + 4), dict(workspace_bytes=0),
                     dict(rois_skipped=P6 + 8), dict(window=[0.5] * 31 + [NAN]), dict(window=[INF] + [0.5] * 31)]

ENTRIES = {
    "mi_ensemble_reduce": dict(
        params=("samples", "B", "members", "chw", "mean_out", "std_out", "stream"),
        base=dict(samples=P1, B=2, members=3, chw=100, mean_out=P2, std_out=P3, stream=None),
        rules=[("members < 1", dict(members=0)), ("B outside [1, 65535]", dict(B=0)), ("chw outside [1, 2^32)", dict(chw=0)),
               ("std_out with members < 2", dict(members=1)), ("null samples / mean_out", dict(samples=None))],
        further=[dict(members=-1), dict(B=65536), dict(chw=2 ** 32), dict(chw=-5), dict(mean_out=None)]),
    "mi_ensemble_quantiles": dict(
        params=("samples", "B", "members", "chw", "q", "nq", "out", "stream"),
        base=dict(samples=P1, B=2, members=3, chw=100, q=[0.5, 0.9], nq=2, out=P2, stream=None),
        rules=[("members < 1", dict(members=0)), ("B outside [1, 65535]", dict(B=0)), ("chw outside [1, 2^32)", dict(chw=0)),
               ("members > 64", dict(members=65)), ("nq outside [1, 8]", dict(nq=0)), ("null q", dict(q=None)),
               ("a q[i] that is NaN or outside [0, 1]", dict(q=[0.5, NAN])), ("null samples / out", dict(samples=None))],
        further=[dict(B=65536), dict(chw=2 ** 32), dict(nq=9), dict(nq=-1), dict(q=[1.5, 0.5]), dict(q=[0.0, -0.25]), dict(out=None)]),
    "mi_ensemble_scores": _ensemble(
        "mi_ensemble_scores_workspace_bytes",
        params=("samples", "truth", "B", "members", "chw", "q", "nq", "sums", "invalid", "rank_hist", "counts", "crps_map", "workspace",
                "workspace_bytes", "stream"),
        base=dict(samples=P1, truth=P2, B=2, members=3, chw=100, q=[0.1, 0.9], nq=2, sums=P3, invalid=P4, rank_hist=P5, counts=P6,
                  crps_map=P7, workspace=P8, workspace_bytes="NEED", stream=None),
        rules=[("B outside [1, 65535]", dict(B=0)), ("members outside [1, 64]", dict(members=65)), ("chw outside [1, 2^32)", dict(chw=0)),
               ("nq outside [0, 8]", dict(nq=9)), ("a level that is NaN or outside [0, 1]", dict(q=[0.1, 1.5])),
               ("a null pointer", dict(sums=None)), ("counts and nq disagreeing", dict(counts=None)),
               ("not 8-byte aligned", dict(invalid=P4 + 4)), ("not 4-byte aligned", dict(truth=P2 + 2)),
               ("workspace_bytes below the query's answer", dict(workspace_bytes="NEED-1")),
               ("an output overlapping an input or another output", dict(rank_hist=P3 + 8))],
        further=[dict(B=65536), dict(members=0), dict(chw=2 ** 32), dict(nq=-1), dict(q=[NAN, 0.5]), dict(q=None), dict(samples=None),
                 dict(truth=None), dict(invalid=None), dict(rank_hist=None), dict(workspace=None), dict(nq=0, q=None), dict(nq=0, q=None, counts=None, sums=None),
                 dict(sums=P3 + 1), dict(rank_hist=P5 + 2), dict(counts=P6 + 4), dict(workspace=P8 + 4), dict(samples=P1 + 1), dict(crps_map=P7 + 2),
                 dict(workspace_bytes=0), dict(truth=P1 + 400), dict(crps_map=P2 + 4), dict(workspace=P3 + 8), dict(counts=P5 + 8),
                 dict(crps_map=None, invalid=P3 + 56)]),
    "mi_ensemble_gram": _ensemble(
        "mi_ensemble_gram_workspace_bytes",
        params=("samples", "B", "members", "chw", "gram", "invalid", "workspace", "workspace_bytes", "stream"),
        base=dict(samples=P1, B=2, members=3, chw=100, gram=P2, invalid=P3, workspace=P4, workspace_bytes="NEED", stream=None),
        rules=[("B outside [1, 65535]", dict(B=0)), ("members outside [2, 64]", dict(members=1)), ("chw outside [1, 2^32)", dict(chw=0)),
               ("a null pointer", dict(gram=None)), ("not 8-byte aligned", dict(invalid=P3 + 4)), ("samples not 4-byte aligned", dict(samples=P1 + 2)),
               ("workspace_bytes below the query's answer", dict(workspace_bytes="NEED-1")),
               ("gram, invalid or the workspace overlapping", dict(invalid=P2 + 8))],
        further=[dict(B=65536), dict(members=65), dict(chw=2 ** 32), dict(samples=None), dict(invalid=None), dict(workspace=None), dict(gram=P2 + 1),
                 dict(workspace=P4 + 4), dict(workspace_bytes=0), dict(gram=P1 + 8), dict(workspace=P2 + 136), dict(members=12, chw=5000, workspace_bytes=8)]),
    "mi_ensemble_project": dict(
        params=("samples", "B", "members", "chw", "weights", "n_modes", "out", "stream"),
        base=dict(samples=P1, B=2, members=3, chw=100, weights=P2, n_modes=2, out=P3, stream=None),
        rules=[("B outside [1, 65535]", dict(B=0)), ("members outside [2, 64]", dict(members=65)), ("chw outside [1, 2^32)", dict(chw=0)),
               ("n_modes outside [1, 8]", dict(n_modes=9)), ("a null pointer", dict(weights=None)), ("weights not 8-byte aligned", dict(weights=P2 + 4)),
               ("samples or out not 4-byte aligned", dict(out=P3 + 2)), ("any two overlapping", dict(samples=P3 + 4))],
        further=[dict(members=1), dict(n_modes=0), dict(samples=None), dict(out=None), dict(samples=P1 + 1), dict(weights=P1 + 8), dict(out=P2 + 8), dict(out=P1 + 4)]),
    "mi_noise_power_spectrum": dict(
        query="mi_noise_power_spectrum_workspace_bytes", query_args=("B", "K", "C", "H", "W", "roi", "step"),
        params=("a", "b", "B", "K", "C", "H", "W", "roi", "step", "detrend", "window", "scale", "flags", "nps", "radial", "radial_count", "rois_used",
                "rois_skipped", "workspace", "workspace_bytes", "stream"),
        base=dict(a=P1, b=P2, B=2, K=3, C=1, H=70, W=83, roi=32, step=16, detrend=2, window=WINDOW, scale=1.0, flags=0, nps=P3, stream=None, **_SPECTRUM_OUT),
        rules=_SPECTRUM_RULES + [
            ("scale not finite", dict(scale=INF)), ("a null pointer", dict(nps=None)), ("not 8-byte aligned", dict(radial=P4 + 4)),
            ("a or b not 4-byte aligned", dict(a=P1 + 2)), ("workspace_bytes below the query's answer", dict(workspace_bytes="NEED-1")),
            ("an output overlapping an input or another output", dict(rois_used=P3 + 8)),
            ("a window entry that is not finite", dict(window=[0.5] * 30 + [NAN, INF]))],
        further=_SPECTRUM_FURTHER + [dict(K=0), dict(H=46371, W=46371, step=1, K=17, B=1),      # (ROIs per member < 2^31, chunks not)
                                     dict(scale=NAN), dict(a=None), dict(nps=P3 + 4), dict(b=P2 + 1), dict(b=None, nps=None),
                                     dict(b=P1 + 4 * 70 * 83), dict(nps=P1 + 8), dict(workspace=P2 + 8), dict(radial=P3 + 2 * 32 * 32 * 8 - 8),
                                     dict(b=None, window=[0.5] * 31 + [NAN])]),
    "mi_cross_spectrum": dict(
        query="mi_cross_spectrum_workspace_bytes", query_args=("B", "Kx", "Ky", "C", "H", "W", "roi", "step"),
        params=("x", "y", "B", "Kx", "Ky", "C", "H", "W", "roi", "step", "detrend", "window", "flags", "planes", "radial", "radial_count", "rois_used",
                "rois_skipped", "workspace", "workspace_bytes", "stream"),
        base=dict(x=P1, y=P2, B=2, Kx=3, Ky=3, C=1, H=70, W=83, roi=32, step=16, detrend=2, window=WINDOW, flags=0, planes=P3, stream=None, **_SPECTRUM_OUT),
        rules=[("Kx or Ky < 1", dict(Ky=0)), ("Kx != Ky with neither equal to 1", dict(Kx=2))] + _SPECTRUM_RULES + [
            ("a null pointer", dict(planes=None)), ("not 8-byte aligned", dict(radial=P4 + 4)), ("x or y not 4-byte aligned", dict(y=P2 + 2)),
            ("workspace_bytes below the query's answer", dict(workspace_bytes="NEED-1")),
            ("an output overlapping an input or another output", dict(rois_used=P3 + 8)),
            ("a window entry that is not finite", dict(window=[0.5] * 30 + [NAN, INF]))],
        further=_SPECTRUM_FURTHER + [dict(Kx=0), dict(H=46371, W=46371, step=1, Kx=17, Ky=1, B=1),
                                     dict(Kx=-1, Ky=1), dict(Kx=4), dict(x=None), dict(y=None), dict(planes=P3 + 4), dict(x=P1 + 2),
                                     dict(planes=P1 + 8), dict(workspace=P2 + 8), dict(radial=P3 + 4 * 2 * 32 * 32 * 8 - 8), dict(radial=P3 + 2 * 32 * 32 * 8),
                                     dict(Kx=1, planes=P1 + 2 * 70 * 83 * 4), dict(Kx=1, planes=P1 + 2 * 70 * 83 * 4 - 8), dict(Ky=1, workspace=P2 + 2 * 70 * 83 * 4 - 8),
                                     dict(y=P1, window=[0.5] * 31 + [INF]), dict(y=P1 + 4, window=[0.5] * 31 + [INF])]),
}

QUERIES = {
    "mi_ensemble_scores_workspace_bytes": [(2, 3, 100), (1, 1, 1), (1, 64, 1024), (3, 5, 1025), (65535, 64, 2 ** 32 - 1), (0, 3, 100), (65536, 3, 100),
                                           (2, 0, 100), (2, 65, 100), (2, 3, 0), (2, 3, 2 ** 32), (0, 0, 0)],
    "mi_ensemble_gram_workspace_bytes": [(2, 3, 100), (1, 2, 1), (1, 8, 4096), (1, 9, 4097), (3, 64, 10000), (0, 3, 100), (65536, 3, 100), (2, 1, 100),
                                         (2, 65, 100), (2, 3, 0), (2, 3, 2 ** 32), (0, 0, 0)],
    "mi_noise_power_spectrum_workspace_bytes": [(2, 3, 1, 70, 83, 32, 16), (1, 1, 1, 32, 32, 32, 16), (1, 4, 1, 48, 48, 32, 16), (1, 1, 1, 32, 288, 32, 16),
                                                (2, 3, 2, 70, 83, 32, 16), (1, 8, 1, 2500, 2048, 64, 32), (1, 2, 1, 128, 200, 128, 64),
                                                (0, 1, 1, 64, 64, 32, 16), (1, 0, 1, 64, 64, 32, 16), (1, 1, 1, 64, 64, 33, 16), (1, 1, 1, 64, 64, 32, 0),
                                                (1, 1, 1, 31, 64, 32, 16), (1, 1, 1, 64, 31, 32, 16), (256, 1, 256, 64, 64, 32, 16),
                                                (1, 1, 1, 70000, 70000, 32, 1), (1, 1, 1, 46371, 46371, 32, 1), (1, 17, 1, 46371, 46371, 32, 1)],
    "mi_cross_spectrum_workspace_bytes": [(2, 3, 3, 1, 70, 83, 32, 16), (1, 1, 1, 1, 32, 32, 32, 16), (1, 4, 1, 1, 48, 48, 32, 16), (1, 1, 4, 1, 48, 48, 32, 16),
                                          (1, 1, 1, 1, 32, 288, 32, 16), (2, 3, 3, 2, 70, 83, 32, 16), (1, 8, 1, 1, 2500, 2048, 64, 32),
                                          (1, 2, 2, 1, 128, 200, 128, 64), (0, 1, 1, 1, 64, 64, 32, 16), (1, 2, 3, 1, 64, 64, 32, 16),
                                          (1, 0, 1, 1, 64, 64, 32, 16), (1, 1, 0, 1, 64, 64, 32, 16), (1, 1, 1, 1, 64, 64, 33, 16), (1, 1, 1, 1, 64, 64, 32, 0),
                                          (1, 1, 1, 1, 31, 64, 32, 16), (256, 1, 1, 256, 64, 64, 32, 16), (1, 1, 1, 1, 70000, 70000, 32, 1),
                                          (1, 1, 1, 1, 46371, 46371, 32, 1), (1, 1, 17, 1, 46371, 46371, 32, 1)],
}


def cases() -> list:
    """[(entry, rule or None, "alone" | "with later" | "further", the changed arguments)]."""
    out = []
    for name, e in ENTRIES.items():
        rules = e["rules"]
        for i, (label, change) in enumerate(rules):
            out.append((name, label, "alone", dict(change)))
            later = {}
            for _, c in reversed(rules[i:]):      # (an earlier rule's change wins where two name one argument)
                later.update(c)
            out.append((name, label, "with later", later))
        out += [(name, None, "further", dict(c)) for c in e["further"]]
    return out


def _num(v):
    return float(v) if isinstance(v, str) else v


def call(native, name: str, changes: dict):
    """One call of entry `name` with its base arguments and `changes`: (rc, the whole mi_last_error text)."""
    lib, e = native.lib(), ENTRIES[name]
    a = {**e["base"], **changes}
    if isinstance(a.get("workspace_bytes"), str):      # "NEED" / "NEED-1": against the query's answer for the BASE shape
        need = getattr(lib, e["query"])(*(e["base"][k] for k in e["query_args"]))
        assert need > 0, (name, need)
        a["workspace_bytes"] = need - (a["workspace_bytes"] == "NEED-1")
    argtypes = {n: t for n, _, t in native.SYMBOLS}[name]
    args = []
    for key, ctype in zip(e["params"], argtypes):
        v = a[key]
        if ctype in (C.POINTER(C.c_double), C.POINTER(C.c_float)):
            if isinstance(v, list):
                v = (ctype._type_ * len(v))(*[_num(x) for x in v])
            elif isinstance(v, int):
                v = C.cast(v, ctype)
        args.append(_num(v))
    rc = getattr(lib, name)(*args)
    return rc, lib.mi_last_error().decode()


def query(native, name: str, args):
    """(size, the message if the size is 0 else null)."""
    lib = native.lib()
    size = getattr(lib, name)(*args)
    return size, (lib.mi_last_error().decode() if size == 0 else None)


def snapshot() -> dict:
    native = load()
    rows = []
    for name, label, how, changes in cases():
        rc, msg = call(native, name, changes)
        if rc != -1:      # MI_EINVAL: anything else got past the rules
            raise SystemExit(f"{name} {changes}: rc {rc} ({msg}): every recorded call must be refused")
        rows.append([name, label, how, changes, rc, msg])
    sizes = [[name, list(args), *query(native, name, args)] for name, table in QUERIES.items() for args in table]
    return {"cases": rows, "queries": sizes}


def _generated_at() -> str:
    def git(*a):
        return subprocess.run(("git", "-C", ROOT) + a, capture_output=True, text=True, check=True).stdout.strip()
    try:
        dirty = git("status", "--porcelain", "--", "medical-image-denoising-using-diffusion_amd")
        return git("rev-parse", "HEAD") + (" (package modified)" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main(argv) -> int:
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    snap = snapshot()
    with open(out, "w") as f:      # one line per case: a diff of the file reads as a list of what changed
        f.write('{\n "generated_at": ' + json.dumps(_generated_at()) + ',\n "cases": [\n' + ",\n".join("  " + json.dumps(r) for r in snap["cases"])
                + '\n ],\n "queries": [\n' + ",\n".join("  " + json.dumps(r) for r in snap["queries"]) + "\n ]\n}\n")
    print(f"{out}: {len(snap['cases'])} refused calls of {len(ENTRIES)} entries, {len(snap['queries'])} queries")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
