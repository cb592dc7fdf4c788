"""Host-only: the planner against the oracle over a grid of constructor arguments, the inventory of the topologies whose
ConvTranspose is materialised (conv_transpose_kernel + chan_total_kernel: tests/topology_cases.py), the float64 walker the GPU
tests of those topologies judge against, and the a-priori fp32 bound of a ConvTranspose.  Through tools/plan_dump.py; no GPU."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plan_dump as pd

from midd_amd import native
from midd_amd.config import UNetConfig, topology
from oracle import ddim_oracle as orc
from tests import topology_cases as tc
from tests.test_gpu_parity import CONFIG_SWEEP

CONVT, CHAN_TOT = "midd::conv_transpose_kernel", "midd::chan_total_kernel"
COMPUTE_MODES = ("f16x3", "f32")

# planner refusals by message family -> how the oracle fails on the same configuration
REFUSALS = {
    "skip": (re.compile(r"skip stack (underflow|empty)"), "IndexError"),                   # a residual block pops an empty stack
    "channels": (re.compile(r"expected \d+ input channels, graph provides \d+"), "RuntimeError"),
    "size": (re.compile(r"network output is \d+x\d+ for a \d+x\d+ input"), "shape"),
}
HEAD_DIM = re.compile(r"attention head_dim \d+ unsupported \(32/64/96/128\)")               # the one documented limit of the planner


def plan_text(variant, kw, B, H, W, compute="f16x3"):
    """-> (dump text, None) or (None, refusal message)"""
    try:
        plan = pd.make_plan(kw, compute, variant)
    except native.MiddError as e:
        return None, str(e)
    try:
        return pd.dump(plan, B, H, W, 0), None
    except native.MiddError as e:
        return None, str(e)
    finally:
        native.lib().mi_plan_destroy(plan)


def oracle_outcome(variant, kw, H=16, W=16):
    """'ok' when the oracle's forward runs and returns an input-sized output; else how it fails"""
    x = torch.zeros(1, 1, H, W)
    try:
        cfg = UNetConfig(variant=variant, **kw)
        topo = topology(cfg)                 # (the cddpm constructor itself pops the skip widths)
        with torch.no_grad():
            y = orc.unet_forward(tc.zero_state_dict(cfg), topo, x, x, torch.zeros(1, dtype=torch.long))
    except (IndexError, RuntimeError) as e:
        return type(e).__name__
    return "ok" if y.shape == x.shape else "shape"


@pytest.fixture(scope="module")
def sweep():
    """[(variant, kw, {compute: dump text} or None, refusal message, oracle outcome)] over the grid at 16x16, B = 1"""
    rows = []
    for variant, kw in tc.grid():
        text, msg = plan_text(variant, kw, 1, 16, 16)
        texts = None
        if text is not None:
            t32, m32 = plan_text(variant, kw, 1, 16, 16, "f32")
            assert m32 is None, (variant, kw, m32)          # what one compute mode plans, the other plans
            texts = {"f16x3": text, "f32": t32}
        rows.append((variant, kw, texts, msg, oracle_outcome(variant, kw)))
    return rows


def test_planner_accepts_what_the_oracle_runs(sweep):
    """The planner accepts a configuration if and only if the oracle's forward runs and returns an input-sized output; the sole
    exception is the head_dim limit.  Every refusal is of a known family, and the oracle fails the same way."""
    accepted, head_dim, families = 0, 0, {k: 0 for k in REFUSALS}
    for variant, kw, texts, msg, outcome in sweep:
        if texts is not None:
            accepted += 1
            assert outcome == "ok", (variant, kw, outcome)
        elif HEAD_DIM.search(msg):
            head_dim += 1                                   # (the oracle may run these: no claim either way)
        else:
            fam = [k for k, (rx, _) in REFUSALS.items() if rx.search(msg)]
            assert len(fam) == 1, (variant, kw, msg)
            families[fam[0]] += 1
            assert outcome == REFUSALS[fam[0]][1], (variant, kw, msg, outcome)
    print(f"grid {len(sweep)}: accepted {accepted}, head_dim {head_dim}, refused {families}")
    assert accepted > 200 and all(families.values()) and head_dim


def _has(text, kernel):
    return kernel in tc.kernels(text)


def test_unfolded_cases_reach_the_two_kernels():
    """Every UNFOLDED_CASES entry materialises a ConvTranspose and totals it with chan_total_kernel, in both compute modes, once per
    module tests/topology_cases.py::materialised_ups names (which the GPU tests rely on)."""
    for cid, (variant, kw, B, H, W) in tc.UNFOLDED_CASES.items():
        ups = tc.materialised_ups(topology(UNetConfig(variant=variant, **kw)), H, W)
        assert ups, cid
        for compute in COMPUTE_MODES:
            text, msg = plan_text(variant, kw, B, H, W, compute)
            assert msg is None, (cid, msg)
            lines = text.splitlines()
            assert sum(CONVT in l for l in lines) == len(ups) and sum(CHAN_TOT in l for l in lines) == len(ups), (cid, compute)
            for a, b in zip(lines, lines[1:]):              # chan_total follows each ConvTranspose
                assert (CONVT in a) == (CHAN_TOT in b), (cid, compute, a, b)


def test_last_level_attention_alone_never_unfolds(sweep):
    """What CONFIG_SWEEP (tests/test_gpu_parity.py) relies on: with attention at the last level only the fold always applies."""
    seen = 0
    for variant, kw, texts, msg, outcome in sweep:
        if texts is None or kw["attention_resolutions"] != (len(kw["channel_mult"]) - 1,):
            continue
        seen += 1
        for text in texts.values():
            assert not _has(text, CONVT) and not _has(text, CHAN_TOT), (variant, kw)
    assert seen >= 20
    for kw, variant, B, H, W in CONFIG_SWEEP:
        text, msg = plan_text(variant, kw, B, H, W)
        assert msg is None and not _has(text, CONVT) and not _has(text, CHAN_TOT), kw
    unfolded = sum(_has(texts["f16x3"], CONVT) for _, _, texts, _, _ in sweep if texts)
    print(f"{unfolded} accepted grid configurations launch {CONVT}")
    assert unfolded > 100


def test_every_op_kind_of_the_grid_is_reached_by_a_listed_case(sweep):
    """An op kind (tests/topology_cases.py::op_signatures) that some accepted grid configuration reaches and neither UNFOLDED_CASES
    nor CONFIG_SWEEP does has no GPU test: a planner change that opens such a path fails here."""
    listed = [(v, kw, B, H, W) for v, kw, B, H, W in tc.UNFOLDED_CASES.values()] + [(v, kw, B, H, W) for kw, v, B, H, W in CONFIG_SWEEP]
    covered = set()
    for variant, kw, B, H, W in listed:
        for compute in COMPUTE_MODES:
            text, msg = plan_text(variant, kw, B, H, W, compute)
            assert msg is None, (kw, msg)
            covered |= {f"{compute} {s}" for s in tc.op_signatures(text)}
    reached = set()
    for variant, kw, texts, msg, outcome in sweep:
        for compute, text in (texts or {}).items():
            reached |= {f"{compute} {s}" for s in tc.op_signatures(text)}
    assert any("convT" in s for s in reached) and any("chan_tot" in s for s in reached)
    assert reached <= covered, sorted(reached - covered)


# ------------------------------------------------------------------------------ chan_total's LDS
def test_unfolded_convtranspose_of_1024_channels_is_refused_by_name():
    """chan_total_kernel asks for ppi * C * 16 + (C + 2) * 48 bytes of dynamic LDS and does not raise its 64 KB limit: 1024 channels
    take 65632 bytes.  The planner refuses the topology with the figures; 512 channels (33 KB) plan."""
    def kw(mult):
        return dict(model_channels=128, channel_mult=mult, num_res_blocks=1, attention_resolutions=(0,), time_emb_dim=32)
    text, msg = plan_text("cddpm", kw((1, 8, 2)), 1, 16, 16)
    assert text is None and re.search(r"ups\.\d+: an unfolded ConvTranspose of 1024 channels: chan_total needs 65632 bytes of LDS .* limit is 65536", msg), msg
    for compute in COMPUTE_MODES:
        text, msg = plan_text("cddpm", kw((1, 4, 2)), 1, 16, 16, compute)
        assert msg is None and any(CONVT in l and "c512+0->512" in l for l in text.splitlines()), msg
    # the same widths folded (attention at the last level only) never needed chan_total: still planned
    folded = dict(kw((1, 8, 2)), attention_resolutions=(2,))
    text, msg = plan_text("cddpm", folded, 1, 16, 16)
    assert msg is None and not _has(text, CHAN_TOT), msg


# ------------------------------------------------------------------------------ the float64 walker
@pytest.mark.parametrize("cid", sorted(tc.UNFOLDED_CASES))
def test_float64_walker_equals_the_oracle_and_isolates(cid):
    cfg, topo, sd, x, cond, t = tc.case_inputs(cid)
    trace = {}
    with torch.no_grad():
        eps = orc.unet_forward(sd, topo, x, cond, t, trace=lambda n, v: trace.__setitem__(n, v))
        w64 = tc.walk(tc.cast_state_dict(sd, torch.float64), topo, x, cond, t)
        w32 = tc.walk(sd, topo, x, cond, t, dtype=torch.float32)
    assert set(w64) == set(trace) and all(v.dtype == torch.float64 for v in w64.values())
    # in float32 the walker IS the oracle
    assert torch.equal(w32["out_conv"], eps) and all(torch.equal(w32[n], trace[n]) for n in trace)
    # chained in float64: the oracle's own rounding (fp32, a few hundred terms per output, ~70 layers deep)
    worst = {n: float((trace[n].double() - w64[n]).abs().max() / max(1.0, float(w64[n].abs().max()))) for n in trace}
    top = max(worst, key=worst.get)
    print(f"case {cid}: fp32 oracle vs float64 walker, worst layer {top} {worst[top]:.2e} (relative to max(1, max|layer|))")
    assert worst[top] < 1e-5, top
    # isolated on its own chained outputs it reproduces them exactly
    with torch.no_grad():
        iso = tc.walk(tc.cast_state_dict(sd, torch.float64), topo, x, cond, t, given=dict(w64))
    assert all(torch.equal(iso[n], w64[n]) for n in w64)
    # ... and a perturbed input of one module moves that module's consumers only
    up, pred, consumer = tc.materialised_ups(topo, x.shape[2], x.shape[3])[0]
    with torch.no_grad():
        moved = tc.walk(tc.cast_state_dict(sd, torch.float64), topo, x, cond, t, given={**w64, pred: w64[pred] + 1.0})
    changed = {n for n in w64 if not torch.equal(moved[n], w64[n])}
    assert up in changed and consumer not in changed and changed <= {m.name for m in topo.ups}, changed
    assert tc.rb_inputs(topo, consumer)[0] == up


@pytest.mark.parametrize("cin", [64, 128, 192])
def test_convtranspose_fp32_bound_holds_for_torch(cin):
    """|y32 - y64| <= (n + 1) 2^-24 (|x| * |w| + |b|), n = 4 Cin + 1, per element, for torch's own fp32 ConvTranspose2d: the gate
    the GPU kernel is held to (tests/test_gpu_unfolded_topologies.py) is one any correct fp32 evaluation meets with a wide margin,
    while a structural error (a wrong tap) moves an output by about its own magnitude, some 1e4 bounds."""
    g = torch.Generator().manual_seed(cin)
    x = torch.randn(2, cin, 5, 7, generator=g)                       # odd map: border taps on every side
    w = torch.randn(cin, cin, 4, 4, generator=g) / (4 * cin) ** 0.5
    b = torch.randn(cin, generator=g)
    y32 = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    y64 = F.conv_transpose2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    bound = tc.conv_transpose_bound(x, w, b)
    used = float(((y32.double() - y64).abs() / bound).max())
    print(f"Cin {cin}: torch fp32 uses {100 * used:.2f} % of the bound; bound / max|y| = {float(bound.max() / y64.abs().max()):.1e}")
    assert used <= 1.0
    # a wrong tap parity is far outside it: the kernel flipped in x
    wrong = F.conv_transpose2d(x.double(), w.double().flip(3), b.double(), stride=2, padding=1)
    assert float(((wrong - y64).abs() / bound).max()) > 100
