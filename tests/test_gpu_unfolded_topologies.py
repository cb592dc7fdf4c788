"""The topologies whose ConvTranspose the planner materialises (tests/topology_cases.py: UNFOLDED_CASES) on the GPU, through the C
ABI: conv_transpose_kernel (csrc/resample.hip), chan_total_kernel (csrc/groupnorm.hip), the planner branch that selects them, the
GroupNorm consumer reading their totals beside a skip's, and attention blocks at levels other than the last.

Gates: the project's stated tolerances (tests/test_gpu_parity.py) with layer errors relative to max(1, max|layer|); for the
ConvTranspose alone the a-priori fp32 bound of tests/topology_cases.py::conv_transpose_bound.  Every test prints what it gated on.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from midd_amd import UNetDiffusion, DiffusionDenoiser, timestep_list
from midd_amd import native
from oracle import ddim_oracle as orc
from tests import topology_cases as tc
from tests.test_gpu_parity import COMPUTE_MODES, TOL_EPS, TOL_FINAL, TOL_LAYER

pytestmark = pytest.mark.gpu

CASES = sorted(tc.UNFOLDED_CASES)


def _model(cid, sd, compute):
    variant, kw, _, _, _ = tc.UNFOLDED_CASES[cid]
    m = UNetDiffusion(variant=variant, compute=compute, **kw)
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    return m.to("cuda").eval()


def _rel(got, want):
    """max|got - want| relative to max(1, max|want|), in float64"""
    want = want.double()
    return float((got.double() - want).abs().max() / max(1.0, float(want.abs().max())))


def _fetch_all(model, topo, x):
    """{name: device output (CPU tensor)} of every module the device materialises; a folded ConvTranspose has none"""
    B, _, H, W = x.shape
    out = {}
    for name, kind in [("in_conv", "in")] + [(m.name, m.kind) for m in topo.downs + topo.mid + topo.ups]:
        try:
            out[name] = model.debug_fetch(name, B, H, W).cpu()
        except native.MiddError:
            assert kind == "up", name
    return out


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The case's inputs, the fp32 oracle's trace and the float64 chained walk: computed once, shared, never written to"""
    cfg, topo, sd, x, cond, t = tc.case_inputs(cid)
    trace = {}
    with torch.no_grad():
        orc.unet_forward(sd, topo, x, cond, t, trace=lambda n, v: trace.__setitem__(n, v))
        w64 = tc.walk(tc.cast_state_dict(sd, torch.float64), topo, x, cond, t)
    return cfg, topo, sd, x, cond, t, trace, w64


@functools.lru_cache(maxsize=None)
def device_run(cid, compute):
    """One forward of the case on the device: (model, eps, {name: output}) as CPU tensors"""
    cfg, topo, sd, x, cond, t, _, _ = reference(cid)
    model = _model(cid, sd, compute)
    eps = model(x.cuda(), cond.cuda(), t.cuda()).cpu()
    return model, eps, _fetch_all(model, topo, x)


# ------------------------------------------------------------------------------ a. forward, per layer
@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("cid", CASES)
def test_forward_per_layer_vs_oracle(cid, compute):
    cfg, topo, sd, x, cond, t, trace, _ = reference(cid)
    model, eps, dev = device_run(cid, compute)
    B, _, H, W = x.shape
    ups = tc.materialised_ups(topo, H, W)
    assert ups
    for up, pred, _ in ups:                      # materialised: fetchable, at the doubled size
        assert up in dev, f"{up} has no materialised output"
        assert dev[up].shape == (B, dev[pred].shape[1], 2 * dev[pred].shape[2], 2 * dev[pred].shape[3]), (up, dev[up].shape)
    worst = {}
    for name, want in trace.items():
        if name in ("time_mlp", "out_conv"):
            continue
        if name not in dev:
            assert any(m.name == name and m.kind == "up" for m in topo.ups) and name not in [u for u, _, _ in ups], name
            continue
        assert dev[name].shape == want.shape, name
        worst[name] = _rel(dev[name], want)
    d_eps = _rel(eps, trace["out_conv"])
    print(f"case {cid} {compute}: eps {d_eps:.2e}; layers " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    assert torch.isfinite(eps).all()
    assert max(worst.values()) < TOL_LAYER, max(worst, key=worst.get)
    assert d_eps < TOL_EPS


# ------------------------------------------------------------------------------ b. the ConvTranspose kernel alone
@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("cid", CASES)
def test_conv_transpose_alone_within_the_fp32_bound(cid, compute):
    """conv_transpose_kernel on the device's own input against float64, element by element (every batch row, corners and edges
    included) under the a-priori bound; the ratio to torch's fp32 error on the same input is printed, not gated (the kernel sums
    its 4 Cin products sequentially, torch does not)."""
    cfg, topo, sd, x, cond, t, _, _ = reference(cid)
    _, _, dev = device_run(cid, compute)
    for up, pred, _ in tc.materialised_ups(topo, x.shape[2], x.shape[3]):
        xin, w, b = dev[pred], sd[f"{up}.weight"], sd[f"{up}.bias"]
        y64 = F.conv_transpose2d(xin.double(), w.double(), b.double(), stride=2, padding=1)
        y32 = F.conv_transpose2d(xin, w, b, stride=2, padding=1)
        bound = tc.conv_transpose_bound(xin, w, b)
        err = (dev[up].double() - y64).abs()
        err32 = (y32.double() - y64).abs()
        used = float((err / bound).max())
        print(f"case {cid} {compute} {up} Cin {xin.shape[1]} {tuple(xin.shape[2:])}->{tuple(y64.shape[2:])}: max|d| {float(err.max()):.2e}, "
              f"{100 * used:.2f} % of the bound (torch fp32: {100 * float((err32 / bound).max()):.2f} %), "
              f"device / torch fp32 max error = {float(err.max() / err32.max()):.2f}")
        assert dev[up].shape == y64.shape
        assert bool((err <= bound).all()), (up, np.unravel_index(int((err / bound).argmax()), err.shape), used)


# ------------------------------------------------------------------------------ c. the statistics path under cancellation
@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("cid", ["A", "B"])
def test_group_norm_totals_under_cancellation(cid, compute):
    """100 std(output) added to every ConvTranspose bias: the consumer's GroupNorm takes E[x^2] - mean^2 from chan_total_kernel's
    totals at |mean| / std of 100 (A) and some tens (B).  Every layer and eps against the float64 chained walk."""
    cfg, topo, sd, x, cond, t, _, base64 = reference(cid)
    sd = dict(sd)
    for m in topo.ups:
        if m.kind == "up":
            sd[f"{m.name}.bias"] = (sd[f"{m.name}.bias"].double() + 100.0 * float(base64[m.name].std())).float()
    trace = {}
    with torch.no_grad():
        orc.unet_forward(sd, topo, x, cond, t, trace=lambda n, v: trace.__setitem__(n, v))
        w64 = tc.walk(tc.cast_state_dict(sd, torch.float64), topo, x, cond, t)
    last = tc.materialised_ups(topo, x.shape[2], x.shape[3])[-1][0]
    ratio = float(w64[last].mean().abs() / w64[last].std())
    own = max(_rel(trace[n], w64[n]) for n in trace)
    print(f"case {cid} {compute}: |mean| / std at {last} = {ratio:.1f}; fp32 oracle vs float64, worst layer {own:.2e}")
    assert ratio > 20                            # the input does what it is for
    assert own < TOL_EPS / 20                    # ... and is not itself hard for fp32
    model = _model(cid, sd, compute)
    eps = model(x.cuda(), cond.cuda(), t.cuda()).cpu()
    dev = _fetch_all(model, topo, x)
    worst = {n: _rel(v, w64[n]) for n, v in dev.items()}
    d_eps = _rel(eps, w64["out_conv"])
    print(f"case {cid} {compute} shifted: eps {d_eps:.2e}; layers " + " ".join(f"{k}={v:.1e}" for k, v in worst.items()))
    assert max(worst.values()) < TOL_EPS, max(worst, key=worst.get)
    assert d_eps < TOL_EPS


# ------------------------------------------------------------------------------ d. the consumer alone
@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("cid", ["A", "E"])
def test_consumer_block_alone_on_the_device_inputs(cid, compute):
    """The residual block after each materialised ConvTranspose: the float64 block on the device's own inputs (the ConvTranspose
    output whose totals chan_total_kernel left, and the skip) against the device's output.  The ratio to the fp32 oracle's error
    on the same inputs is printed (DESIGN.md records it)."""
    cfg, topo, sd, x, cond, t, _, _ = reference(cid)
    _, _, dev = device_run(cid, compute)
    with torch.no_grad():
        iso64 = tc.walk(tc.cast_state_dict(sd, torch.float64), topo, x, cond, t, given=dev)
        iso32 = tc.walk(sd, topo, x, cond, t, given=dev, dtype=torch.float32)
    for up, _, consumer in tc.materialised_ups(topo, x.shape[2], x.shape[3]):
        assert tc.rb_inputs(topo, consumer)[0] == up
        d, d32 = _rel(dev[consumer], iso64[consumer]), _rel(iso32[consumer], iso64[consumer])
        print(f"case {cid} {compute} {consumer} after {up}: device {d:.2e}, fp32 oracle {d32:.2e} on the same inputs, ratio {d / d32:.1f}")
        assert d < TOL_LAYER, consumer


# ------------------------------------------------------------------------------ e. bits
@pytest.mark.parametrize("compute", COMPUTE_MODES)
def test_case_a_bits(compute):
    """Nothing reads scratch the call did not write and the totals arena is cleared (the same bits under every workspace fill);
    a sample alone equals its row of the batch; two consecutive calls are equal."""
    cfg, topo, sd, x, cond, t, _, _ = reference("A")
    model = _model("A", sd, compute)
    xc, cc, tc_ = x.cuda(), cond.cuda(), t.cuda()
    B, _, H, W = x.shape
    (up, _, consumer), = tc.materialised_ups(topo, H, W)
    runs = []
    for pattern in (255, 0, 127, None):
        model.poison_workspace = pattern
        eps = model(xc, cc, tc_)
        runs.append((eps.cpu(), model.debug_fetch(up, B, H, W).cpu(), model.debug_fetch(consumer, B, H, W).cpu()))
        assert all(torch.isfinite(v).all() for v in runs[-1]), pattern
        assert all(torch.equal(a, b) for a, b in zip(runs[0], runs[-1])), pattern
    model.poison_workspace = 255
    again = model(xc, cc, tc_).cpu()
    assert torch.equal(again, runs[0][0]), "two consecutive calls differ"
    for i in range(B):
        one = model(xc[i:i + 1], cc[i:i + 1], tc_[i:i + 1]).cpu()
        d = float((one[0] - runs[0][0][i]).abs().max())
        print(f"case A {compute}: sample {i} alone vs its batch row: max|d| = {d:.1e}")
        assert torch.equal(one[0], runs[0][0][i]), i


# ------------------------------------------------------------------------------ f. sampler
@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("cid,B", [("A", 4), ("C", 2)])
def test_sampler_vs_oracle(cid, B, compute):
    """DiffusionDenoiser.denoise, 3 inference steps: case A at B = 4 runs as two side-by-side programs of 2 on two streams (cddpm,
    explicit step noise); case C at B = 2 (deterministic)."""
    cfg, topo, sd, _, _, _, _, _ = reference(cid)
    variant, _, _, H, W = tc.UNFOLDED_CASES[cid]
    model = _model(cid, sd, compute)
    noisy = torch.from_numpy(tc.synthetic_xray(B, H, W, seed=900 + B))
    steps = timestep_list(50, 3)
    kw, okw = {}, {}
    if variant == "cddpm":
        g = np.random.Generator(np.random.Philox(key=17))
        noise = torch.from_numpy(np.stack([0.5 * g.standard_normal((B, 1, H, W), dtype=np.float32) for _ in steps]))
        kw["step_noise"], okw["step_noise"] = noise.cuda(), list(noise)
    out = DiffusionDenoiser(model, noise_steps=50).denoise(noisy.cuda(), inference_steps=3, **kw).cpu()
    want = orc.denoise(sd, topo, noisy, 50, 3, **okw)
    d = float((out.double() - want.double()).abs().max())
    print(f"case {cid} {compute} B={B}: {len(steps)} iterations, max|denoise - oracle| = {d:.2e}")
    assert torch.isfinite(out).all() and d < TOL_FINAL
