"""The device at activation magnitudes other than 1: the residual stream scaled by an exact power of two (tests/scale_cases.py: the
lever), a batch whose samples sit at three different scales, the all-zero stream, and the top of the statistics range.  What only
this exercises: the 120-bit GroupNorm totals away from 2^0 (csrc/stats_common.h), the per-(sample, convolution) power-of-two prescale
of raw split-fp16 operands and its undoing in the epilogue, the weight exponents of csrc/midd_weights.hip, ACT_PRESCALE / ATT_PRESCALE.

Reference: the float64 chained walk (tests/topology_cases.py::walk) on the same scaled weights.  Gates: TOL_LAYER / TOL_EPS of
tests/test_gpu_parity.py, layer errors relative to max(2^k, max|layer| of the sample) -- fp32 arithmetic is equivariant under
power-of-two scaling, so a correct kernel meets at 2^k the gate it meets at 1.  The fp32 oracle's own error on every case is below
1e-5 (tests/test_scale_cases_cpu.py).  Every test prints what it gated on; DESIGN.md records the table.
"""
import functools

import pytest
import torch

from midd_amd import UNetDiffusion, DiffusionDenoiser
from midd_amd import native
from midd_amd.weights import synthetic_xray
from oracle import ddim_oracle as orc
from tests import scale_cases as sc
from tests.test_gpu_parity import COMPUTE_MODES, TOL_EPS, TOL_FINAL, TOL_LAYER

pytestmark = pytest.mark.gpu

CIDS = sorted(sc.CONFIGS)


@functools.lru_cache(maxsize=None)
def _model(cid, compute, batch_invariant=False):
    """One model per (configuration, mode); `_load` swaps the weights (the plan re-uploads when a parameter changed)"""
    variant, kw, _, _, _ = sc.CONFIGS[cid]
    return UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant, **kw).to("cuda").eval()


def _load(cid, compute, sd, batch_invariant=False):
    m = _model(cid, compute, batch_invariant)
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    m.check_status = True
    return m


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


def _forward(model, topo, x, cond, t):
    eps = model(x.cuda(), cond.cuda(), t.cuda()).cpu()
    return eps, _fetch_all(model, topo, x)


def _gate(label, eps, dev, trace, w64, floor):
    """Per layer rel_per_sample(floor) < TOL_LAYER, eps with floor 1 < TOL_EPS; prints the worst layer, the fp32 oracle's error on
    the same layer and the ratio (not gated)."""
    worst ={n: sc.rel_per_sample(v, w64[n], floor) for n, v in dev.items()}
    d_eps = sc.rel_per_sample(eps, w64["out_conv"], 1.0)
    top = max(worst, key=lambda n: float("inf") if worst[n] != worst[n] else worst[n])
    own = sc.rel_per_sample(trace[top], w64[top], floor)
    own_eps = sc.rel_per_sample(trace["out_conv"], w64["out_conv"], 1.0)
    print(f"{label}: worst layer {top} {worst[top]:.2e} (fp32 oracle {own:.2e}, ratio {worst[top] / max(own, 1e-30):.1f}); "
          f"eps {d_eps:.2e} (fp32 oracle {own_eps:.2e}, ratio {d_eps / max(own_eps, 1e-30):.1f})")
    failed = {n: v for n, v in worst.items() if not v < TOL_LAYER}
    assert not failed, failed
    assert d_eps < TOL_EPS, d_eps
    assert bool(torch.isfinite(eps).all())
    return worst[top], d_eps


# ------------------------------------------------------------------------------ a. uniform scale
@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("k", sc.GPU_SCALES)
@pytest.mark.parametrize("cid", CIDS)
def test_uniform_scale_per_layer_vs_float64(cid, k, compute):
    cfg, topo, _, x, cond, t = sc.case(cid)
    sdk, trace, w64 = sc.reference(cid, k)
    eps, dev = _forward(_load(cid, compute, sdk), topo, x, cond, t)
    _gate(f"{cid} {compute} k={k}", eps, dev, trace, w64, floor=2.0 ** k)


# ------------------------------------------------------------------------------ b. zero stream
@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("cid", CIDS)
def test_zero_stream(cid, compute):
    """s = 0: the sum of squares of every raw operand is 0 (raw_prescale_exp's S = 0 branch), var = 0 in every GroupNorm prologue; no
    MiddError, every stream layer exactly zero, eps -- a function of the betas and out_conv alone -- within the gate."""
    cfg, topo, _, x, cond, t = sc.case(cid)
    sdk, trace, w64 = sc.reference(cid, None)
    eps, dev = _forward(_load(cid, compute, sdk), topo, x, cond, t)
    assert dev
    for name, v in dev.items():
        assert float(v.abs().max()) == 0.0, name
    d = sc.rel_per_sample(eps, w64["out_conv"], 1.0)
    print(f"{cid} {compute} zero stream: eps {d:.2e}, max|eps| {float(w64['out_conv'].abs().max()):.3f}")
    assert bool(torch.isfinite(eps).all()) and d < TOL_EPS


# ------------------------------------------------------------------------------ c. mixed-scale batch
@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cid", CIDS)
def test_mixed_scale_batch_per_layer_vs_float64(cid, reverse, compute):
    """Samples scaled by (2^-10, 1, 2^12) -- and in the reverse order -- in one launch: their raw-operand exponents differ by 5 to 11,
    so an exponent or a total read from a neighbouring sample shows in that sample's own relative error."""
    cfg, topo, sd, _, _, _ = sc.case(cid)
    xm, cm, t, trace, w64 = sc.mixed_reference(cid, reverse)
    eps, dev = _forward(_load(cid, compute, sd), topo, xm, cm, t)
    _gate(f"{cid} {compute} mixed{' reversed' if reverse else ''}", eps, dev, trace, w64, floor=1.0)


@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("cid", CIDS)
def test_mixed_scale_batch_rows_equal_the_samples_alone(cid, compute):
    """batch_invariant=True: each sample at B = 1 equals its row of the mixed batch bit for bit, eps and every fetchable layer."""
    cfg, topo, sd, _, _, _ = sc.case(cid)
    xm, cm, t, _, _ = sc.mixed_reference(cid)
    model = _load(cid, compute, sd, batch_invariant=True)
    eps, dev = _forward(model, topo, xm, cm, t)
    assert bool(torch.isfinite(eps).all())
    for i in range(xm.shape[0]):
        one, one_dev = _forward(model, topo, xm[i:i + 1], cm[i:i + 1], t[i:i + 1])
        assert one_dev.keys() == dev.keys()
        differ = [n for n in dev if not torch.equal(one_dev[n][0], dev[n][i])]
        assert not differ, (i, differ)
        assert torch.equal(one[0], eps[i]), i


# ------------------------------------------------------------------------------ d. sampler
@pytest.mark.parametrize("compute", COMPUTE_MODES)
def test_sampler_at_scale_vs_oracle(compute):
    """denoise, 3 inference steps, default network at k = 12: the update kernels see the same eps whatever the stream's scale."""
    cfg, topo, _, _, _, _ = sc.case("default")
    sdk = sc.reference("default", 12)[0]
    noisy = torch.from_numpy(synthetic_xray(2, 24, 40, seed=912))
    want = orc.denoise(sdk, topo, noisy, 50, 3)
    out = DiffusionDenoiser(_load("default", compute, sdk), noise_steps=50).denoise(noisy.cuda(), inference_steps=3).cpu()
    d = float((out.double() - want.double()).abs().max())
    print(f"default {compute} k=12 B=2: max|denoise - oracle| = {d:.2e}")
    assert bool(torch.isfinite(out).all()) and d < TOL_FINAL


# ------------------------------------------------------------------------------ e. the upper end is reported, never returned
@pytest.mark.parametrize("compute", COMPUTE_MODES)
@pytest.mark.parametrize("k", sc.ERANGE_SCALES)
@pytest.mark.parametrize("cid", ["default", "small"])
def test_beyond_the_statistics_range_is_reported(cid, k, compute):
    """At k >= 32 every activation is finite (the fp32 oracle is finite and right: tests/test_scale_cases_cpu.py) but a workgroup's
    partial sum of squares is >= 2^63, four binades past what the totals hold (same file: ..._keep_their_distance_...): the call
    raises MI_ERANGE and says why; with the status check off the image is NaN -- never finite and wrong."""
    cfg, topo, _, x, cond, t = sc.case(cid)
    sdk, trace, w64 = sc.reference(cid, k)
    assert all(bool(torch.isfinite(v).all()) for v in trace.values())
    model = _load(cid, compute, sdk)
    with pytest.raises(native.MiddError) as ei:
        model(x.cuda(), cond.cuda(), t.cuda())
    print(f"{cid} {compute} k={k}: {ei.value}")
    assert ei.value.code == -5 and "statistics range" in str(ei.value)
    model.check_status = False
    try:
        eps = model(x.cuda(), cond.cuda(), t.cuda()).cpu()
    finally:
        model.check_status = True
    want = w64["out_conv"]
    finite = torch.isfinite(eps)
    bound = TOL_EPS * want.abs().reshape(want.shape[0], -1).amax(dim=1).clamp_min(1.0).reshape(-1, 1, 1, 1)
    wrong = finite & ((eps.double() - want).abs() >= bound)
    print(f"{cid} {compute} k={k} unchecked: {int(finite.sum())} of {eps.numel()} pixels finite, {int(wrong.sum())} of them wrong")
    assert int(wrong.sum()) == 0
    assert bool(torch.isnan(eps).any())
