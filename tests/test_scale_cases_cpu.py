"""Host-only checks of tests/scale_cases.py: the lever scales the residual stream and nothing else, and the references the GPU tests
(tests/test_gpu_dynamic_range.py) compare against are themselves easy for fp32 at every scale -- the fp32 oracle stays 20x inside
the gate the device is held to, so a device failure there is the device's.
"""
import pytest
import torch

from tests import scale_cases as sc

CIDS = sorted(sc.CONFIGS)
ORACLE_VS_WALK = 1e-5            # the fp32 oracle against the float64 walk, per layer and sample: 20x under TOL_LAYER = 2e-4


def _finite(tensors):
    return all(bool(torch.isfinite(v).all()) for v in tensors.values())


@pytest.mark.parametrize("cid", CIDS)
def test_scaled_state_dict_touches_the_stream_writers_only(cid):
    cfg, topo, sd, _, _, _ = sc.case(cid)
    whole, bias_only = sc.stream_writers(topo)
    sdk = sc.scaled_state_dict(sd, topo, 12)
    assert sdk.keys() == sd.keys()
    for name in sd:
        prefix, leaf = name.rsplit(".", 1)
        scaled = prefix in whole or (prefix in bias_only and leaf == "bias")
        assert torch.equal(sdk[name], sd[name] * (4096.0 if scaled else 1.0)), name
        assert sdk[name].data_ptr() != sd[name].data_ptr(), name
    # every reader of the stream is left alone, every kind of writer is present where the topology has one
    assert not any(p.endswith((".block1.2", ".block1.0", ".block2.0", ".qkv", ".norm")) or p.startswith(("out_conv", "time_mlp"))
                   for p in whole + bias_only)
    assert "in_conv" in whole and any(p.endswith(".block2.3") for p in whole) and any(p.endswith(".proj") for p in whole)
    assert any(p.endswith(".res_conv") for p in bias_only)
    assert {m.name for m in topo.downs + topo.ups if m.kind in ("down", "up")} <= set(bias_only)
    zero = sc.scaled_state_dict(sd, topo, None)
    assert all(float(zero[f"{p}.weight"].abs().max()) == 0.0 and float(zero[f"{p}.bias"].abs().max()) == 0.0 for p in whole)
    assert all(float(zero[f"{p}.bias"].abs().max()) == 0.0 and torch.equal(zero[f"{p}.weight"], sd[f"{p}.weight"]) for p in bias_only)


def test_mixed_inputs_and_rel_per_sample():
    x = torch.ones(3, 1, 2, 2)
    xm, cm = sc.mixed_inputs(x, 2 * x)
    assert [float(v.max()) for v in xm] == [2.0 ** -10, 1.0, 4096.0] and torch.equal(cm, 2 * xm)
    want = torch.tensor([1.0, 100.0, 0.0]).reshape(3, 1, 1, 1).expand(3, 1, 2, 2)
    got = want + torch.tensor([0.5, 1.0, 0.25]).reshape(3, 1, 1, 1)
    assert sc.rel_per_sample(got, want, floor=1) == 0.5               # 0.5 / 1, 1 / 100, 0.25 / max(1, 0)
    assert sc.rel_per_sample(got, want, floor=1 / 16) == 4.0          # sample 2: 0.25 / (1 / 16)
    bad = got.clone()
    bad[1, 0, 0, 0] = float("nan")
    assert not sc.rel_per_sample(bad, want, floor=1) < 1e30           # NaN never passes a gate


@pytest.mark.parametrize("k", [k for k in sc.CPU_SCALES if k is not None])
@pytest.mark.parametrize("cid", CIDS)
def test_uniform_scale_references(cid, k):
    cfg, topo, _, _, _, _ = sc.case(cid)
    _, trace0, w0 = sc.reference(cid, 0)
    _, trace, w64 = sc.reference(cid, k)
    assert _finite(trace) and _finite(w64)
    s = 2.0 ** k
    # the lever does what it is for (not exact: GroupNorm's eps = 1e-5 is not scaled)
    for name in sc.stream_layers(topo):
        ratio = float(w64[name].abs().max()) / (s * float(w0[name].abs().max()))
        assert 0.5 < ratio < 2.0, (name, ratio)
    # eps barely moves
    if k >= 0:
        d = float((w64["out_conv"] - w0["out_conv"]).abs().max()) / float(w0["out_conv"].abs().max())
        assert d < 0.05, d
    # the reference alone is far inside the device's gates
    own = {n: sc.rel_per_sample(trace[n], w64[n], floor=0) for n in trace}
    worst = max(own, key=own.get)
    print(f"{cid} k={k}: fp32 oracle vs float64 walk, worst layer {worst} {own[worst]:.2e}")
    assert all(v < ORACLE_VS_WALK for v in own.values()), (worst, own[worst])


@pytest.mark.parametrize("cid", CIDS)
def test_gated_and_reported_scales_keep_their_distance_from_the_statistics_range(cid):
    """The largest sum-of-squares partial a producer workgroup forms, bracketed for any tiling (scale_cases.partial_bracket_log2):
    at every scale the GPU tests gate it is at least four binades under 2^59, at every scale they expect MI_ERANGE at least
    four above -- neither kind of test sits near the boundary, where the outcome would depend on the planner's tiles."""
    cfg, topo, _, _, _, _ = sc.case(cid)
    for k in sc.GPU_SCALES + sc.ERANGE_SCALES:
        lo, hi = sc.partial_bracket_log2(sc.reference(cid, k)[2], topo)
        print(f"{cid} k={k}: 2^{lo:.1f} <= largest partial <= 2^{hi:.1f}; the scale at which it meets 2^59 lies in "
              f"[{k + (sc.STAT_RANGE_LOG2 - hi) / 2:.1f}, {k + (sc.STAT_RANGE_LOG2 - lo) / 2:.1f}]")
        if k in sc.GPU_SCALES:
            assert hi <= sc.STAT_RANGE_LOG2 - sc.RANGE_MARGIN_BINADES, (k, hi)
        else:
            assert lo >= sc.STAT_RANGE_LOG2 + sc.RANGE_MARGIN_BINADES, (k, lo)
    _, hi = sc.partial_bracket_log2(sc.mixed_reference(cid)[4], topo)      # the mixed batch's largest sample
    assert hi <= sc.STAT_RANGE_LOG2 - sc.RANGE_MARGIN_BINADES, hi


@pytest.mark.parametrize("cid", CIDS)
def test_zero_stream_references(cid):
    cfg, topo, _, _, _, _ = sc.case(cid)
    _, trace, w64 = sc.reference(cid, None)
    for name in sc.stream_layers(topo):
        assert float(trace[name].abs().max()) == 0.0 and float(w64[name].abs().max()) == 0.0, name
    assert bool(torch.isfinite(trace["out_conv"]).all()) and bool(torch.isfinite(w64["out_conv"]).all())
    assert float(w64["out_conv"].abs().max()) > 0.0                   # eps is then a function of the betas and out_conv
    assert sc.rel_per_sample(trace["out_conv"], w64["out_conv"], floor=0) < ORACLE_VS_WALK


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cid", CIDS)
def test_mixed_batch_references(cid, reverse):
    cfg, topo, _, _, _, _ = sc.case(cid)
    xm, cm, t, trace, w64 = sc.mixed_reference(cid, reverse)
    assert _finite(trace) and _finite(w64)
    own = {n: sc.rel_per_sample(trace[n], w64[n], floor=0) for n in trace}
    worst = max(own, key=own.get)
    first = next(m.name for m in topo.downs)
    per_sample = [float(v.abs().max()) for v in w64[first]]
    print(f"{cid} mixed{' reversed' if reverse else ''}: stream max per sample at {first} {['%.3g' % v for v in per_sample]}; "
          f"fp32 oracle vs float64 walk, worst layer {worst} {own[worst]:.2e}")
    assert all(v < ORACLE_VS_WALK for v in own.values()), (worst, own[worst])
    # the samples really sit at different scales where the raw operands are read: a factor of at least 2^5 between the extremes
    assert max(per_sample) / min(per_sample) > 32.0, per_sample
    if reverse:                                                       # the reversed batch is the same samples, in the other order
        _, _, _, _, fwd = sc.mixed_reference(cid, False)
        assert sc.rel_per_sample(w64["out_conv"].flip(0), fwd["out_conv"], floor=0) < 1e-12
