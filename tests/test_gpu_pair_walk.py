"""GPU: the pair walk of the fp16-MFMA 3x3 kernel with 16-channel chunks (two chunks in 4 + 5 K steps, the shared step carrying
tap 8 of the even chunk in registers across the transform of the odd one; csrc/conv_mfma_f16x3_body.h: PAIR).

Per-module outputs of the default network (`mi_debug_fetch`) against the CPU oracle's trace, in the two compute modes that run
this kernel text:
  * "f16x3": the per-module gate of tests/test_gpu_parity.py, max|d| < TOL_LAYER = 2e-4;
  * "f16"  : that mode's own acceptance rule (tests/f16_emulation.py: max|d| <= 2 E_max, rms <= 1.5 E_rms, E = the oracle under
             the autocast emulation against the fp32 oracle), applied per module -- 2e-4 is not a bound a one-product fp16 mode
             meets or is meant to meet.
Shapes, the smallest that reach what can go wrong:
  * B = 1, 64 x 64   chunk counts 3, 6, 9, 12 and the concatenated 18 / 24: pairs plus an unpaired tail (48, 144 channels), small tiles;
  * B = 3, 40 x 24   ragged tile edges; tiles whose halo leaves the image, so the stash read and the shared step's tap 0 meet the
                     zero padding written in chunk 0 only;
  * B = 8, 128 x 128 1024 tiles per sample > 768 persistent workgroups: two tiles per workgroup, i.e. the pairing restarts at a
                     tile switch with the weight ring running on cyclically, and the res phase sits between two tiles.
                     The oracle runs rows 0 and 7 only (samples are independent; CPU time).
The 64-pixel tile (16, 1, 3, 4, 1) -- five ring slots, the one tile on which a 4-step chunk leaves fewer weight groups behind the
next chunk than the ring holds (after = 3 < D = 4) -- is picked by side-by-side sub-batch programs only; a single forward takes
it in batch-invariant mode, which plans every launch as such a sub-batch would: B = 1, 64 x 64 with `batch_invariant=True`, per
module under the same gates (the oracle trace of the first shape is reused).
A further case reaches the same tile the way the benchmark does, through two side-by-side sub-batch programs: a 3-iteration
sampler run at B = 4, 48 x 48 (two programs of 2), judged on the sampler output with the sampler gates of the two modes
(1e-3; the f16 rule).
Host-side (plan dump): these shapes cover every pair-walk instantiation the plans of the benchmark's shapes launch, and the
B = 8 case really has more tiles than persistent workgroups per sample."""
import re

import numpy as np
import pytest
import torch

from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests.f16_emulation import AutocastEmulation, distance, gate
from tests.test_plan_dump_cpu import launches

pytestmark = pytest.mark.gpu

TOL_LAYER = 2e-4          # tests/test_gpu_parity.py: per-module activations
TOL_FINAL = 1e-3          # tests/test_gpu_parity.py: sampler output
SIDE_CASE = (4, 48, 48)   # sampler run: two sub-batch programs of 2
SHAPES = {"b1_64": (1, 64, 64, [0]), "b3_40x24": (3, 40, 24, [0, 1, 2]), "b8_128": (8, 128, 128, [0, 7])}
PAIR_WALK = re.compile(r"midd::conv_mfma_f16(?:x3)?_kernel<3, [12], \d+, \d+, \d+, \d+, \d+, (?:false|true), 0>$")


@pytest.fixture(scope="module")
def sd():
    return make_state_dict(UNetConfig(), seed=42)


@pytest.fixture(scope="module")
def models(sd):
    out = {}
    for compute in ("f16x3", "f16"):
        m = UNetDiffusion(compute=compute)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        out[compute] = m.to("cuda").eval()
    return out


@pytest.fixture(scope="module")
def invariant_models(sd):
    out = {}
    for compute in ("f16x3", "f16"):
        m = UNetDiffusion(compute=compute, batch_invariant=True)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        out[compute] = m.to("cuda").eval()
    return out


@pytest.fixture(scope="module")
def oracle_traces(sd):
    """shape -> (inputs, {module: fp32 output}, {module: output under the autocast emulation}), computed once, never modified."""
    cache = {}

    def get(name):
        if name not in cache:
            B, H, W, rows = SHAPES[name]
            x = torch.from_numpy(synthetic_xray(B, H, W, seed=71, kind="uniform"))
            c = torch.from_numpy(synthetic_xray(B, H, W, seed=72))
            t = torch.tensor([49, 3, 17, 0, 25, 40, 9, 33][:B])
            sdt, topo = orc.to_torch(sd), topology(UNetConfig())
            fp32, emu = {}, {}
            with torch.no_grad():
                orc.unet_forward(sdt, topo, x[rows], c[rows], t[rows], trace=lambda n, v: fp32.__setitem__(n, v.numpy().copy()))
                with AutocastEmulation(True):
                    orc.unet_forward(sdt, topo, x[rows], c[rows], t[rows], trace=lambda n, v: emu.__setitem__(n, v.float().numpy().copy()))
            cache[name] = (x, c, t, fp32, emu)
        return cache[name]

    return get


@pytest.mark.parametrize("compute", ["f16x3", "f16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_per_module_outputs_vs_oracle(models, oracle_traces, shape, compute):
    _per_module(models[compute], oracle_traces, shape, compute)


@pytest.mark.parametrize("compute", ["f16x3", "f16"])
def test_per_module_outputs_on_the_64_pixel_tile(invariant_models, oracle_traces, compute):
    _per_module(invariant_models[compute], oracle_traces, "b1_64", compute)


def _per_module(model, oracle_traces, shape, compute):
    B, H, W, rows = SHAPES[shape]
    x, c, t, fp32, emu = oracle_traces(shape)
    eps = model(x.cuda(), c.cuda(), t.cuda())
    torch.cuda.synchronize()
    assert torch.isfinite(eps).all()
    worst, checked = {}, 0
    for name, want in fp32.items():
        if name == "time_mlp":
            continue
        if name == "out_conv":
            got = eps.cpu().numpy()[rows]
        else:
            try:
                got = model.debug_fetch(name, B, H, W).cpu().numpy()[rows]
            except native.MiddError:
                # a ConvTranspose folded into its consumer has no materialised output
                assert any(m.name == name and m.kind == "up" for m in topology(UNetConfig()).ups), name
                continue
        assert got.shape == want.shape, name
        checked += 1
        if compute == "f16x3":
            worst[name] = distance(got, want)[0]
        else:
            e_max, e_rms = distance(emu[name], want)
            if e_max == 0.0:                     # a module the emulation leaves in fp32 (nothing rounded yet)
                worst[name] = distance(got, want)[0]
                assert worst[name] < TOL_LAYER, name
            else:
                worst[name] = gate(got, want, e_max, e_rms, f"{shape} {name}")[0]
    print(f"{shape} {compute}: {checked} modules, worst {max(worst, key=worst.get)} {max(worst.values()):.2e}")
    assert checked >= 20
    if compute == "f16x3":
        assert max(worst.values()) < TOL_LAYER, max(worst, key=worst.get)


@pytest.mark.parametrize("compute", ["f16x3", "f16"])
def test_side_by_side_sampler_vs_oracle(models, sd, compute):
    B, H, W = SIDE_CASE
    noisy = torch.from_numpy(synthetic_xray(B, H, W, seed=73))
    sdt, topo = orc.to_torch(sd), topology(UNetConfig())
    want = orc.denoise(sdt, topo, noisy, noise_steps=50, inference_steps=3).numpy()
    got = DiffusionDenoiser(models[compute], noise_steps=50).denoise(noisy.cuda(), inference_steps=3).cpu().numpy()
    d = distance(got, want)[0]
    print(f"side-by-side sampler {compute}: max|d| = {d:.3e}")
    if compute == "f16x3":
        assert d < TOL_FINAL
    else:
        with AutocastEmulation(True):
            emu = orc.denoise(sdt, topo, noisy, noise_steps=50, inference_steps=3).float().numpy()
        gate(got, want, *distance(emu, want), "side-by-side sampler")


def _pair_walk_kernels(B, H, W, side, compute):
    _, rows = launches({}, B, H, W, side, compute)
    return {r["kernel"] for r in rows if PAIR_WALK.match(r["kernel"])}


@pytest.mark.parametrize("compute", ["f16x3", "f16"])
def test_the_three_shapes_reach_the_benchmarks_pair_walk_instantiations(compute):
    """Every 16-channel-chunk 3x3 instantiation launched by the plans of the benchmark's shapes (B = 8 at 256 x 256 as two
    sub-batch programs of 4, the same unsplit, and the single image) is launched by at least one of the shapes above
    (host only: mi_debug_plan_dump).  DESIGN.md section 5 lists the pair-walk instantiations no GPU test of this file reaches."""
    reached = _pair_walk_kernels(SIDE_CASE[0] // 2, SIDE_CASE[1], SIDE_CASE[2], 1, compute)
    for B, H, W, _ in SHAPES.values():
        reached |= _pair_walk_kernels(B, H, W, 0, compute)
    bench = _pair_walk_kernels(4, 256, 256, 1, compute) | _pair_walk_kernels(8, 256, 256, 0, compute) | _pair_walk_kernels(1, 256, 256, 0, compute)
    print(f"{compute}: reached {sorted(reached)}\nbenchmark plans {sorted(bench)}")
    assert bench and bench <= reached, sorted(bench - reached)
    # both members of a pair, an unpaired tail and the folded res_conv are among them
    assert any(", true, 0>" in k for k in reached) and any("<3, 2," in k for k in reached)


@pytest.mark.parametrize("compute", ["f16x3", "f16"])
def test_the_b8_128_case_really_walks_two_tiles_per_workgroup(compute):
    """What the B = 8, 128 x 128 case is for (host only, from the plan dump): at least one pair-walk launch WITH and one WITHOUT the
    folded res_conv has more tiles per sample than persistent workgroups per sample, so the pairing restarts at a tile switch."""
    B, H, W, _ = SHAPES["b8_128"]
    _, rows = launches({}, B, H, W, 0, compute)
    multi = set()
    for r in rows:
        m = re.search(r"wgs/img (\d+) tiles (\d+)x(\d+)", r["line"])
        if m and PAIR_WALK.match(r["kernel"]) and int(m.group(2)) * int(m.group(3)) > int(m.group(1)):
            multi.add(", true, 0>" in r["kernel"])
    assert multi == {False, True}, multi
