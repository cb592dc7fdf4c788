"""compute="f16" (MI_COMPUTE_F16 = 2) without a GPU: the mode is accepted by every host layer, its plans name only one-plane
kernel instantiations, the hand-counted DMA waits of the one-plane 3x3 / 1x1 instantiations hold in the replay model of
tests/test_dma_protocol_cpu.py, the compiled one-plane kernels really issue one MFMA per product and no lo-half arithmetic,
and (build container only) the fixtures' yardstick E is reproducible and the oracle may stand in for the reference under the
autocast emulation (tests/f16_emulation.py)."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from midd_amd import UNetConfig, UNetDiffusion, native, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from tests import golden
from tests.f16_emulation import AutocastEmulation, distance
from tests.test_abi_cpu import _cfg_struct
from tests.test_dma_protocol_cpu import instantiated_tiles, replay
from tests.test_plan_dump_cpu import launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medical-image-denoising-using-diffusion_amd", "csrc")


# ------------------------------------------------------------------------------ 1. the mode exists in every host layer
def test_mode_2_is_accepted_by_abi_and_python_and_only_by_argument(monkeypatch):
    lib = native.lib()
    assert native.MI_COMPUTE["f16"] == 2
    for flags in (0, native.MI_COMPUTE_BATCH_INVARIANT):
        s = _cfg_struct(UNetConfig())
        s.compute_mode = 2 | flags
        h = C.c_void_p()
        assert lib.mi_unet_plan_create(C.byref(s), C.byref(h)) == 0, lib.mi_last_error()
        assert lib.mi_unet_num_weights(h) == 308
        lib.mi_plan_destroy(h)
    s = _cfg_struct(UNetConfig())
    s.compute_mode = 7
    h = C.c_void_p()
    assert lib.mi_unet_plan_create(C.byref(s), C.byref(h)) == -1 and b"unknown compute_mode 7" in lib.mi_last_error()

    monkeypatch.delenv("MIDD_COMPUTE", raising=False)
    assert UNetDiffusion(compute="f16").compute == "f16"
    assert UNetDiffusion().compute == "f16x3", "the default does not change"
    assert UNetDiffusion(variant="cddpm").compute == "f16x3"
    monkeypatch.setenv("MIDD_COMPUTE", "f16")
    with pytest.raises(ValueError) as ei:            # the reduced-precision mode is never selected by the environment
        UNetDiffusion()
    assert 'compute="f16"' in str(ei.value), "the message points to the argument"
    assert UNetDiffusion(compute="f16").compute == "f16" and UNetDiffusion(compute="f16x3").compute == "f16x3"
    monkeypatch.setenv("MIDD_COMPUTE", "f32")
    assert UNetDiffusion().compute == "f32"          # the environment still selects between the parity modes


def test_callers_forward_the_argument():
    import inspect
    from midd_amd import cli, hybrid, server
    assert "compute" in inspect.signature(cli.denoise_image_diffusion).parameters
    assert "compute" in inspect.signature(hybrid.HybridDenoisingRouter.__init__).parameters
    svc = server.DiffusionService(device=torch.device("cpu"), compute="f16")
    svc.load_models()
    assert svc.diffusion_model.compute == "f16"
    svc = server.DiffusionService(device=torch.device("cpu"))
    svc.load_models()
    assert svc.diffusion_model.compute == "f16x3"


# ------------------------------------------------------------------------------ 2. what an f16 plan launches
# every kernel the f16 plans of the shipped configurations reach (recorded from the planner: the f16x3 picker's choices, one plane)
F16_INVENTORY = {
    "midd::attention_f16_kernel<96>",
    "midd::conv1x1_f16_kernel<1, 3, 1>", "midd::conv1x1_f16_kernel<1, 3, 2>", "midd::conv1x1_f16_kernel<2, 3, 1>",
    "midd::conv_mfma_f16_kernel<3, 1, 16, 1, 3, 4, 1, false, 0>", "midd::conv_mfma_f16_kernel<3, 1, 16, 1, 3, 4, 1, false, 2>",
    "midd::conv_mfma_f16_kernel<3, 1, 16, 1, 3, 4, 1, true, 0>", "midd::conv_mfma_f16_kernel<3, 1, 16, 1, 3, 4, 1, true, 2>",
    "midd::conv_mfma_f16_kernel<3, 1, 16, 2, 3, 4, 1, false, 0>", "midd::conv_mfma_f16_kernel<3, 1, 16, 2, 3, 4, 1, false, 2>",
    "midd::conv_mfma_f16_kernel<3, 1, 16, 2, 3, 4, 1, true, 0>", "midd::conv_mfma_f16_kernel<3, 1, 16, 2, 3, 4, 1, true, 2>",
    "midd::conv_mfma_f16_kernel<3, 1, 8, 1, 3, 2, 1, false, 0>", "midd::conv_mfma_f16_kernel<3, 1, 8, 1, 3, 2, 1, true, 0>",
    "midd::conv_mfma_f16_kernel<3, 2, 16, 1, 3, 4, 1, false, 0>", "midd::conv_mfma_f16_kernel<3, 2, 16, 2, 3, 4, 1, false, 0>",
    "midd::conv_mfma_f16_kernel<3, 2, 8, 1, 3, 2, 1, false, 0>",
    "midd::in_conv1_kernel", "midd::out_conv_kernel<1>", "midd::resize_bilinear_kernel",
}
SHIPPED = [(1, 256), (4, 256), (8, 256), (32, 256), (8, 512)]


def test_f16_plans_name_only_one_plane_instantiations():
    seen = set()
    for (B, S), side in itertools.product(SHIPPED, (0, 1)):
        text, rows = launches({}, B, S, S, side, compute="f16")
        assert len(rows) == 73 and "ops=73" in text
        for r in rows:
            k = r["kernel"]
            seen.add(k)
            assert "f16x3" not in k and "_f32_" not in k, r["line"]          # no launch goes through another mode's kernel
            if " conv " in r["line"] or " attn " in r["line"]:
                assert re.match(r"midd::(conv_mfma_f16_kernel|conv1x1_f16_kernel|attention_f16_kernel)<", k), r["line"]
            if r["lds"] is not None:
                assert r["lds"] <= 160 * 1024, r["line"]
        # the f16 plan is the f16x3 plan with the kernels' names changed: same tiles, grids, splits (the picker's choices are kept)
        _, rows3 = launches({}, B, S, S, side, compute="f16x3")
        assert [r["kernel"].replace("_f16x3_", "_f16_") for r in rows3] == [r["kernel"] for r in rows]
        assert [r["grid"] for r in rows3] == [r["grid"] for r in rows]
    assert seen == F16_INVENTORY, seen ^ F16_INVENTORY


def test_one_plane_geometry_halves_slices_and_deepens_rings():
    """The sibling hook of mi_debug_conv16_geometry: planes = 2 is the existing hook, planes = 1 halves the weight pieces per
    step (so never more pieces per wave), stages the same activation pieces, and never has a shallower ring."""
    lib = native.lib()

    def geo(ks, stride, tile, cb, planes=None):
        out = [C.c_int() for _ in range(4)]
        rc = (lib.mi_debug_conv16_geometry(ks, stride, *tile, cb, *[C.byref(v) for v in out]) if planes is None else
              lib.mi_debug_conv16_geometry_planes(ks, stride, *tile, cb, planes, *[C.byref(v) for v in out]))
        return None if rc else tuple(v.value for v in out)
    for tile in instantiated_tiles():
        for ks, stride in ((3, 1), (3, 2), (1, 1)):
            two, one = geo(ks, stride, tile, 0, 2), geo(ks, stride, tile, 0, 1)
            assert two == geo(ks, stride, tile, 0)
            assert one is not None and one[0] >= two[0] and one[1] <= two[1] and one[2] == two[2] and one[3] <= 160 * 1024, (tile, ks, stride, one, two)
    # the tile the f16x3 picker had to reject for its two-slot ring (2x2 waves, 96 couts) gets five with 6 KB slices:
    # (53248 - 16704 fixed bytes) / 6144 = 5.9
    assert geo(3, 1, (16, 2, 3, 2, 2), 0, 2)[0] == 2 and geo(3, 1, (16, 2, 3, 2, 2), 0, 1)[0] == 5
    assert geo(3, 1, (16, 2, 3, 4, 1), 0, 3) is None and b"planes" in lib.mi_last_error()
    assert geo(3, 1, (16, 4, 3, 4, 1), 0, 1) is None and b"not instantiated" in lib.mi_last_error()


# ------------------------------------------------------------------------------ 3. the DMA protocol of the one-plane instantiations
def test_every_vmcnt_immediate_of_every_one_plane_instantiation():
    """tests/test_dma_protocol_cpu.py's replay (one wave's program order as a queue of outstanding operations), fed with the
    ring depth and pieces per wave of the ONE-PLANE geometry: the kernel text is the same, so the protocol is; what changes
    are the numbers the immediates are computed from (deeper rings, fewer weight pieces per wave)."""
    lib = native.lib()
    checked, worst = 0, 0
    for tile in instantiated_tiles():
        tw, mt, nt, wm, wn = tile
        variants = [(3, 1, 0), (3, 2, 0), (1, 1, 0)]
        if tile in ((16, 2, 3, 4, 1), (16, 1, 3, 4, 1)):
            variants.append((3, 1, 2))
        for ks, stride, cbt in variants:
            out = [C.c_int() for _ in range(4)]
            if lib.mi_debug_conv16_geometry_planes(ks, stride, *tile, cbt, 1, *[C.byref(v) for v in out]) != 0:
                continue
            ring, ppw, apw, lds = (v.value for v in out)
            assert 2 <= ring <= 6 and lds <= 160 * 1024
            cb = cbt if cbt else (2 if ks == 1 else 1)
            res_options = (0, 1, 2, 3, 4, 6, 9, 12) if (ks == 3 and stride == 1) else (0,)
            for nblk, res_steps, tiles_per_wg, has_resid in itertools.product((1, 2, 3, 6, 9, 24), res_options, (1, 2, 3), (False, True)):
                worst = max(worst, replay(ks, ring, ppw, apw, mt, nt, wm, cb, nblk, res_steps, tiles_per_wg, has_resid))
                checked += 1
    assert checked > 5000 and worst <= 63
    print(f"{checked} one-plane schedules replayed; largest vmcnt immediate {worst}")


# ------------------------------------------------------------------------------ 4. the compiled kernels
@pytest.fixture(scope="module")
def f16_isa(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    out_dir = tmp_path_factory.mktemp("isa_f16")

    def one(src):
        out = os.path.join(str(out_dir), src + ".s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", os.path.join(CSRC, src), "-o", out],
                       check=True, capture_output=True, timeout=1200)
        return src, open(out).read()
    with ThreadPoolExecutor(max_workers=3) as ex:
        return dict(ex.map(one, ["conv_mfma_f16x3.hip", "conv1x1_f16x3.hip", "attention_f16x3.hip"]))


def _kernel_bodies(text, stem):
    """{template arguments (mangled tail): instruction lines} of every kernel whose mangled name starts with `stem`."""
    out = {}
    for m in re.finditer(r"^(_ZN4midd\d+" + stem + r"I\w+):.*\n", text, re.M):
        end = text.index(".end_amdhsa_kernel", m.end())
        out[m.group(1).split(stem, 1)[1]] = [l.strip().split(" ")[0] for l in text[m.end():end].splitlines() if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    return out


@pytest.mark.parametrize("src,two,one", [("conv_mfma_f16x3.hip", "conv_mfma_f16x3_kernel", "conv_mfma_f16_kernel"),
                                         ("conv1x1_f16x3.hip", "conv1x1_f16x3_kernel", "conv1x1_f16_kernel"),
                                         ("attention_f16x3.hip", "attention_f16x3_kernel", "attention_f16_kernel")])
def test_one_plane_kernels_issue_a_third_of_the_mfmas_and_no_lo_half(f16_isa, src, two, one):
    """So that the mode cannot silently be f16x3 under another name: every one-plane instantiation has exactly one third of the
    v_mfma instructions of its split-fp16 twin, and none of the v_fma_mix{lo,hi}_f16 that form the lo half."""
    k2, k1 = _kernel_bodies(f16_isa[src], two), _kernel_bodies(f16_isa[src], one)
    assert k2 and set(k2) == set(k1), set(k2) ^ set(k1)
    for args in k2:
        n2, n1 = sum(i.startswith("v_mfma") for i in k2[args]), sum(i.startswith("v_mfma") for i in k1[args])
        assert n1 > 0 and n2 == 3 * n1, (args, n2, n1)
        assert all(i == "v_mfma_f32_16x16x32_f16" for i in k1[args] if i.startswith("v_mfma")), args
        mix2, mix1 = (sum(i.startswith("v_fma_mix") for i in k[args]) for k in (k2, k1))
        if src == "attention_f16x3.hip":
            # the compiler also fuses q's scale-and-round (fp16(q * scale), the hi half itself) into v_fma_mixlo_f16, in both
            # kernels: what must be gone are the lo halves of q and of P
            assert 0 < mix1 < mix2 / 2, (args, mix2, mix1)
        else:
            assert mix1 == 0 and mix2 > 0, (args, mix2, mix1)
        assert any(i == "v_cvt_pk_f16_f32" for i in k1[args]), args
    print(f"{src}: {len(k2)} instantiations, MFMA count exactly 3 : 1")


# ------------------------------------------------------------------------------ 5. the yardstick (build container only)
@pytest.mark.reference
def test_oracle_under_emulation_is_the_reference_under_emulation_and_E_is_reproducible(reference_module):
    """Case (a) of the fixtures (full ddim network, B = 2, 64 x 64, 50 iterations): the repository's oracle under the autocast
    emulation equals the reference under it (<= 1e-6), which licenses the oracle as the live yardstick of the GPU tests; and the
    E stored in the fixture is what a recomputation from the reference gives."""
    from oracle import ddim_oracle as orc
    from tests.golden.make_golden import build
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    g = golden.load("f16_mode_ddim_64")
    cfg = UNetConfig()
    sd = make_state_dict(cfg, seed=int(g["seed_weights"]))
    noisy = torch.from_numpy(synthetic_xray(2, 64, 64, seed=int(g["seed_image"])))
    den = reference_module.ddim.DiffusionDenoiser(build(reference_module.ddim, cfg, seed=int(g["seed_weights"]), perturb=False), noise_steps=50)
    with torch.no_grad():
        ref32 = den.denoise(noisy.clone(), inference_steps=50).numpy()
        with AutocastEmulation(True) as mode:
            ref_emu = den.denoise(noisy.clone(), inference_steps=50).numpy()
        assert mode.calls > 50 * 70, "the emulation must see the network's contractions"
        with AutocastEmulation(True):
            orc_emu = orc.denoise(orc.to_torch(sd), topology(cfg), noisy, noise_steps=50, inference_steps=50).numpy()
    d = distance(orc_emu, ref_emu)
    e_max, e_rms = distance(ref_emu, ref32)
    print(f"oracle vs reference under the emulation: {d[0]:.2e}; E recomputed {e_max:.3e} / {e_rms:.3e}, stored {float(g['x_E_max']):.3e} / {float(g['x_E_rms']):.3e}")
    assert d[0] <= 1e-6
    # A recomputation may run with another thread count: torch's CPU kernels then sum in another order, the fp32 values move by
    # ~1e-7, and a few of the ~10^8 fp16 roundings of the run fall the other way.  The root-mean-square barely sees that (2 %);
    # the maximum is one pixel's value and may be another pixel's after it (10 %).
    assert abs(e_max - float(g["x_E_max"])) <= 0.10 * e_max and abs(e_rms - float(g["x_E_rms"])) <= 0.02 * e_rms
    assert np.abs(ref32 - g["x_fp32"]).max() <= 1e-5


def test_fixtures_carry_their_yardstick():
    for name, keys in (("f16_mode_ddim_64", ["x"] + [f"{q}_it{k}" for q in ("eps", "x") for k in (0, 24, 49)]),
                       ("f16_mode_cddpm_64", ["x"]), ("f16_mode_ddim_128", ["x"])):
        g = golden.load(name)
        for k in keys:
            e = distance(g[f"{k}_emu"], g[f"{k}_fp32"])
            assert e == (float(g[f"{k}_E_max"]), float(g[f"{k}_E_rms"])) and 1e-5 < e[1] < e[0] < 2e-2, (name, k, e)
    g = golden.load("f16_mode_cddpm_64")
    assert sum(k.startswith("step_noise_") for k in g.files) == 50 and g["step_noise_07"].shape == (2, 1, 64, 64)
