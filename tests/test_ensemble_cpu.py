"""CPU-only checks of the posterior ensembles of the cddpm sampler (include/midd.h: mi_denoise_ensemble,
mi_ensemble_workspace_bytes, mi_ensemble_reduce, mi_step_noise_fill_member): the C ABI's declarations and argument rules, the
host-only workspace size, the numpy restatement of the member-keyed generator, and the Python argument rules.  What the device
computes is judged in test_gpu_ensemble.py."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetDiffusion, native
from tests import ensemble_reference as ens
from tests.isa_dump import isa_dump
from tests import step_noise_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_denoise_ensemble", "mi_ensemble_workspace_bytes", "mi_ensemble_reduce", "mi_step_noise_fill_member"}
FAKE, NOISY = 0x10000, 0x20000          # non-null "device pointers" for calls that must fail before anything reads them


@pytest.fixture()
def plan():
    """An unfinalized cddpm plan: every host-side rule can be checked on it, no GPU call can succeed."""
    lib = native.lib()
    m = UNetDiffusion(variant="cddpm", **SMALL)
    cfg = native.UNetCfg()
    c = m.cfg
    cfg.in_channels, cfg.model_channels, cfg.num_levels = c.in_channels, c.model_channels, len(c.channel_mult)
    for i, v in enumerate(c.channel_mult):
        cfg.channel_mult[i] = v
    cfg.num_res_blocks, cfg.num_attention_levels = c.num_res_blocks, len(c.attention_resolutions)
    for i, v in enumerate(c.attention_resolutions):
        cfg.attention_levels[i] = v
    cfg.time_emb_dim, cfg.variant, cfg.compute_mode = c.time_emb_dim, native.MI_VARIANT["cddpm"], native.MI_COMPUTE["f16x3"]
    h = C.c_void_p()
    native.check(lib.mi_unet_plan_create(C.byref(cfg), C.byref(h)))
    yield h
    lib.mi_plan_destroy(h)


def _ensemble(plan, noisy=NOISY, mean=FAKE, std=None, samples=None, B=2, members=4, H=32, W=32, seed=5, sample_offset=0,
              member_offset=0, pass_samples=16):
    return native.lib().mi_denoise_ensemble(plan, noisy, mean, std, samples, B, members, H, W, None, 0, None, None, None, 50,
                                            seed, sample_offset, member_offset, pass_samples, 0, None, 0, None)


# ------------------------------------------------------------------------------ 1. declarations
def test_header_and_binding_declare_the_four_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n: a for n, _, a in native.SYMBOLS}
    assert NEW <= declared and declared == set(bound)
    lib = native.lib()
    for name in NEW:
        assert getattr(lib, name) is not None
    assert "c3 = member index" in header and "0 for mi_denoise_seeded" in header
    assert "reserved: stream id" not in header
    # the member form is the plain fill with one more 64-bit integer in front of the stream
    assert bound["mi_step_noise_fill_member"] == bound["mi_step_noise_fill"][:-1] + [C.c_int64, C.c_void_p]
    common = open(os.path.join(ROOT, "medical-image-denoising-using-diffusion_amd", "csrc", "step_noise_common.h")).read()
    assert "c3 = member index" in common


# ------------------------------------------------------------------------------ 2. argument rules, before any GPU work
@pytest.mark.parametrize("kw,words", [
    (dict(members=0), ["members >= 1"]),
    (dict(members=-3), ["members >= 1"]),
    (dict(member_offset=-1), ["member_offset -1"]),
    (dict(member_offset=(1 << 32) - 3), ["2^32", "4294967296"]),                 # + 4 members = 2^32 + 1
    (dict(pass_samples=0), ["pass_samples >= 1"]),
    (dict(mean=None), ["no output"]),
    (dict(std=FAKE, members=1), ["members >= 2"]),
    (dict(mean=FAKE, noisy=FAKE), ["alias", "noisy", "mean_out"]),
    (dict(mean=None, samples=FAKE, noisy=FAKE), ["alias", "noisy", "samples_out"]),
    (dict(mean=FAKE, std=FAKE), ["alias", "mean_out", "std_out"]),                    # the outputs among themselves
    (dict(mean=FAKE, samples=FAKE), ["alias", "mean_out", "samples_out"]),
    (dict(std=FAKE, samples=FAKE), ["alias", "std_out", "samples_out"]),
    (dict(mean=FAKE + 2 * 32 * 32 * 4 - 4, samples=FAKE + 2 * 32 * 32 * 4), ["alias"]),      # the last float of mean_out overlaps
    (dict(mean=FAKE + 3 * 32 * 32 * 4, samples=FAKE), ["alias"]),                      # mean_out inside samples_out [2,4,1,32,32]
    (dict(sample_offset=-2), ["sample_offset -2"]),
    (dict(H=65536, W=65536), ["2^32", "4294967296"]),
    (dict(B=65536, members=1), ["65535"]),
    (dict(B=0), ["65535"]),
    (dict(B=65535, members=65536), ["2147483647"]),
])
def test_every_argument_rule_names_its_limit(plan, kw, words):
    lib = native.lib()
    assert _ensemble(plan, **kw) == -1, kw
    msg = lib.mi_last_error().decode()
    for w in words:
        assert w in msg, (kw, msg)


def test_the_limits_themselves_pass_the_argument_rules(plan):
    """member_offset + members == 2^32 and B * members == 2^31 - 1 are inside; the unfinalized plan then stops the call (a
    state error, still before any GPU work)."""
    lib = native.lib()
    assert _ensemble(plan, member_offset=(1 << 32) - 4) == -2
    assert b"finalize" in lib.mi_last_error()
    assert _ensemble(plan, B=1, members=(1 << 31) - 1, mean=None, samples=FAKE, noisy=0x1000) == -2     # (8 TB of samples: noisy lies below)
    assert _ensemble(plan, members=1, member_offset=7, mean=None, samples=FAKE) == -2       # the single-member form
    assert _ensemble(None) == -1 and b"null plan" in lib.mi_last_error()
    # buffers that touch without overlapping are fine
    assert _ensemble(plan, mean=FAKE, std=FAKE + 2 * 32 * 32 * 4, samples=FAKE + 4 * 32 * 32 * 4, noisy=FAKE - 2 * 32 * 32 * 4) == -2


def test_reduce_and_member_fill_rules():
    lib = native.lib()
    assert lib.mi_ensemble_reduce(FAKE, 2, 0, 64, FAKE, None, None) == -1 and b"members >= 1" in lib.mi_last_error()
    assert lib.mi_ensemble_reduce(FAKE, 2, 1, 64, FAKE, FAKE, None) == -1 and b"members >= 2" in lib.mi_last_error()
    assert lib.mi_ensemble_reduce(FAKE, 0, 4, 64, FAKE, None, None) == -1 and b"65535" in lib.mi_last_error()
    assert lib.mi_ensemble_reduce(FAKE, 65536, 4, 64, FAKE, None, None) == -1
    assert lib.mi_ensemble_reduce(FAKE, 2, 4, 0, FAKE, None, None) == -1 and b"chw" in lib.mi_last_error()
    assert lib.mi_ensemble_reduce(FAKE, 2, 4, 1 << 32, FAKE, None, None) == -1 and b"4294967296" in lib.mi_last_error()
    assert lib.mi_ensemble_reduce(None, 2, 4, 64, FAKE, None, None) == -1 and b"null" in lib.mi_last_error()
    assert lib.mi_ensemble_reduce(FAKE, 2, 4, 64, None, None, None) == -1 and b"null" in lib.mi_last_error()
    for bad in (-1, 1 << 32):
        assert lib.mi_step_noise_fill_member(None, 1, 1, 1, 8, 8, 1, 0, bad, None) == -1
        assert b"member" in lib.mi_last_error() and b"4294967296" in lib.mi_last_error()
    assert lib.mi_step_noise_fill_member(None, 1, 1, 1, 8, 8, 1, -1, 3, None) == -1 and b"sample_offset" in lib.mi_last_error()
    assert lib.mi_step_noise_fill_member(None, 1, 1, 1, 8, 8, 1, 0, (1 << 32) - 1, None) == -1 and b"null" in lib.mi_last_error()
    assert lib.mi_step_noise_fill_member(None, 0, 4, 1, 8, 8, 1, 0, 3, None) == 0            # nothing to write


# ------------------------------------------------------------------------------ 3. workspace size (host only)
def _sampler_bytes(plan, B, H, W):
    """What mi_workspace_bytes returns for a finalized plan, from the planner's dump (which needs no finalize): the whole-batch
    program, or the two side-by-side half-batch programs when the batch splits."""
    lib = native.lib()

    def program_bytes(b, side):
        buf = C.create_string_buffer(1 << 20)
        assert lib.mi_debug_plan_dump(plan, b, H, W, side, buf, len(buf)) > 0
        return int(re.search(r"bytes=(\d+)", buf.value.decode()).group(1))
    need = program_bytes(B, 0)
    if B % 2 == 0 and B // 2 >= 2:
        need = max(need, 2 * program_bytes(B // 2, 1))
    return need


def test_workspace_bytes(plan):
    lib = native.lib()
    ws = lib.mi_ensemble_workspace_bytes
    H = W = 64
    chw = 1 * H * W
    for bad in (dict(B=0), dict(members=0), dict(pass_samples=0), dict(H=60), dict(B=65536), dict(H=65536, W=65536)):
        a = dict(B=2, members=5, H=H, W=W, pass_samples=4)
        a.update(bad)
        assert ws(plan, a["B"], a["members"], a["H"], a["W"], a["pass_samples"], 0) == 0, bad
    assert ws(None, 2, 5, H, W, 4, 0) == 0
    for B, K, p in [(2, 5, 4), (2, 5, 3), (2, 5, 16), (1, 8, 16), (8, 8, 16), (1, 1, 16)]:
        ext, internal = ws(plan, B, K, H, W, p, 1), ws(plan, B, K, H, W, p, 0)
        n = min(p, B * K)
        tail = (B * K) % n
        run = max(_sampler_bytes(plan, n, H, W), _sampler_bytes(plan, tail, H, W) if tail else 0)
        assert ext >= run + n * chw * 4, (B, K, p)                          # a pass's sampler workspace + its condition images
        assert ext <= run + n * chw * 4 + 512, (B, K, p)                    # (and two roundings to 256 bytes, nothing else)
        assert internal - ext == B * K * chw * 4, (B, K, p)                 # the member outputs, exactly
    # a pass larger than the ensemble is the ensemble
    assert ws(plan, 2, 5, H, W, 10, 0) == ws(plan, 2, 5, H, W, 1000, 0)


# ------------------------------------------------------------------------------ 4. the reference restatement
@pytest.mark.parametrize("seed", [1234, 0x1234567890ABCDEF, 0])
def test_reference_member_zero_is_todays_noise_and_members_are_uncorrelated(seed):
    n = 65536
    e = np.arange(n)
    assert np.array_equal(ens.normal(seed, 3, 7, e, member=0), ref.normal(seed, 3, 7, e))
    assert np.array_equal(ens.normal(seed, 3, 7, e), ref.normal(seed, 3, 7, e))
    assert np.array_equal(ens.step_noise(seed, 2, (2, 1, 8, 8), sample_offset=3), ref.step_noise(seed, 2, (2, 1, 8, 8), sample_offset=3))
    z = [ens.normal(seed, 3, 7, e, member=m) for m in range(8)]
    worst = 0.0
    for a, b in itertools.combinations(range(8), 2):
        assert not np.array_equal(z[a], z[b])
        worst = max(worst, abs(float(np.corrcoef(z[a], z[b])[0, 1])))
    print(f"seed {seed:#x}: max pairwise |correlation| of members 0-7 over {n} elements = {worst:.4f}")
    assert worst < 5.0 / math.sqrt(n)                 # 0.0195: five standard errors of the correlation of independent normals
    # the member word is a counter word of its own: member m of image 3 is not image 3 + m, nor iteration 7 + m
    assert not np.array_equal(z[1], ens.normal(seed, 4, 7, e)) and not np.array_equal(z[1], ens.normal(seed, 3, 8, e))
    # the 32-bit word wraps like the others
    assert np.array_equal(ens.normal(seed, 3, 7, e[:64], member=(1 << 32) + 2), z[2][:64])


def test_reference_reduce_arithmetic():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 5, 3, 4)).astype(np.float32)
    mean, std = ens.reduce(x)
    assert mean.dtype == np.float32 and std.dtype == np.float32 and mean.shape == (2, 3, 4)
    assert np.allclose(mean, x.astype(np.float64).mean(axis=1), rtol=0, atol=1e-7)
    assert np.allclose(std, x.astype(np.float64).std(axis=1, ddof=1), rtol=1e-6, atol=0)
    x[:, :, 0, 0] = 0.3
    assert ens.reduce(x)[1][0, 0, 0] == 0.0                     # a constant pixel: every deviation is exactly zero
    assert ens.reduce(x[:, :1])[1] is None


# ------------------------------------------------------------------------------ 5. Python surface
def test_python_argument_rules_without_a_gpu():
    assert midd_amd.ensemble_reduce is not None and midd_amd.EnsembleResult._fields == ("mean", "std", "samples", "seed")
    x = torch.zeros(1, 1, 32, 32)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="deterministic sampler has no ensemble"):
        ddim.denoise_ensemble(x, inference_steps=2, members=4, seed=1)
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    for bad in (0, -1, 1.5, "4", True, 1 << 31):
        with pytest.raises(ValueError, match="members"):
            d.denoise_ensemble(x, inference_steps=2, members=bad, seed=1)
    for bad in (-1, 1 << 32, 0.5):
        with pytest.raises(ValueError, match="member"):
            d.denoise(x, inference_steps=2, seed=1, member=bad)
        with pytest.raises(ValueError, match="member"):
            midd_amd.step_noise(1, 2, (1, 1, 8, 8), member=bad)
        with pytest.raises(ValueError, match="member_offset"):
            d.denoise_ensemble(x, inference_steps=2, members=2, seed=1, member_offset=bad)
    with pytest.raises(ValueError, match="member"):
        d.denoise(x, inference_steps=2, member=-1)                        # judged even without a seed
    with pytest.raises(ValueError, match="pass seed"):
        d.denoise(x, inference_steps=2, member=2)
    with pytest.raises(ValueError, match=r"2\*\*32"):
        d.denoise_ensemble(x, inference_steps=2, members=2, seed=1, member_offset=(1 << 32) - 1)
    with pytest.raises(ValueError, match="max_batch"):
        d.denoise_ensemble(x, inference_steps=2, members=2, seed=1, max_batch=0)
    with pytest.raises(ValueError, match="seed"):
        d.denoise_ensemble(x, inference_steps=2, members=2, seed=-1)
    with pytest.raises(ValueError, match="sample_offset"):
        d.denoise_ensemble(x, inference_steps=2, members=2, seed=1, sample_offset=-1)
    # valid arguments, CPU tensors: never a silent fall-back
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.denoise_ensemble(x, inference_steps=2, members=2, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.denoise(x, inference_steps=2, seed=1, member=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.ensemble_reduce(torch.zeros(1, 2, 1, 8, 8))
    with pytest.raises(ValueError, match="members"):
        midd_amd.ensemble_reduce(torch.zeros(4, 8))


def test_cli_accepts_samples_and_std_out():
    import inspect
    from midd_amd import cli
    sig = inspect.signature(cli.denoise_image_diffusion).parameters
    assert sig["samples"].default is None and sig["std_out"].default is None
    for argv in (["--samples", "x"], ["--samples", "0"], ["--samples", "4", "--variant", "ddim"], ["--std-out", "s.npy"],
                 ["--samples", "1", "--std-out", "s.npy"]):
        with pytest.raises(SystemExit):
            cli.main(argv + ["--image", "nowhere.png"])
    with pytest.raises(ValueError, match="cddpm"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="ddim", samples=4)
    with pytest.raises(ValueError, match="std-out"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", samples=1, std_out="s.npy")


# ------------------------------------------------------------------------------ static: the kernels' ISA
@pytest.fixture(scope="module")
def pointwise_isa():
    text = isa_dump("out_conv.hip") + isa_dump("ensemble.hip")
    kernels = {}
    for m in re.finditer(r"^(_ZN4midd\w+):", text, re.M):
        end = text.index(".end_amdhsa_kernel", m.start())
        kernels[m.group(1)] = text[m.start():end]
    return kernels


def _descriptor(body, field):
    return int(re.search(r"\.amdhsa_" + field + r" (\d+)", body).group(1))


def _instructions(body):
    """Instruction count of a kernel body as tools/isa_count.py counts it."""
    n = 0
    for l in body.split("\n"):
        t = l.strip().split(" ")[0]
        if t and not t.startswith((".", ";", "_Z")) and not t.endswith(":"):
            n += 1
    return n


def test_out_conv_kernels_keep_their_recorded_shape(pointwise_isa):
    """profiles/step_noise_isa.txt, as numbers a test holds: the unseeded out_conv_kernel<IC> is what it was before the seeded
    twin and before the member word (1338 / 8043 instructions), all four kernels take 109 VGPRs and none has scratch.  The seeded
    kernel's own instruction count is recorded there too; it is the unseeded one that must not move."""
    recorded = {"ILi1E": 1338, "ILi0E": 8043}
    for ic, total in recorded.items():
        seeded = next(b for n, b in pointwise_isa.items() if "out_conv_seeded_kernel" + ic in n)
        plain = next(b for n, b in pointwise_isa.items() if "out_conv_kernel" + ic in n)
        for body in (seeded, plain):
            assert _descriptor(body, "private_segment_fixed_size") == 0 and "scratch_" not in body
            assert _descriptor(body, "next_free_vgpr") == 109
        assert _instructions(plain) == total, (ic, _instructions(plain))
        assert _instructions(seeded) > total


def test_both_out_conv_kernels_add_the_noise_term_as_one_fma(pointwise_isa):
    """A seeded run replays through the noise tensor bit for bit only if out_conv_seeded_kernel and out_conv_kernel round the
    term c3 * noise the same way.  hipcc contracts the unseeded kernel's multiply and add into one v_fmac_f32; the seeded kernel
    asks for the FMA explicitly.  Either kernel falling back to a separate multiply and add would break the replay."""
    for ic in ("ILi1E", "ILi0E"):
        seeded = next(b for n, b in pointwise_isa.items() if "out_conv_seeded_kernel" + ic in n)
        plain = next(b for n, b in pointwise_isa.items() if "out_conv_kernel" + ic in n)

        def ops(body):
            return [l.strip().split(" ")[0] for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";"))]
        s_ops, p_ops = ops(seeded), ops(plain)
        # seeded: the fused add feeds the final store (the clamp rides on it)
        last_store = max(i for i, o in enumerate(s_ops) if o == "global_store_dword")
        assert "v_fma_f32" in s_ops[last_store - 3:last_store], s_ops[last_store - 6:last_store + 1]
        # unseeded: noise load, wait, fused multiply-add
        hits = [i for i, o in enumerate(p_ops) if o == "global_load_dword" and p_ops[i + 1:i + 3] == ["s_waitcnt", "v_fmac_f32_e32"]]
        assert hits, ic


def test_reduce_kernel_rounds_every_product_before_it_is_added(pointwise_isa):
    """The fixed arithmetic has no fused multiply-add: inside the two member loops of either instantiation there are additions and
    multiplications only (hipcc contracts q += d * d into v_fmac_f64 unless told otherwise; the FMAs of the correctly rounded
    division and square root sit outside the loops)."""
    found = 0
    for name, body in pointwise_isa.items():
        if "ensemble_reduce_kernel" not in name:
            continue
        found += 1
        assert _descriptor(body, "private_segment_fixed_size") == 0
        lines = body.split("\n")
        loops = []
        for i, l in enumerate(lines):
            if "Inner Loop Header" in l:
                label = l.split(":")[0].strip()
                j = next(k for k in range(i + 1, len(lines)) if "s_cbranch" in lines[k] and label in lines[k])
                loops.append([x.strip().split(" ")[0] for x in lines[i + 1:j]])
        assert len(loops) == 2, name
        v = 4 if "ILi4E" in name else 1
        assert loops[0].count("v_add_f64") == v and loops[1].count("v_add_f64") == 2 * v and loops[1].count("v_mul_f64") == v, name
        for ops in loops:
            assert not [o for o in ops if "fma" in o], (name, ops)
    assert found == 2
