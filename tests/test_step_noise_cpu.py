"""CPU-only checks of the seeded step noise (include/midd.h: mi_denoise_seeded, mi_step_noise_fill): the numpy restatement of
the specification against the Random123 known answers, the C ABI's declarations and limits, the Python argument rules, and
`denoise_sharded(pass_offset=True)` under a two-rank gloo group.  The device's values are judged in test_gpu_step_noise.py."""
import ctypes as C
import math
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import midd_loader  # the spawned workers import this module without conftest.py

midd_loader.load()
import midd_amd  # noqa: E402
from midd_amd import DiffusionDenoiser, UNetDiffusion, native  # noqa: E402
from tests import step_noise_reference as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)


# ------------------------------------------------------------------------------ the specification itself
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_numpy_philox_reproduces_the_random123_known_answers(counter, key, want):
    got = ref.philox4x32_10(counter, key)
    assert " ".join(f"{int(v):08x}" for v in got) == want


def test_reference_normals_are_bounded_and_keyed_by_every_counter_word():
    e = np.arange(4096)
    z = ref.normal(0x1234567890ABCDEF, 3, 7, e)
    assert np.isfinite(z).all() and np.abs(z).max() <= math.sqrt(2 * 24 * math.log(2)) + 1e-12      # u1 >= 2^-24: |z| <= 5.77
    for other in (ref.normal(0x1234567890ABCDEF, 4, 7, e), ref.normal(0x1234567890ABCDEF, 3, 8, e),
                  ref.normal(0x1234567890ABCDEE, 3, 7, e), ref.normal(0x0234567890ABCDEF, 3, 7, e), ref.normal(0x1234567890ABCDEF, 3, 7, e + 1)):
        assert not np.array_equal(z, other)
    full = ref.step_noise(0x1234567890ABCDEF, 2, (2, 1, 4, 8), sample_offset=3)
    assert np.array_equal(full[1, 0].ravel(), 0.5 * ref.normal(0x1234567890ABCDEF, 3, 1, np.arange(32)))
    assert np.array_equal(full[0, 1].ravel(), 0.5 * ref.normal(0x1234567890ABCDEF, 4, 0, np.arange(32)))


# ------------------------------------------------------------------------------ C ABI
def test_header_declares_and_library_exports_the_seeded_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n: a for n, _, a in native.SYMBOLS}
    assert {"mi_denoise_seeded", "mi_step_noise_fill"} <= declared and declared == set(bound)
    lib = native.lib()
    assert lib.mi_denoise_seeded is not None and lib.mi_step_noise_fill is not None
    # mi_denoise_seeded is mi_denoise with (seed, sample_offset) in the place of the noise pointer
    plain, seeded = bound["mi_denoise"], bound["mi_denoise_seeded"]
    at = plain.index(C.c_void_p, 12)
    assert seeded == plain[:at] + [C.c_uint64, C.c_int64] + plain[at + 1:]
    # the specification's constants are in the header, not left to the implementation
    for word in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "cospif", "2^-24"):
        assert word in header, word


def test_fill_refuses_what_the_counter_cannot_hold_without_a_gpu():
    lib = native.lib()
    assert lib.mi_step_noise_fill(None, 1, 1, 1, 8, 8, 1, -1, None) == -1
    assert b"sample_offset" in lib.mi_last_error()
    assert lib.mi_step_noise_fill(None, 1, 1, 1, 65536, 65536, 1, 0, None) == -1            # C*H*W == 2^32
    assert b"2^32" in lib.mi_last_error() and b"4294967296" in lib.mi_last_error()
    assert lib.mi_step_noise_fill(None, 1, 1, 4, 2 ** 30, 2 ** 30, 1, 0, None) == -1         # (a product that overflows 64 bits too)
    assert lib.mi_step_noise_fill(None, 1, 1, 1, 65536, 65535, 1, 0, None) == -1             # in range, but no destination
    assert b"null" in lib.mi_last_error()
    assert lib.mi_step_noise_fill(None, 0, 4, 1, 8, 8, 1, 0, None) == 0                      # nothing to write


def test_denoise_seeded_checks_the_offset_before_any_gpu_work():
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
    cfg.time_emb_dim, cfg.variant = c.time_emb_dim, native.MI_VARIANT["cddpm"]
    h = C.c_void_p()
    native.check(lib.mi_unet_plan_create(C.byref(cfg), C.byref(h)))
    args = (None, None, 2, 32, 32, None, 0, None, None, None, 50)
    assert lib.mi_denoise_seeded(h, *args, 5, -3, 0, None, 0, None) == -1
    assert b"sample_offset -3" in lib.mi_last_error()
    assert lib.mi_denoise_seeded(h, None, None, 2, 65536, 65536, None, 0, None, None, None, 50, 5, 0, 0, None, 0, None) == -1
    assert b"2^32" in lib.mi_last_error()
    assert lib.mi_denoise_seeded(None, *args, 5, 0, 0, None, 0, None) == -1
    lib.mi_plan_destroy(h)


# ------------------------------------------------------------------------------ Python surface
def test_seed_arguments_are_validated_without_a_gpu():
    assert midd_amd.step_noise is not None
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    x = torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError, match="either seed"):
        d.denoise(x, inference_steps=2, seed=1, step_noise=torch.zeros(2, 1, 1, 32, 32))
    with pytest.raises(ValueError, match="either seed"):
        d.model.run_sampler(x, [1, 0], d.beta, d.alpha, d.alpha_hat, clamp_eps=False, seed=1, step_noise=torch.zeros(2, 1, 1, 32, 32))
    for bad in (-1, 1 << 64, 1.5, "7", True):
        with pytest.raises(ValueError, match="seed"):
            d.denoise(x, inference_steps=2, seed=bad)
    for bad in (-1, 1 << 63, 0.5):
        with pytest.raises(ValueError, match="sample_offset"):
            d.denoise(x, inference_steps=2, seed=1, sample_offset=bad)
        with pytest.raises(ValueError, match="sample_offset"):
            midd_amd.step_noise(1, 2, (1, 1, 8, 8), sample_offset=bad)
    with pytest.raises(ValueError, match="shape"):
        midd_amd.step_noise(1, 2, (1, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # valid arguments, CPU tensor: never a silent fall-back
        d.denoise(x, inference_steps=2, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        midd_amd.step_noise(1, 2, (1, 1, 8, 8), device="cpu")


def test_cli_accepts_a_seed():
    import inspect
    from midd_amd import cli
    assert inspect.signature(cli.denoise_image_diffusion).parameters["seed"].default is None
    with pytest.raises(SystemExit):
        cli.main(["--seed", "x", "--image", "nowhere.png"])


# ------------------------------------------------------------------------------ sharding
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _per_image(x, sample_offset):
    """Stands in for a seeded denoise(): per sample, and a function of the sample's GLOBAL index."""
    idx = torch.arange(sample_offset, sample_offset + x.shape[0], dtype=x.dtype).view(-1, 1, 1, 1)
    return x * 0.5 + idx


def _worker(rank, world, port, out_dir):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import midd_loader
    midd_loader.load()
    from midd_amd.sharding import denoise_sharded
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    full = torch.rand(8, 1, 16, 16, generator=torch.Generator().manual_seed(0))
    seen = []

    def fn(x, sample_offset):
        seen.append((x.shape[0], sample_offset))
        return _per_image(x, sample_offset)

    got = denoise_sharded(fn, full, pass_offset=True)
    assert seen == [(4, 4 * rank)], seen
    plain = denoise_sharded(lambda x: x * 0.5, full)              # the default call still passes the images alone
    torch.save((got, plain), os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_pass_offset_hands_every_rank_its_first_global_index(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    full = torch.rand(8, 1, 16, 16, generator=torch.Generator().manual_seed(0))
    for r in range(world):
        got, plain = torch.load(os.path.join(tmp_path, f"r{r}.pt"))
        assert torch.equal(got, _per_image(full, 0)), r           # sharded == single process
        assert torch.equal(plain, full * 0.5), r


def test_pass_offset_without_a_process_group():
    from midd_amd.sharding import denoise_sharded
    full = torch.rand(4, 1, 8, 8)
    assert torch.equal(denoise_sharded(_per_image, full, pass_offset=True), _per_image(full, 0))
    assert torch.equal(denoise_sharded(lambda x: x + 1, full), full + 1)
