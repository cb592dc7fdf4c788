"""CPU-only: WHICH rule a batched sampler call reports when a call breaks two at once (include/midd.h: mi_denoise_ensemble,
mi_denoise_tiled, mi_denoise_tiled_ensemble, mi_denoise_slots).  One case per adjacent pair of each call's order of checks --
the argument rules in check_*_args order, no output, std_out with one member, the aliasing pairs in (i, j) order, the state
check -- on an unfinalized plan, so nothing reaches the GPU.  The rules themselves, one at a time, are judged in
test_ensemble_cpu.py, test_tiled_cpu.py, test_tiled_ensemble_cpu.py and test_slots_cpu.py."""
import ctypes as C

import numpy as np
import pytest

from midd_amd import UNetDiffusion, native

SMALL = dict(model_channels=16, time_emb_dim=64)
# non-null "device pointers", 1 MiB apart, for calls that must fail before anything reads them (every buffer below is < 1 MiB)
NOISY, MEAN, STD, SAMPLES, TILES = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000
FP = C.POINTER(C.c_float)
TAB = np.linspace(1e-4, 0.02, 50, dtype=np.float32)
IMG_BYTES = 2 * 90 * 70 * 4                                 # noisy / image_out / mean_out / std_out of the tiled cases (B 2, 90x70)


@pytest.fixture(scope="module")
def plan():
    """An unfinalized cddpm plan: every host-side rule can be checked on it, no GPU call can succeed."""
    lib = native.lib()
    c = UNetDiffusion(variant="cddpm", **SMALL).cfg
    cfg = native.UNetCfg()
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


def _reports(rc, first, never=()):
    """The call failed with MI_EINVAL, its message holds every word of `first` and none of `never` (the other broken rule)."""
    msg = native.lib().mi_last_error().decode()
    assert rc == -1, msg
    for w in first:
        assert w in msg, msg
    for w in never:
        assert w not in msg, msg


# ------------------------------------------------------------------------------ mi_denoise_ensemble
def _ensemble(plan, null_plan=False, noisy=NOISY, mean=MEAN, std=STD, samples=None, B=2, members=4, H=32, W=32, sample_offset=0,
              member_offset=0, pass_samples=16):
    return native.lib().mi_denoise_ensemble(None if null_plan else plan, noisy, mean, std, samples, B, members, H, W, None, 0,
                                            None, None, None, 50, 5, sample_offset, member_offset, pass_samples, 0, None, 0, None)


@pytest.mark.parametrize("kw,first,never", [
    (dict(null_plan=True, members=0), ["null plan"], ["members"]),
    (dict(members=0, member_offset=-1), ["members 0", "members >= 1"], ["member_offset"]),
    (dict(members=0, pass_samples=0), ["members 0"], ["pass_samples"]),
    (dict(member_offset=-1, pass_samples=0), ["member_offset -1"], ["pass_samples"]),
    (dict(member_offset=(1 << 32) - 3, pass_samples=0), ["member_offset + members <= 4294967296"], ["pass_samples"]),
    (dict(pass_samples=0, B=0), ["pass_samples >= 1"], ["B 0"]),
    (dict(B=65536, members=1 << 20), ["B 65536 outside [1, 65535]"], ["B * members"]),
    (dict(B=0, sample_offset=-2), ["B 0 outside [1, 65535]"], ["sample_offset"]),
    (dict(B=65535, members=1 << 20, sample_offset=-2), ["B * members", "2147483647"], ["sample_offset"]),
    (dict(sample_offset=-2, H=0), ["sample_offset -2"], ["bad image shape"]),
    (dict(H=0, mean=None, std=None), ["bad image shape"], ["no output"]),
    (dict(H=65536, W=65536, mean=None, std=None), ["2^32", "4294967296"], ["no output"]),
    (dict(mean=None, std=None, members=1), ["no output", "samples_out"], ["finalize"]),
    (dict(members=1, mean=NOISY), ["std_out needs members >= 2"], ["alias"]),
    (dict(mean=NOISY, std=NOISY + 4), ["noisy and mean_out alias"], ["std_out alias"]),                        # (0, 1) before (0, 2)
    (dict(std=NOISY, samples=NOISY), ["noisy and std_out alias"], ["samples_out alias"]),                      # (0, 2) before (0, 3)
    (dict(std=MEAN, samples=NOISY), ["noisy and samples_out alias"], ["std_out alias"]),                       # (0, 3) before (1, 2)
    (dict(std=MEAN, samples=MEAN + 4), ["mean_out and std_out alias"], ["samples_out alias"]),                 # (1, 2) before (1, 3)
    (dict(std=MEAN + 8192, samples=MEAN + 4), ["mean_out and samples_out alias"], ["std_out and samples_out alias"]),      # (1, 3) before (2, 3): std_out follows mean_out, samples_out runs over both
])
def test_ensemble_reports_the_first_broken_rule(plan, kw, first, never):
    _reports(_ensemble(plan, **kw), first, never)


def test_ensemble_alias_message_and_state_check(plan):
    lib = native.lib()
    assert _ensemble(plan, mean=NOISY) == -1
    assert lib.mi_last_error().decode() == ("noisy and mean_out alias (overlap): noisy is read every step and the reduce reads "
                                            "samples_out while it writes mean_out and std_out")
    assert _ensemble(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _ensemble(plan, noisy=None, samples=SAMPLES) == -2      # a null noisy is judged after the state


# ------------------------------------------------------------------------------ mi_denoise_tiled
def _tiled(plan, null_plan=False, noisy=NOISY, image=MEAN, tiles=None, B=2, H=90, W=70, th=32, tw=32, oy=8, ox=8, seeded=1,
           sample_offset=0, pass_samples=16):
    return native.lib().mi_denoise_tiled(None if null_plan else plan, noisy, image, tiles, B, H, W, th, tw, oy, ox, None, 0,
                                         None, None, None, 50, seeded, 5, sample_offset, pass_samples, 0, None, 0, None)


@pytest.mark.parametrize("kw,first,never", [
    (dict(null_plan=True, th=36), ["null plan"], ["multiples"]),
    (dict(th=36, H=16), ["multiples of 8"], ["tile <= image"]),
    (dict(th=96, tw=72), ["tile height 96 exceeds the image height 90"], ["width"]),
    (dict(th=96, oy=-1), ["tile height 96 exceeds"], ["overlap"]),
    (dict(oy=17, tw=72), ["overlap 17 of tile height 32"], ["width"]),
    (dict(tw=72, ox=-1), ["tile width 72 exceeds the image width 70"], ["overlap"]),
    (dict(ox=17, pass_samples=0), ["overlap 17 of tile width 32"], ["pass_samples"]),
    (dict(H=92680, th=92680, oy=46340, pass_samples=0), ["overlap 46340x8", "overlap <= 46339"], ["pass_samples"]),
    (dict(pass_samples=0, sample_offset=-2), ["pass_samples >= 1"], ["sample_offset"]),
    (dict(sample_offset=-2, B=0), ["sample_offset -2"], ["B 0"]),
    (dict(H=65536, W=65536, B=0), ["2^32", "4294967296"], ["B 0"]),
    (dict(B=0, image=NOISY), ["B 0 must be positive"], ["alias"]),
    (dict(B=1 << 30, H=64, W=64, oy=0, ox=0, image=NOISY), ["B * tiles", "2147483647"], ["alias"]),
    (dict(image=NOISY, tiles=NOISY), ["noisy and image_out alias"], ["tiles_out"]),                            # (0, 1) before (0, 2)
    (dict(image=NOISY + IMG_BYTES, tiles=NOISY + 4), ["noisy and tiles_out alias"], ["image_out and tiles_out alias"]),      # (0, 2) before (1, 2): image_out follows noisy, tiles_out runs over both
])
def test_tiled_reports_the_first_broken_rule(plan, kw, first, never):
    _reports(_tiled(plan, **kw), first, never)


def test_tiled_alias_message_and_state_check(plan):
    lib = native.lib()
    assert _tiled(plan, tiles=MEAN + IMG_BYTES - 4) == -1
    assert lib.mi_last_error().decode() == ("image_out and tiles_out alias (overlap): noisy is read by every pass and the blend "
                                            "reads the tiles while it writes image_out")
    assert _tiled(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _tiled(plan, noisy=None, image=None, seeded=0) == -2      # null pointers are judged after the state


# ------------------------------------------------------------------------------ mi_denoise_tiled_ensemble
def _tiled_ensemble(plan, null_plan=False, noisy=NOISY, mean=MEAN, std=STD, samples=None, tiles=None, B=2, members=3, H=90, W=70,
                    th=32, tw=32, oy=8, ox=8, sample_offset=0, member_offset=0, pass_samples=16):
    return native.lib().mi_denoise_tiled_ensemble(
        None if null_plan else plan, noisy, mean, std, samples, tiles, B, members, H, W, th, tw, oy, ox, None, 0, None, None, None, 50,
        5, sample_offset, member_offset, pass_samples, 0, None, 0, None)


@pytest.mark.parametrize("kw,first,never", [
    (dict(null_plan=True, members=0), ["null plan"], ["members"]),
    (dict(th=36, members=0), ["multiples of 8"], ["members"]),                                                 # the tile rules come first
    (dict(pass_samples=0, members=0), ["pass_samples >= 1"], ["members"]),
    (dict(B=0, members=0), ["B 0 must be positive"], ["members"]),
    (dict(B=1 << 30, H=64, W=64, oy=0, ox=0, members=0), ["B * tiles", "2147483647"], ["members 0"]),
    (dict(members=0, member_offset=-1), ["members 0", "members >= 1"], ["member_offset"]),
    (dict(member_offset=-1, mean=None, std=None), ["member_offset -1"], ["no output"]),
    (dict(member_offset=(1 << 32) - 2, mean=None, std=None), ["member_offset + members <= 4294967296"], ["no output"]),
    # 2^20 images x 4 tiles x 2^10 members break the size rule; so do they with the last member words, which are judged first
    (dict(B=1 << 20, H=64, W=64, oy=0, ox=0, members=1 << 10, member_offset=(1 << 32) - 5), ["member_offset + members <= 4294967296"],
     ["B * members * tiles"]),
    (dict(B=1 << 20, H=64, W=64, oy=0, ox=0, members=1 << 10, mean=None, std=None), ["B * members * tiles"], ["no output"]),
    (dict(mean=None, std=None, members=1), ["no output", "tiles_out"], ["finalize"]),
    (dict(members=1, mean=NOISY), ["std_out needs members >= 2"], ["alias"]),
    (dict(mean=NOISY, std=NOISY + 4), ["noisy and mean_out alias"], ["std_out alias"]),                        # (0, 1) before (0, 2)
    (dict(std=NOISY, samples=NOISY), ["noisy and std_out alias"], ["samples_out alias"]),                      # (0, 2) before (0, 3)
    (dict(samples=NOISY, tiles=NOISY), ["noisy and samples_out alias"], ["tiles_out alias"]),                  # (0, 3) before (0, 4)
    (dict(tiles=NOISY + 4, std=MEAN), ["noisy and tiles_out alias"], ["std_out alias"]),                       # (0, 4) before (1, 2)
    (dict(std=MEAN, samples=MEAN + 4), ["mean_out and std_out alias"], ["samples_out alias"]),                 # (1, 2) before (1, 3)
    (dict(samples=MEAN + 4, tiles=MEAN + 8), ["mean_out and samples_out alias"], ["tiles_out alias"]),         # (1, 3) before (1, 4)
    (dict(tiles=MEAN - 4, samples=STD + 8), ["mean_out and tiles_out alias"], ["samples_out alias"]),          # (1, 4) before (2, 3)
    (dict(samples=STD + 8, tiles=STD + 16), ["std_out and samples_out alias"], ["tiles_out alias"]),           # (2, 3) before (2, 4)
    (dict(samples=STD + IMG_BYTES, tiles=STD + 8), ["std_out and tiles_out alias"], ["samples_out and tiles_out alias"]),      # (2, 4) before (3, 4): samples_out follows std_out, tiles_out runs over both
])
def test_tiled_ensemble_reports_the_first_broken_rule(plan, kw, first, never):
    _reports(_tiled_ensemble(plan, **kw), first, never)


def test_tiled_ensemble_alias_message_and_state_check(plan):
    lib = native.lib()
    assert _tiled_ensemble(plan, samples=SAMPLES, tiles=SAMPLES + 3 * IMG_BYTES - 4) == -1
    assert lib.mi_last_error().decode() == ("samples_out and tiles_out alias (overlap): noisy is read by every pass and the reduce "
                                            "reads the tiles while it writes mean_out, std_out and samples_out")
    assert _tiled_ensemble(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _tiled_ensemble(plan, noisy=None, mean=None, std=None, tiles=TILES) == -2      # a null noisy is judged after the state


# ------------------------------------------------------------------------------ mi_denoise_slots
def _slots(plan, null_plan=False, cond=NOISY, x=MEAN, B=2, H=32, W=32, rows=((40, 40), (20, 20), (0, 0)), n_rows=None, iter_base=None,
           sample_index=None, noise_steps=50, step_noise=None, seeded=1, tables=True):
    t = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
    ib = None if iter_base is None else (C.c_int32 * len(iter_base))(*iter_base)
    si = None if sample_index is None else (C.c_int64 * len(sample_index))(*sample_index)
    tab = TAB.ctypes.data_as(FP) if tables else None
    return native.lib().mi_denoise_slots(None if null_plan else plan, cond, x, B, H, W, t.ctypes.data_as(C.POINTER(C.c_int32)),
                                         len(rows) if n_rows is None else n_rows, ib, si, tab, tab, tab, noise_steps, step_noise,
                                         seeded, 5, 0, None, 0, None)


@pytest.mark.parametrize("kw,first,never", [
    (dict(null_plan=True, cond=None), ["null plan"], ["argument"]),
    (dict(tables=False, n_rows=-1), ["null argument"], ["n_rows"]),
    (dict(n_rows=-1, B=0), ["n_rows -1", "n_rows >= 0"], ["bad shape"]),
    (dict(H=0, noise_steps=0), ["bad shape B 2, 0x32"], ["noise_steps"]),
    (dict(noise_steps=0, iter_base=(-1, 0)), ["noise_steps 0", "noise_steps >= 1"], ["t_rows", "iter_base"]),
    (dict(rows=((40, 50), (20, 20)), step_noise=SAMPLES), ["t_rows[0][1]=50", "[-1,50)"], ["seeded together"]),
    (dict(rows=((50, 40), (20, 20)), iter_base=(-1, 0)), ["t_rows[0][0]=50"], ["iter_base"]),                  # a slot's rows before its iter_base
    (dict(iter_base=(-1, 0), sample_index=(-4, 0)), ["iter_base[0]=-1"], ["sample_index"]),
    (dict(sample_index=(-4, 0), rows=((40, 50), (20, 20))), ["sample_index[0]=-4"], ["t_rows"]),               # slot 0 before slot 1
    (dict(sample_index=(0, -4), step_noise=SAMPLES), ["sample_index[1]=-4"], ["seeded together"]),
    (dict(step_noise=SAMPLES, H=65536, W=65536), ["seeded together with step_noise"], ["2^32"]),
    (dict(H=65536, W=65536, x=NOISY), ["2^32", "4294967296"], ["alias"]),
    (dict(x=NOISY + 4), ["x and cond alias (overlap)"], ["finalize"]),
])
def test_slots_reports_the_first_broken_rule(plan, kw, first, never):
    _reports(_slots(plan, **kw), first, never)


def test_slots_state_check_comes_last(plan):
    lib = native.lib()
    assert _slots(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _slots(plan, noise_steps=2000, rows=((1500, 40),)) == -2      # the time table's rows are judged after the state
