"""CPU-only checks of networks with more than one image channel (`in_channels` 2..4; what the device computes with them is judged in
tests/test_gpu_multichannel.py):

  * the widths such a network may have.  in_conv_kernel and the out_conv kernels keep their weights in LDS and neither raises its
    limit, so (in_channels, model_channels) and (in_channels, model_channels * channel_mult[0]) are bounded by 64 KB per workgroup.
    mi_unet_plan_create refuses what the launch would refuse, naming the limit -- the byte counts are restated here from the kernels'
    LDS layout (in_conv.hip, out_conv_body.h), independently of the library's own functions (midd_internal.h);
  * the workspace sizes grow by the documented C * H * W terms;
  * the 2^32 element-index rule of the seeded step noise counts C * H * W, not H * W.
"""
import ctypes as C
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plan_dump as pd
from midd_amd import native
from tests import tiled_reference

LIMIT = 64 * 1024
STAT_BYTES = 6 * 8                    # stats_common.h: STAT_WORDS = 2 sums x 3 limbs of 8 bytes per channel
HEAD_DIMS = (32, 64, 96, 128)         # attention runs on 2 heads of these sizes: the last level has 64, 128, 192 or 256 channels


def in_conv_bytes(ic, cout):
    """in_conv_kernel: weights [9][2 ic][Cout] + bias [Cout], the statistics scratch [2][Cout][256 // (Cout / 16) pixel lanes] and
    2 floats of alignment slack, then (Cout + 2) publish accumulators."""
    ppi = 256 // (cout // 16)
    return (9 * 2 * ic * cout + cout + 2 * cout * ppi + 2) * 4 + (cout + 2) * STAT_BYTES


def out_conv_bytes(ic, c):
    """out_conv_*_kernel: the static 18 x 18 halo tile of 16 channels at a pixel stride of 20 floats, weights [ic][9][C], scale / shift [2][C]."""
    return 18 * 18 * 20 * 4 + (ic * 9 * c + 2 * c) * 4


def _create(kw, variant="cddpm"):
    """(plan or None, message)."""
    try:
        return pd.make_plan(kw, variant=variant), ""
    except native.MiddError as e:
        assert e.code == -1, e                                    # MI_EINVAL: judged by mi_unet_plan_create, before any launch
        return None, str(e)


def _kw_for_width(ic, mc):
    """A two-level topology of width mc whose last level has a channel count the attention kernels take, or None."""
    for m in range(1, 17):
        if mc * m // 2 in HEAD_DIMS and (mc * m) % 2 == 0:
            return dict(in_channels=ic, model_channels=mc, channel_mult=(1, m), num_res_blocks=1, attention_resolutions=(1,), time_emb_dim=32)
    return None


WIDEST_IN = {2: 160, 3: 112, 4: 96}      # by hand from in_conv_bytes: e.g. ic = 4, 96 -> 65 000 bytes, 112 -> 70 440
WIDEST_OUT = {2: 480, 3: 336, 4: 256}    # 25 920 + (36 ic + 8) C <= 65 536


@pytest.mark.parametrize("ic", [2, 3, 4])
def test_in_conv_width_limit(ic):
    lib = native.lib()
    widest = max(mc for mc in range(16, 1025, 16) if in_conv_bytes(ic, mc) <= LIMIT)
    assert widest == WIDEST_IN[ic]
    planned = []
    for mc in range(16, 513, 16):
        kw = _kw_for_width(ic, mc) or dict(in_channels=ic, model_channels=mc, channel_mult=(1, 1), num_res_blocks=1,
                                           attention_resolutions=(1,), time_emb_dim=32)
        plan, msg = _create(kw)
        if in_conv_bytes(ic, mc) > LIMIT:
            assert plan is None, (ic, mc)
            assert f"in_channels {ic}" in msg and f"model_channels {mc}" in msg and "in_conv" in msg and "LDS" in msg, msg
            assert f"{in_conv_bytes(ic, mc)} bytes" in msg and f"limit is {LIMIT} bytes" in msg, msg
        elif _kw_for_width(ic, mc) is None:
            assert plan is None and "head_dim" in msg and "LDS" not in msg, (ic, mc, msg)      # another rule's business
        else:
            assert plan is not None, (ic, mc, msg)
            text = pd.dump(plan, 2, 40, 24, 0)                   # plans, and on the general kernels
            assert "midd::in_conv_kernel" in text and "midd::out_conv_kernel<0>" in text
            planned.append(mc)
            lib.mi_plan_destroy(plan)
    # the widest width a topology can have under both rules plans; the first multiple of 16 beyond the LDS limit is refused (above)
    assert planned[-1] == max(mc for mc in range(16, widest + 1, 16) if _kw_for_width(ic, mc))
    assert in_conv_bytes(ic, widest + 16) > LIMIT
    print(f"in_channels {ic}: in_conv fits up to model_channels {widest} ({in_conv_bytes(ic, widest)} bytes), planned widths {planned}")


@pytest.mark.parametrize("ic", [2, 3, 4])
def test_out_conv_width_limit(ic):
    """model_channels 16 with channel_mult (m, 4): out_conv reads 16 m channels, the last level has 64."""
    lib = native.lib()
    widest = max(c for c in range(16, 2049, 16) if out_conv_bytes(ic, c) <= LIMIT)
    assert widest == WIDEST_OUT[ic]
    for c in (widest, widest + 16):
        kw = dict(in_channels=ic, model_channels=16, channel_mult=(c // 16, 4), num_res_blocks=1, attention_resolutions=(1,), time_emb_dim=32)
        plan, msg = _create(kw, variant="cddpm")
        if c == widest:
            assert plan is not None, msg
            assert "midd::out_conv_kernel<0>" in pd.dump(plan, 1, 16, 16, 0)
            lib.mi_plan_destroy(plan)
        else:
            assert plan is None
            assert f"in_channels {ic}" in msg and f"{c} channels" in msg and "out_conv" in msg and f"{LIMIT} bytes" in msg, msg


def test_one_channel_keeps_its_widths():
    """in_channels = 1: every width the attention rule leaves (model_channels divides 64, 128, 192 or 256) plans as before -- 32, 48
    and 64 on in_conv1_kernel, which sizes its own LDS; the others on in_conv_kernel, where 256 takes 64 616 bytes."""
    lib = native.lib()
    assert in_conv_bytes(1, 256) <= LIMIT < in_conv_bytes(1, 272)
    got = {}
    for mc in range(16, 273, 16):
        kw = _kw_for_width(1, mc)
        if kw is None:
            continue
        plan, msg = _create(kw)
        assert plan is not None, (mc, msg)
        got[mc] = len(pd.dump(plan, 1, 16, 16, 0).splitlines())
        lib.mi_plan_destroy(plan)
    assert sorted(got) == [16, 32, 48, 64, 96, 128, 192, 256]
    assert all(n > 10 for n in got.values()), got
    # the widest out_conv of one channel: 44 C + 25 920 <= 65 536
    assert out_conv_bytes(1, 896) <= LIMIT < out_conv_bytes(1, 912)
    for c, ok in ((896, True), (912, False)):
        plan, msg = _create(dict(model_channels=16, channel_mult=(c // 16, 4), num_res_blocks=1, attention_resolutions=(1,), time_emb_dim=32))
        assert (plan is not None) == ok, (c, msg)
        if plan is not None:
            lib.mi_plan_destroy(plan)


def test_the_issue_network_is_refused_at_plan_time():
    """in_channels = 4 at model_channels = 128 planned 33 launches and failed at the first of them (MI_EHIP)."""
    plan, msg = _create(dict(in_channels=4, model_channels=128, channel_mult=(1, 1), num_res_blocks=1, attention_resolutions=(1,), time_emb_dim=32))
    assert plan is None and "in_channels 4 with model_channels 128" in msg and "65536" in msg, msg


# ------------------------------------------------------------------------------ workspace sizes
TOPO = dict(model_channels=32, channel_mult=(1, 2), num_res_blocks=2, attention_resolutions=(1,), time_emb_dim=32)


def _program_bytes(plan, B, H, W):
    """What mi_workspace_bytes answers for the finalized plan, from the dump (tests/test_ensemble_cpu.py)."""
    def one(b, side):
        return int(re.search(r"bytes=(\d+)", pd.dump(plan, b, H, W, side)).group(1))
    need = one(B, 0)
    if B % 2 == 0 and B // 2 >= 2:
        need = max(need, 2 * one(B // 2, 1))
    return need


@pytest.mark.parametrize("ic", [1, 3])
def test_workspace_sizes_count_the_channels(ic):
    lib = native.lib()
    plan = pd.make_plan(dict(in_channels=ic, **TOPO), variant="cddpm")
    try:
        B, M, H, W, p = 2, 3, 40, 24, 4
        chw = ic * H * W
        ens = lib.mi_ensemble_workspace_bytes
        internal, ext = ens(plan, B, M, H, W, p, 0), ens(plan, B, M, H, W, p, 1)
        assert ext > 0 and internal - ext == B * M * chw * 4                                   # the members
        run = max(_program_bytes(plan, 4, H, W), _program_bytes(plan, 2, H, W))                # passes of 4 and a tail of 2
        assert run + p * chw * 4 <= ext <= run + p * chw * 4 + 512                              # a pass's condition images
        # the self-ensemble keeps its view outputs in the workspace whatever the flag: the ensemble's layout with views as members
        selfens = lib.mi_self_ensemble_workspace_bytes
        assert selfens(plan, B, 4, H, W, p, 0) == selfens(plan, B, 4, H, W, p, 1) == ens(plan, B, 4, H, W, p, 0)
        assert selfens(plan, B, 4, H, W, p, 0) - ens(plan, B, 4, H, W, p, 1) == B * 4 * chw * 4
        # tiles: 56 x 72 as 32 x 32 tiles with overlap 8 -> 2 x 3 tiles of C * 32 * 32
        Hi, Wi, T, O = 56, 72, 32, 8
        K = len(tiled_reference.origins(Hi, T, O)) * len(tiled_reference.origins(Wi, T, O))
        assert K == 6
        tiled = lib.mi_tiled_workspace_bytes
        t_int, t_ext = tiled(plan, B, Hi, Wi, T, T, O, O, p, 0), tiled(plan, B, Hi, Wi, T, T, O, O, p, 1)
        assert t_ext > 0 and t_int - t_ext == B * K * ic * T * T * 4
        assert t_ext == ens(plan, B, K, T, T, p, 1)
        te = lib.mi_tiled_ensemble_workspace_bytes
        e_int, e_ext = te(plan, B, M, Hi, Wi, T, T, O, O, p, 0), te(plan, B, M, Hi, Wi, T, T, O, O, p, 1)
        assert e_ext == t_ext and e_int - e_ext == M * B * K * ic * T * T * 4
    finally:
        lib.mi_plan_destroy(plan)


def test_sampler_workspace_grows_with_the_channels_by_the_image_buffers_only():
    """Same topology at C = 1 and C = 3: the activations do not depend on C, so the sampler's own workspace (mi_workspace_bytes, read
    from the plan dump: the call itself needs a finalized plan) differs by whole [B, C, H, W] image buffers and roundings at most."""
    lib = native.lib()
    B, H, W = 3, 40, 24
    plans = {ic: pd.make_plan(dict(in_channels=ic, **TOPO), variant="cddpm") for ic in (1, 3)}
    try:
        one, three = (_program_bytes(plans[ic], B, H, W) for ic in (1, 3))
        grow = three - one
        assert 0 <= grow <= 4 * (2 * B * H * W * 4) + 4096, (one, three)          # at most a handful of image buffers, 2 more channels each
    finally:
        for p in plans.values():
            lib.mi_plan_destroy(p)


# ------------------------------------------------------------------------------ the element index of the seeded noise
def test_step_noise_range_counts_the_channels():
    """C * H * W = 4 * 32768 * 32768 = 2^32 is refused, judged before anything is launched (a null destination is judged AFTER the
    range: the same call one channel down reaches it)."""
    lib = native.lib()
    side = 32768
    assert lib.mi_step_noise_fill(None, 1, 1, 4, side, side, 7, 0, None) == -1
    msg = lib.mi_last_error().decode()
    assert "C*H*W" in msg and f"4*{side}*{side}" in msg and "4294967296" in msg, msg
    for c in (1, 3):                                              # H * W alone is 2^30: these pass the range rule
        assert lib.mi_step_noise_fill(None, 1, 1, c, side, side, 7, 0, None) == -1
        assert "null" in lib.mi_last_error().decode()
    assert lib.mi_step_noise_fill(None, 1, 1, 4, side, side - 1, 7, 0, None) == -1 and "null" in lib.mi_last_error().decode()
    assert lib.mi_step_noise_fill_member(None, 1, 1, 4, side, side, 7, 0, 2, None) == -1 and "C*H*W" in lib.mi_last_error().decode()
