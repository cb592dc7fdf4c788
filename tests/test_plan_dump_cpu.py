"""Host-only checks of the planner through `mi_debug_plan_dump` (no GPU, no finalize): which kernel instantiations, tiles, ring depths
and key splits the plans of the BASELINE.json shapes reach -- the inventory VERDICT r3 item 1a asked for, kept as a test so that a
planner change that moves a shipped configuration onto an instantiation no GPU test exercises is noticed on the CPU."""
import re
import sys
import os

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import plan_dump as pd

RANGE_KW = dict(model_channels=32, channel_mult=(1, 2), num_res_blocks=2, attention_resolutions=(1,), time_emb_dim=32)


def launches(kw, B, H, W, side, compute="f16x3"):
    text = pd.dump(pd.make_plan(kw, compute), B, H, W, side)
    rows = []
    for line in text.splitlines()[1:]:
        m = re.search(r"\| (midd::[^|]+?)\s*(?:\| grid (\d+)x(\d+) wgs/img (\d+) tiles (\d+)x(\d+) ring (\d+) ppw (\d+) apw (\d+) lds (\d+))?$", line)
        assert m, line
        rows.append(dict(line=line, kernel=m.group(1).strip(), ring=int(m.group(7)) if m.group(7) else None,
                         lds=int(m.group(10)) if m.group(10) else None, grid=(int(m.group(2)), int(m.group(3))) if m.group(2) else None))
    return text, rows


def test_default_network_launch_list_and_instantiations():
    """configs[1]: two sub-batch programs of 4 at 256x256 -- 73 launches each, and only these 3x3 instantiations."""
    text, rows = launches({}, 4, 256, 256, side=1)
    assert len(rows) == 73 and "ops=73" in text
    conv3 = sorted({r["kernel"] for r in rows if "conv_mfma_f16x3_kernel" in r["kernel"]})
    assert conv3 == sorted([
        "midd::conv_mfma_f16x3_kernel<3, 1, 16, 1, 3, 4, 1, false, 0>", "midd::conv_mfma_f16x3_kernel<3, 1, 16, 1, 3, 4, 1, true, 0>",
        "midd::conv_mfma_f16x3_kernel<3, 1, 16, 2, 3, 4, 1, false, 0>", "midd::conv_mfma_f16x3_kernel<3, 1, 16, 2, 3, 4, 1, true, 0>",
        "midd::conv_mfma_f16x3_kernel<3, 2, 16, 1, 3, 4, 1, false, 0>", "midd::conv_mfma_f16x3_kernel<3, 2, 16, 2, 3, 4, 1, false, 0>"]), conv3
    assert sum("attention_f16x3_kernel<96>" in r["kernel"] for r in rows) == 6
    # side-by-side programs keep every workgroup at three per CU (<= 53 KB) except the stride-2 tiles (one per CU)
    for r in rows:
        if r["lds"] is not None and "<3, 2," not in r["kernel"] and "conv_mfma" in r["kernel"]:
            assert r["lds"] <= 53 * 1024 + 512, r["line"]


def test_shipped_configurations_never_take_a_two_slot_ring():
    """The three 3x3 tiles with a two-slot weight ring and MT = 1 had their res-phase wait one step short until round 4
    (tests/test_dma_protocol_cpu.py); no plan of the default network -- any BASELINE batch / size, alone or side by side -- takes a
    two-slot ring at all (the GPU test `test_two_slot_ring_tiles_...` reaches them through a many-tiny-images shape)."""
    for B, S, side in [(1, 256, 0), (4, 256, 1), (8, 256, 0), (16, 256, 1), (32, 256, 0), (4, 512, 1), (8, 512, 0), (1, 512, 0), (2, 64, 1), (1, 64, 0)]:
        _, rows = launches({}, B, S, S, side)
        assert all(r["ring"] is None or r["ring"] == 0 or r["ring"] >= 4 for r in rows), (B, S, side, [r["line"] for r in rows if r["ring"] in (2, 3)])


def test_red_case_of_round_3_plan():
    """GPUTEST_r03's failing call: B = 4, 104x96 on the 32-channel topology runs two B = 2 programs -- every 3x3 on the 32-pixel two-wave
    tile (8,1,2,2,1) with ONE tile per workgroup, folded res_conv at 1 / 2 / 4 steps, key split 4 x 20 tiles, in_conv1_kernel (the kernel
    the defect was in: DESIGN.md section 2a)."""
    text, rows = launches(RANGE_KW, 2, 104, 96, side=1)
    assert "stat_rep=7" in text and "persist_wgs=640" in text
    k3 = {r["kernel"] for r in rows if "conv_mfma_f16x3_kernel<3, 1" in r["kernel"]}
    assert k3 == {"midd::conv_mfma_f16x3_kernel<3, 1, 8, 1, 2, 2, 1, false, 0>", "midd::conv_mfma_f16x3_kernel<3, 1, 8, 1, 2, 2, 1, true, 0>"}
    assert rows[0]["kernel"] == "midd::in_conv1_kernel"
    assert {int(v) for v in re.findall(r"res_steps(\d+)", text)} == {0, 1, 2, 4}
    assert "ksplit4 tps20" in text
    first = next(r for r in rows if "conv_mfma" in r["kernel"])
    assert first["grid"] == (624, 1) and "tiles 12x26" in first["line"] and "wgs/img 312" in first["line"]


WIDE_3X3 = re.compile(r"midd::conv_mfma_f16x3_kernel<3, 1, 16, [12], 3, 4, 1, (?:false|true), 2>$")


def test_unfinalized_run_alone_plan_lists_the_wide_instantiations():
    """Whether a 3x3 has a wide-chunk weight copy follows from the plan (f16x3, Cin >= 32), not from finalize having packed it: the
    dump of a plan that was never finalized shows the wide launches the finalized plan makes
    (tests/test_gpu_parity_r2.py::test_finalized_plan_dumps_as_the_unfinalized_plan ties the two on the GPU, where the counts were
    checked against the finalized parent build).  Side-by-side and batch-invariant programs take none."""
    def wide(B, side, invariant=False):
        text = pd.dump(pd.make_plan({}, "f16x3", batch_invariant=invariant), B, 256, 256, side)
        assert f"wide={int(not side and not invariant)}" in text.splitlines()[0]
        return [l for l in text.splitlines()[1:] if WIDE_3X3.search(l.split(" | ")[1])]
    alone = wide(1, 0)
    assert len(alone) == 24 and len(wide(8, 0)) == 23
    assert wide(4, 1) == [] and wide(1, 0, invariant=True) == [] and wide(8, 0, invariant=True) == []
    for line in alone:      # Cin >= 32, grid within MIDD_WIDE_MAX_WGS, and the ring the wide tiles have
        m = re.search(r" c(\d+)\+(\d+)->.*\| grid (\d+)x(\d+) .* ring (\d+) ", line)
        assert int(m.group(1)) + int(m.group(2)) >= 32 and int(m.group(3)) * int(m.group(4)) <= 512 and int(m.group(5)) in (4, 6), line


# (ring, ppw, apw, lds bytes) of every tile of MIDD_CONV16_TILES as the 3x3, the 3x3 stride-2 and the general 1x1 kernel, and of
# the two wide tiles: recorded from the library before the geometry was written down once (Conv16Tile, conv_mfma_f16x3.hip)
GEOMETRY = {
    (16, 2, 3, 4, 1): ((4, 2, 3, 53248), (6, 2, 9, 114496), (2, 2, 4, 49920)),
    (16, 1, 3, 4, 1): ((5, 2, 2, 50688), (6, 2, 5, 81216), (5, 2, 2, 51968)),
    (8, 1, 3, 2, 1): ((6, 3, 2, 48896), (6, 3, 5, 60992), (6, 3, 2, 49152)),
    (16, 2, 3, 2, 2): ((2, 3, 2, 44736), (6, 3, 5, 118272), (2, 3, 2, 46016)),
    (16, 1, 3, 2, 2): ((2, 3, 2, 42432), (6, 3, 3, 101632), (3, 3, 1, 50112)),
    (8, 1, 3, 1, 2): ((3, 6, 2, 47808), (6, 6, 3, 89600), (3, 6, 1, 45248)),
    (16, 2, 3, 1, 3): ((2, 6, 2, 52480), (5, 6, 4, 119872), (2, 6, 2, 51968)),
    (8, 1, 3, 1, 3): ((2, 6, 1, 47360), (5, 6, 2, 108608), (2, 6, 1, 46848)),
    (16, 2, 3, 1, 4): ((2, 6, 2, 67392), (3, 6, 3, 102016), (2, 6, 1, 62784)),
    (8, 2, 3, 1, 4): ((2, 6, 1, 62528), (3, 6, 3, 101248), (2, 6, 1, 62784)),
    (8, 1, 3, 1, 4): ((2, 6, 1, 61248), (4, 6, 2, 117376), (2, 6, 1, 60736)),
    (16, 2, 2, 4, 1): ((6, 1, 3, 52672), (6, 1, 9, 101632), (3, 1, 4, 49344)),
    (8, 1, 2, 2, 1): ((6, 2, 2, 36288), (6, 2, 5, 48384), (6, 2, 2, 36544)),
    (16, 2, 2, 2, 2): ((4, 2, 2, 52288), (6, 2, 5, 93056), (3, 2, 2, 45376)),
    (8, 1, 2, 1, 2): ((5, 4, 2, 51520), (6, 4, 3, 64640), (5, 4, 1, 48960)),
    (16, 2, 1, 4, 1): ((6, 1, 3, 39808), (6, 1, 9, 88768), (6, 1, 4, 48768)),
    (8, 1, 1, 2, 1): ((6, 1, 2, 23680), (6, 1, 5, 35776), (6, 1, 2, 23936)),
}
GEOMETRY_WIDE = {(16, 1, 3, 4, 1): (6, 2, 4, 71936), (16, 2, 3, 4, 1): (4, 2, 6, 77056)}


def test_conv16_geometry_of_every_instantiated_tile():
    import ctypes as C
    lib = pd.native.lib()

    def geometry(ks, stride, tile, cb):
        out = [C.c_int() for _ in range(4)]
        rc = lib.mi_debug_conv16_geometry(ks, stride, *tile, cb, *[C.byref(v) for v in out])
        return None if rc else tuple(v.value for v in out)
    for tile, want in GEOMETRY.items():
        assert (geometry(3, 1, tile, 0), geometry(3, 2, tile, 0), geometry(1, 1, tile, 0)) == want, tile
    for tile, want in GEOMETRY_WIDE.items():
        assert geometry(3, 1, tile, 2) == want, tile
    # what conv16_launch does not instantiate is reported as such: an unlisted tile, a wide variant of another tile, a 5x5
    assert geometry(3, 1, (16, 4, 3, 4, 1), 0) is None and b"not instantiated" in lib.mi_last_error()
    assert geometry(3, 1, (8, 1, 3, 2, 1), 2) is None and geometry(5, 1, (16, 2, 3, 4, 1), 0) is None
