"""The pair walk of the fp16-MFMA 3x3 kernel with 16-channel chunks (csrc/conv_mfma_f16x3_body.h: PAIR), on the CPU.

Two 16-channel chunks (c even, c + 1) of a tile take 4 + 5 K steps instead of 5 + 5: the first step of chunk c + 1 carries tap 8
of chunk c in its lower half.  An unpaired last chunk keeps 5 steps.  Two things are checked without a GPU:

* the step count per tile that the kernel and the weight packer share (`mi_debug_conv16_steps` = conv16_num_steps) is
  (nblk / 2) * 9 + (nblk & 1) * 5;
* a replay of one wave's program order with the new walk, in the style of tests/test_dma_protocol_cpu.py (its `Wave` queue model is
  reused): RING / PPW / APW come from the library, for every tile of MIDD_CONV16_TILES, and every counted wait is checked to be
    - no earlier than its data: the weight step multiplied has landed, the chunk transformed has landed, a ring slot is refilled
      only after the step that read it;
    - no more draining than the derived bound: a wait never forces an operation to complete that is younger than the one
      it waits for (the K steps' waits and the chunk-end wait are exact; the former chunk-end ladder `>= D, == 1, else 0` is shown
      to fail this for the 4-step chunk on a ring of five or six slots).
The chunk-end immediates are read from the kernel's text.  The register hand-over of tap 8 is not modelled here: the GPU tests
(tests/test_gpu_pair_walk.py) check it through the results.
"""
import itertools
import os
import re

import pytest

from midd_amd import native
from tests.test_dma_protocol_cpu import CSRC, Wave, geometry, instantiated_tiles

TAPS, HSTEPS = 9, 5


def steps_formula(cin):
    nblk = cin // 16
    return (nblk // 2) * 9 + (nblk & 1) * 5


@pytest.mark.parametrize("cin", [16, 32, 48, 96, 144, 192, 288, 384])
def test_step_count_per_tile(cin):
    lib = native.lib()
    assert lib.mi_debug_conv16_steps(cin, 3, 0) == steps_formula(cin)
    assert lib.mi_debug_conv16_steps(cin, 3, 1) == steps_formula(cin)
    # the other K orders are what they were: wide chunks 9 per pair + 5, the 1x1 one step per 32 channels
    assert lib.mi_debug_conv16_steps(cin, 3, 2) == (cin // 32) * 9 + (cin // 16 & 1) * 5
    assert lib.mi_debug_conv16_steps(cin, 1, 0) == (cin + 31) // 32


def test_step_counts_named_in_the_design():
    assert [steps_formula(c) for c in (48, 96, 192)] == [14, 27, 54]


def chunk_steps(nblk):
    """Steps of every chunk of a tile: pairs of 4 + 5, an unpaired last chunk 5."""
    return [4 if (c % 2 == 0 and c + 1 < nblk) else 5 for c in range(nblk)]


def kernel_chunk_end_arms():
    """The chunk-end ladder as conv_mfma_f16x3_body.h spells it: {after: k} for every arm `after == a -> cmin(k, D) * PPW`.
    The replay below waits with what the KERNEL TEXT says, not with a formula of its own: an arm that is missing there (the
    ladder then falls through to vmcnt(0)) or that names the wrong count fails the drain / landed checks."""
    src = open(os.path.join(CSRC, "conv_mfma_f16x3_body.h")).read()
    lad = src[src.index("if (after >= D) wait_vm_and_barrier<D * PPW>();"):]
    lad = lad[:lad.index("else wait_vm_and_barrier<0>();")]
    arms = {int(a): int(k) for a, k in re.findall(r"else if \(after == (\d+)\) wait_vm_and_barrier<cmin\((\d+), D\) \* PPW>\(\);", lad)}
    assert lad.count("wait_vm_and_barrier") == len(arms) + 1, "an arm of the ladder this test cannot read"
    return arms


ARMS = kernel_chunk_end_arms()


def chunk_end_wait(after, D, ppw, old_ladder=False):
    if old_ladder:
        return D * ppw if after >= D else ppw if after == 1 else 0
    if after >= D:
        return D * ppw
    return min(ARMS[after], D) * ppw if after in ARMS else 0


def test_the_kernels_ladder_has_an_arm_for_every_after_below_the_deepest_ring():
    assert ARMS == {1: 1, 2: 2, 3: 3, 4: 4}          # MIDD_RING_MAX 6: D <= 5


def replay(ring, ppw, apw, mt, nt, nblk, res_steps, tiles_per_wg, has_resid, old_ladder=False):
    """Program order of the pair-walk kernel for one wave.  Returns (largest immediate, number of chunk-end waits that drained
    something younger than the chunk they waited for)."""
    D = ring - 1
    RL, RG = 2 * mt, (2 if mt == 1 else 1)
    w = Wave()
    issued, consumed = [0], [0]
    drained = [0]

    def wait_for(n, needed):
        """vmcnt(n) that must cover `needed`: no earlier than the data, and nothing younger than it is forced to land."""
        if needed in w.q:
            last = len(w.q) - 1 - w.q[::-1].index(needed)
            # (a tile's output stores share the counter: the first steps after an epilogue wait for a few of them too, as
            # they always have; they are not what "draining the ring" is about and are left out of the bound)
            younger = sum(1 for op in w.q[last + 1:] if op != "store")
            assert n <= younger, f"vmcnt({n}) returns before {needed} has landed ({younger} operations are younger)"
            if n < younger:
                drained[0] += 1
        w.wait(n)

    def issue_w():
        k = issued[0]
        assert k - ring <= consumed[0] - 1, f"ring slot of W({k}) refilled before step {k - ring} was read"
        w.issue(("W", k), ppw)
        issued[0] += 1

    def mfma_step():
        assert w.landed(("W", consumed[0])), f"weights of step {consumed[0]} multiplied before they landed"
        consumed[0] += 1

    def k_step(with_a, issue_next_a, next_label):
        before = drained[0]
        wait_for((D - 1) * ppw + (apw if with_a else 0), ("W", consumed[0]))
        assert drained[0] == before, f"step {consumed[0]}: the step wait drains more than W({consumed[0]}) needs"
        issue_w()
        if issue_next_a:
            w.issue(next_label, apw)
        mfma_step()

    def res_phase():
        if res_steps == 0:
            return
        g = 0
        w.issue(("R", g), RG * RL)
        w.wait(0)
        for r in range(0, res_steps, RG):
            if r + RG < res_steps:
                w.issue(("R", g + 1), RG * RL)
                for i in range(RG):
                    if r + i < res_steps:
                        w.wait((D - 1) * ppw + (RG * RL if i < D else 0))
                        issue_w()
                        mfma_step()
                w.wait(RG * ppw)
                assert w.landed(("R", g + 1)), f"res operands of group {g + 1} split before they landed"
                g += 1
            else:
                for i in range(RG):
                    if r + i < res_steps:
                        w.wait((D - 1) * ppw)
                        issue_w()
                        mfma_step()

    def epilogue():
        if has_resid:
            w.issue("resid", mt * nt)
            w.wait(0)
        w.issue("store", mt * nt)

    steps_of = chunk_steps(nblk)
    assert sum(steps_of) == native.lib().mi_debug_conv16_steps(16 * nblk, 3, 0)
    w.issue(("A", 0, 0), apw)
    for _ in range(D):
        issue_w()
    w.wait(0)
    for tile in range(tiles_per_wg):
        has_next_tile = tile + 1 < tiles_per_wg
        for c, steps in enumerate(steps_of):
            more_in_tile = c + 1 < nblk
            more = more_in_tile or has_next_tile
            nxt = ("A", tile, c + 1) if more_in_tile else ("A", tile + 1, 0)
            assert w.landed(("A", tile, c)), f"chunk {c} of tile {tile} transformed before it landed"
            for j in range(steps):
                if more:
                    k_step(with_a=1 <= j <= D, issue_next_a=(j == 0), next_label=nxt)
                else:
                    k_step(False, False, None)
            if more:
                if not more_in_tile:
                    res_phase()
                after = steps - 1 + (0 if more_in_tile else res_steps)
                wait_for(chunk_end_wait(after, D, ppw, old_ladder), nxt)
                assert w.landed(nxt), f"{nxt} transformed before it landed (after={after}, D={D})"
                if not more_in_tile:
                    epilogue()
            else:
                res_phase()
    w.wait(0)
    epilogue()
    # the ring is cyclic over the tile's steps: every step of every tile was requested exactly once, in order
    assert consumed[0] == tiles_per_wg * (sum(steps_of) + res_steps)
    return w.max_imm, drained[0]


def pair_walk_geometries():
    out = []
    for tile in instantiated_tiles():
        for stride in (1, 2):
            geo = geometry(3, stride, tile, 0)
            if geo is not None:
                out.append((tile, stride) + geo[:3])
    assert len(out) >= 20
    return out


def test_every_counted_wait_of_the_pair_walk():
    checked, worst, rings = 0, 0, set()
    for tile, stride, ring, ppw, apw in pair_walk_geometries():
        _, mt, nt, _, _ = tile
        rings.add(ring)
        res_options = (0, 1, 2, 3, 6, 12) if stride == 1 else (0,)
        for nblk, res_steps, tiles_per_wg, has_resid in itertools.product((1, 2, 3, 4, 9, 24), res_options, (1, 2, 3), (False, True)):
            imm, drained = replay(ring, ppw, apw, mt, nt, nblk, res_steps, tiles_per_wg, has_resid)
            assert drained == 0, (tile, stride, nblk, res_steps, tiles_per_wg)
            worst = max(worst, imm)
            checked += 1
    assert checked > 3000 and worst <= 63
    assert {r for r in rings if r >= 5}, "no tile with a ring of five or more slots: the 4-step chunk's wait is not exercised"
    print(f"{checked} schedules replayed; ring depths {sorted(rings)}; largest vmcnt immediate {worst}")


def test_the_former_chunk_end_ladder_would_drain_the_ring():
    """The checker itself, and why the ladder changed: `after >= D / == 1 / else 0` waits with vmcnt(0) after a 4-step chunk
    (after = 3) on a ring with D = 4 or 5 steps in flight, forcing weight steps to land that the next chunk's transform does not
    need.  The model counts such waits; the derived min(after, D) * PPW has none."""
    deep = [g for g in pair_walk_geometries() if g[2] - 1 >= 4]
    assert deep
    for tile, stride, ring, ppw, apw in deep:
        _, mt, nt, _, _ = tile
        _, drained_old = replay(ring, ppw, apw, mt, nt, 4, 0, 1, False, old_ladder=True)
        _, drained_new = replay(ring, ppw, apw, mt, nt, 4, 0, 1, False)
        assert drained_old > 0 and drained_new == 0, (tile, stride, ring)


def test_the_model_catches_a_wait_that_is_too_permissive():
    """A chunk-end wait that counts one weight group too many returns before the next chunk's activations have landed."""
    tile, stride, ring, ppw, apw = next(g for g in pair_walk_geometries() if g[2] - 1 >= 4)
    D = ring - 1
    w = Wave()
    w.issue(("A", 0), apw)
    for k in range(D):
        w.issue(("W", k), ppw)
    w.wait(0)
    for j in range(4):                                  # an even chunk: 4 steps
        w.wait((D - 1) * ppw + (apw if 1 <= j <= D else 0))
        w.issue(("W", D + j), ppw)
        if j == 0:
            w.issue(("A", 1), apw)
    w.wait(4 * ppw)                                     # 3 groups are younger than A(1), not 4
    assert not w.landed(("A", 1))
