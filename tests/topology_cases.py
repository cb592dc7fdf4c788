"""Shared by tests/test_topology_sweep_cpu.py and tests/test_gpu_unfolded_topologies.py: the topologies whose ConvTranspose the planner
cannot fold into a 3x3 (the popped skip already has the doubled size, so `flush_up` in csrc/midd_planner.hip materialises it with
conv_transpose_kernel + chan_total_kernel), the grid of constructor arguments the host-only sweep walks, and a per-module
restatement of the network on tensors of any float type (float64 for the tests) built from the oracle's own block functions.

TEST INFRASTRUCTURE ONLY: nothing here is imported by the package.
"""
import itertools
import re

import numpy as np
import torch
import torch.nn.functional as F

from midd_amd.config import UNetConfig, param_shapes, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc


def _kw(mc, mult, nrb, att, te):
    return dict(model_channels=mc, channel_mult=mult, num_res_blocks=nrb, attention_resolutions=att, time_emb_dim=te)


# id -> (variant, constructor kwargs, B, H, W).  Every one lists conv_transpose_kernel and chan_total_kernel in its plan
# (tests/test_topology_sweep_cpu.py::test_unfolded_cases_reach_the_two_kernels).
UNFOLDED_CASES = {
    # ConvT 8x12 -> 16x24 at C = 64; chan_total with 3 pixel rows and stat_rep 5; attention at level 0 with key split 4
    "A": ("cddpm", _kw(32, (2, 2), 1, (0,), 32), 3, 16, 24),
    # two materialised ConvT, the smallest from a 2x3 map (every output pixel is a border pixel), plus one bilinear 2x
    "B": ("ddim", _kw(32, (2, 2, 2, 2), 1, (1,), 40), 2, 16, 24),
    # ConvT 12x20 -> 24x40, five attention blocks at level 1 (key split 4), resize
    "C": ("ddim", _kw(32, (1, 2, 2), 2, (1,), 32), 2, 24, 40),
    # ConvT at C = 128, head_dim 64, two resizes
    "D": ("cddpm", _kw(16, (2, 4, 8, 8), 1, (2,), 32), 2, 16, 16),
    # ConvT at C = 192 (chan_total: 48 quads -> 5 pixel lanes, 16 idle threads), key split 8, head dims 32 / 64 / 96
    "E": ("cddpm", _kw(64, (1, 2, 3), 2, (0, 1), 64), 1, 32, 16),
}


def case_inputs(cid):
    """(cfg, topo, fp32 state dict (torch), x, cond, t) of a case: shared by the CPU and the GPU tests"""
    variant, kw, B, H, W = UNFOLDED_CASES[cid]
    cfg = UNetConfig(variant=variant, **kw)
    seed = 700 + ord(cid)
    sd = orc.to_torch(make_state_dict(cfg, seed=seed, perturb_norm=True))
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.random((B, 1, H, W), dtype=np.float32))
    cond = torch.from_numpy(synthetic_xray(B, H, W, seed=seed))
    t = torch.from_numpy(rng.integers(0, 50, B)).to(torch.int64)
    return cfg, topology(cfg), sd, x, cond, t


GRID_VARIANTS = ("ddim", "cddpm")
GRID_MODEL_CHANNELS = (32, 64)
GRID_CHANNEL_MULT = ((1, 2), (2, 2), (1, 1), (1, 2, 2), (1, 2, 3), (2, 2, 4), (2, 2, 2, 2), (1, 2, 3, 4))
GRID_NUM_RES_BLOCKS = (1, 2, 3)


def attention_placements(levels):
    """none, each single level, every pair of levels"""
    return [()] + [(i,) for i in range(levels)] + list(itertools.combinations(range(levels), 2))


def grid():
    """(variant, kwargs) over both variants, two widths, eight channel_mult tuples of 2-4 levels, 1-3 residual blocks per level and
    every attention placement of at most two levels."""
    for variant, mc, mult, nrb in itertools.product(GRID_VARIANTS, GRID_MODEL_CHANNELS, GRID_CHANNEL_MULT, GRID_NUM_RES_BLOCKS):
        for att in attention_placements(len(mult)):
            yield variant, _kw(mc, mult, nrb, att, 32)


# ------------------------------------------------------------------------------ plan dump helpers (host only)
def op_signatures(dump_text):
    """The op kinds a plan reaches, one string per distinct kind: the planner's op column, the kernel family (template arguments
    dropped), kernel size, stride, prologue, attention hand-off mode, and whether the launch reads a concatenated second source
    and a folded res_conv."""
    out = set()
    for line in dump_text.splitlines()[1:]:
        m = re.match(r"op\d+ (\w+)\s+\d+x\d+ c\d+\+(\d+)->\d+ k(\d+) s(\d+) pro(\d+) res_steps(\d+) att(\d+) .*\| (midd::\w+)", line)
        assert m, line
        kind, c1, ks, stride, pro, res, att, kernel = m.groups()
        out.add(f"{kind} {kernel} k{ks} s{stride} pro{pro} att{att} cat{int(int(c1) > 0)} res{int(int(res) > 0)}")
    return out


def kernels(dump_text):
    return {m.group(1) for m in re.finditer(r"\| (midd::\w+)", dump_text)}


# ------------------------------------------------------------------------------ the network, module by module, in any float type
def zero_state_dict(cfg, dtype=torch.float32):
    """Weights of the right shapes and nothing else (the sweep only asks whether the graph closes)."""
    return {name: torch.zeros(shape, dtype=dtype) for name, shape in param_shapes(cfg)}


def cast_state_dict(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def walk(sd, topo, x, condition, t, given=None, dtype=torch.float64):
    """Every module output of UNetDiffusion.forward as {name: tensor} (`out_conv` is eps), computed in `dtype` with the oracle's
    block functions.  `sd` must already be in `dtype`.  The sinusoidal embedding stays float32 -- that is the specification
    (oracle/ddim_oracle.py::sinusoidal) -- and is promoted after it.

    Chained (`given` None) this is oracle.unet_forward.  With `given` = {name: tensor}, a module whose input is the output of a
    module named there (its predecessor, or the skip it pops) reads the given tensor instead of this walk's own, so each output
    is one module applied to the given inputs: that module's error alone, nothing from upstream."""
    given = given or {}
    out = {}

    def src(name):
        return given[name].to(dtype) if name in given else out[name]

    e = orc.sinusoidal(t, topo.cfg.model_channels)
    assert e.dtype == torch.float32
    e = F.linear(e.to(dtype), sd["time_mlp.1.weight"], sd["time_mlp.1.bias"])
    temb = out["time_mlp"] = F.linear(F.silu(e), sd["time_mlp.3.weight"], sd["time_mlp.3.bias"])
    h = torch.cat([x, condition], dim=1).to(dtype)
    out["in_conv"] = F.conv2d(h, sd["in_conv.weight"], sd["in_conv.bias"], padding=1)
    prev = "in_conv"

    def run(m, h):
        if m.kind == "rb":
            return orc.residual_block(sd, m.name, h, temb)
        if m.kind == "attn":
            return orc.attention_block(sd, m.name, h)
        if m.kind == "down":
            return F.conv2d(h, sd[f"{m.name}.weight"], sd[f"{m.name}.bias"], stride=2, padding=1)
        assert m.kind == "up", m.kind
        return F.conv_transpose2d(h, sd[f"{m.name}.weight"], sd[f"{m.name}.bias"], stride=2, padding=1)

    skips = []
    for m in topo.downs:
        out[m.name] = run(m, src(prev))
        prev = m.name
        skips.append(m.name)
    for m in topo.mid:
        out[m.name] = run(m, src(prev))
        prev = m.name
    for m in topo.ups:
        h = src(prev)
        if m.kind == "rb":
            skip = src(skips.pop())
            if h.shape[2:] != skip.shape[2:]:
                h = F.interpolate(h, size=skip.shape[2:], mode="bilinear", align_corners=False)
            h = torch.cat([h, skip], dim=1)
        out[m.name] = run(m, h)
        prev = m.name
    h = F.group_norm(src(prev), 8, sd["out_conv.0.weight"], sd["out_conv.0.bias"], eps=1e-5)
    out["out_conv"] = F.conv2d(F.silu(h), sd["out_conv.2.weight"], sd["out_conv.2.bias"], padding=1)
    return out


def rb_inputs(topo, name):
    """(predecessor, popped skip) module names of residual block `name` in `ups`."""
    skips = [m.name for m in topo.downs]
    prev = topo.mid[-1].name
    for m in topo.ups:
        skip = skips.pop() if m.kind == "rb" else None
        if m.name == name:
            return prev, skip
        prev = m.name
    raise KeyError(name)


def materialised_ups(topo, H, W):
    """[(up module, predecessor, consumer residual block)] of the ConvTranspose modules whose consumer pops a skip that does not
    have the pre-upsample size -- the ones the planner cannot fold -- for an H x W input.  Sizes follow the same walk as above."""
    size = {"in_conv": (H, W)}
    prev = "in_conv"
    skips = []
    for m in topo.downs + topo.mid:
        h, w = size[prev]
        size[m.name] = (h // 2, w // 2) if m.kind == "down" else (h, w)
        prev = m.name
        if m in topo.downs:
            skips.append(m.name)
    found, pending = [], None
    for m in topo.ups:
        h, w = size[prev]
        if m.kind == "up":
            size[m.name] = (2 * h, 2 * w)
            pending = (m.name, prev)
        elif m.kind == "rb":
            skip = size[skips.pop()]
            if pending and skip != size[pending[1]]:       # (the fold needs the skip at the pre-upsample size)
                found.append(pending + (m.name,))
            size[m.name] = skip
            pending = None
        else:
            assert pending is None, "an attention block straight after a ConvTranspose is not in the case list"
            size[m.name] = (h, w)
        prev = m.name
    return found


# ------------------------------------------------------------------------------ the fp32 ConvTranspose bound
def conv_transpose_bound(x, w, b):
    """Per-element a-priori bound on |fp32 result - exact| of ConvTranspose2d(Cin, Cout, 4, 2, 1) for ANY summation order with one
    rounding per operation: an output is a sum of at most n = 4 Cin + 1 terms (four taps of Cin products, and the bias), so the
    error is at most gamma_n * sum|terms| with gamma_n = n u / (1 - n u) <= (n + 1) u for n^2 u <= 1, u = 2^-24 (Higham, Accuracy
    and Stability of Numerical Algorithms, section 3.1; n <= 4 * 1024 + 1 here)."""
    x, w, b = x.double(), w.double(), b.double()
    n = 4 * x.shape[1] + 1
    mag = F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2, padding=1)
    return (n + 1) * 2.0 ** -24 * mag
