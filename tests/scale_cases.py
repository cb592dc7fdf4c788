"""Shared by tests/test_scale_cases_cpu.py and tests/test_gpu_dynamic_range.py: the lever that scales the residual stream of the network
by an exact power of two, mixed-scale batches, the four configurations both files run, and their references (fp32 oracle trace and
float64 chained walk), computed once per (configuration, scale).

The lever.  The stream is what in_conv writes and every module adds to.  Multiplying the parameters that WRITE it by s = 2^k -- in_conv,
every residual block's block2.3, every attention block's proj, and the bias alone of every res_conv, stride-2 convolution and
ConvTranspose (their weights act on a stream that is already scaled) -- multiplies the stream by s exactly in exact arithmetic, and
by a power of two in fp32 (no rounding changes).  Everything that READS the stream does so through a GroupNorm, which is
scale-invariant up to its eps = 1e-5, so block1, qkv, out_conv and with them eps see what they saw at s = 1.

TEST INFRASTRUCTURE ONLY: nothing here is imported by the package.
"""
import functools

import numpy as np
import torch

from midd_amd.config import UNetConfig, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import topology_cases as tc

# id -> (variant, constructor kwargs, B, H, W): the smallest networks that reach each raw-operand kernel; 24 x 40 leaves ragged edge
# tiles on both axes.  unfolded_A keeps the size of tests/topology_cases.py::UNFOLDED_CASES["A"].
CONFIGS = {
    "small": ("ddim", dict(model_channels=16, time_emb_dim=64), 3, 24, 40),
    "default": ("ddim", {}, 3, 24, 40),
    "unfolded_A": tc.UNFOLDED_CASES["A"],
    "rgb": ("ddim", dict(in_channels=3), 3, 24, 40),
}
# Weight seeds, chosen for a PRECONDITION of the inputs and nothing else: the lever must put every stream layer within a factor 2 of
# 2^k x its size at k = 0 (tests/test_scale_cases_cpu.py asserts it in float64; no device code is involved).  That is not automatic
# at k <= -12: once the stream is below sqrt(eps) = 3e-3 a GroupNorm no longer normalises it, its output collapses to beta, and what
# each block adds to the stream is set by the betas instead of the data -- still s x (an O(1) tensor), but a different one, whose
# smallest layer is 0.37 .. 0.60 of the k = 0 one over seeds 1 .. 12 of every configuration here (1.0 .. 1.34 at the upper end).
# These are the seeds in 1 .. 12 with the largest minimum ratio: 0.577, 0.568, 0.596, 0.602.
SEEDS = {"small": 5, "default": 8, "unfolded_A": 11, "rgb": 10}
TIMESTEPS = (3, 49, 20)
CPU_SCALES = (-30, -12, 0, 12, 20, 32, 40, None)          # k; None: s = 0
MIXED_SCALES = (2.0 ** -10, 1.0, 2.0 ** 12)


def scale_of(k):
    return 0.0 if k is None else 2.0 ** k


def stream_writers(topo):
    """(parameters scaled whole, parameters of which only the bias is scaled) as state-dict prefixes"""
    whole, bias_only = ["in_conv"], []
    for m in topo.downs + topo.mid + topo.ups:
        if m.kind == "rb":
            whole.append(f"{m.name}.block2.3")
            if m.in_c != m.out_c:
                bias_only.append(f"{m.name}.res_conv")
        elif m.kind == "attn":
            whole.append(f"{m.name}.proj")
        else:
            assert m.kind in ("down", "up"), m.kind
            bias_only.append(m.name)
    return whole, bias_only


def scaled_state_dict(sd, topo, k):
    """A copy of the fp32 torch state dict `sd` with the stream-writing parameters multiplied by 2^k exactly (k None: by 0)."""
    s = scale_of(k)
    whole, bias_only = stream_writers(topo)
    out = {name: v.clone() for name, v in sd.items()}
    for name in [f"{p}.weight" for p in whole] + [f"{p}.bias" for p in whole + bias_only]:
        assert sd[name].dtype == torch.float32, name
        out[name] = sd[name] * s
        assert torch.equal(out[name].double(), sd[name].double() * s), name       # a power of two inside fp32's range: nothing rounded
    return out


def mixed_inputs(x, cond, scales=MIXED_SCALES):
    """x[b] and cond[b] multiplied by scales[b]"""
    s = torch.tensor(scales, dtype=x.dtype).reshape(-1, 1, 1, 1)
    assert s.shape[0] == x.shape[0]
    return x * s, cond * s


def rel_per_sample(got, want, floor):
    """max over b of  max|got[b] - want[b]| / max(floor, max|want[b]|)  in float64.  NaN in `got` gives NaN (which fails every `<`)."""
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    B = want.shape[0]
    err = (got - want).abs().reshape(B, -1).amax(dim=1)
    den = want.abs().reshape(B, -1).amax(dim=1).clamp_min(float(floor))
    return float((err / den).max())


def stream_layers(topo):
    """names of the module outputs that ARE the stream: in_conv and every module of downs, mid and ups"""
    return ["in_conv"] + [m.name for m in topo.downs + topo.mid + topo.ups]


# ------------------------------------------------------------------------------ the upper end of the statistics range
# csrc/stats_common.h::stat_add_lds: a producer workgroup converts its fp32 partial sum of squares of ONE channel of ONE sample to
# fixed point, and a partial >= 2^59 (biased exponent > 185) adds STAT_NAN_SENTINEL instead: the group then reads as NaN and the
# call reports MI_ERANGE.  A workgroup's partial covers its tile(s) of one sample -- 16 .. 128 pixels per tile of the MFMA
# convolutions, times the tiles a persistent workgroup walks -- so, whatever the planner chose, the LARGEST partial P of a tensor lies in
#     max x^2  <=  P  <=  max over (sample, channel) of the sum of x^2 over the image,
# and both ends scale as 4^k under the lever.
STAT_RANGE_LOG2 = 59
RANGE_MARGIN_BINADES = 4          # of the partial: 2^55 and 2^63
GPU_SCALES = (-30, -12, 12, 20)   # returned and gated
ERANGE_SCALES = (32, 40)          # reported as MI_ERANGE, never returned


def partial_bracket_log2(w64, topo):
    """(log2 of a lower bound, log2 of an upper bound) of the largest per-channel sum-of-squares partial any producer workgroup can
    form over the stream layers of the float64 walk `w64`"""
    lo = max(float(w64[n].square().amax()) for n in stream_layers(topo))
    hi = max(float(w64[n].square().sum(dim=(2, 3)).amax()) for n in stream_layers(topo))
    return float(np.log2(lo)), float(np.log2(hi))


@functools.lru_cache(maxsize=None)
def case(cid):
    """(cfg, topo, fp32 torch state dict, x, cond, t) of a configuration; never written to"""
    variant, kw, B, H, W = CONFIGS[cid]
    cfg = UNetConfig(variant=variant, **kw)
    seed = SEEDS[cid]
    sd =orc.to_torch(make_state_dict(cfg, seed=seed, perturb_norm=True))
    ic = cfg.in_channels
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.random((B, ic, H, W), dtype=np.float32))
    cond = torch.from_numpy(np.concatenate([synthetic_xray(B, H, W, seed=seed + 31 * c) for c in range(ic)], axis=1))
    t = torch.tensor(TIMESTEPS, dtype=torch.int64)
    assert B == len(TIMESTEPS)
    return cfg, topology(cfg), sd, x, cond, t


def _both_walks(sd, topo, x, cond, t):
    trace = {}
    with torch.no_grad():
        orc.unet_forward(sd, topo, x, cond, t, trace=lambda n, v: trace.__setitem__(n, v))
        w64 = tc.walk(tc.cast_state_dict(sd, torch.float64), topo, x, cond, t)
    return trace, w64


@functools.lru_cache(maxsize=None)
def reference(cid, k):
    """(scaled state dict, fp32 oracle trace, float64 chained walk) of configuration `cid` at stream scale 2^k: computed once,
    shared, never written to"""
    cfg, topo, sd, x, cond, t = case(cid)
    sdk = scaled_state_dict(sd, topo, k)
    return (sdk,) + _both_walks(sdk, topo, x, cond, t)


@functools.lru_cache(maxsize=None)
def mixed_reference(cid, reverse=False):
    """(x, cond, t, fp32 oracle trace, float64 walk) of the mixed-scale batch on the unscaled weights; `reverse`: batch order reversed"""
    cfg, topo, sd, x, cond, t = case(cid)
    xm, cm = mixed_inputs(x, cond)
    if reverse:
        xm, cm, t = xm.flip(0).contiguous(), cm.flip(0).contiguous(), t.flip(0).contiguous()
    return (xm, cm, t) + _both_walks(sd, topo, xm, cm, t)
