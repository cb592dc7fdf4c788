"""CPU emulation of CUDA autocast for the yardstick of compute="f16" (DESIGN.md section 4).

`AutocastEmulation` is a TorchFunctionMode under which `conv2d`, `conv_transpose2d`, `linear`, `matmul` / `bmm` see every fp32
tensor argument rounded to fp16 (round to nearest even) and back, and -- with round_results=True, the autocast emulation -- return
their result rounded the same way; everything else stays fp32.  With round_results=False ("inputs only") it is the arithmetic
contract of compute="f16" itself, in torch: fp16 multiplicands, fp32 accumulation and results.

The distance of a network run under the emulation to the plain fp32 run is the yardstick E (max-norm and root-mean-square);
`gate(delta, E)` is the acceptance rule of the mode: max|delta| <= 2 E_max and rms(delta) <= 1.5 E_rms.  The emulation leaves out
the fp16 rounding autocast also applies inside SiLU and the additions, so E is if anything smaller than a real autocast run's.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch.overrides import TorchFunctionMode

MAX_FACTOR, RMS_FACTOR = 2.0, 1.5

_OPS = {F.conv2d, F.conv_transpose2d, F.linear, torch.matmul, torch.bmm, torch.Tensor.matmul, torch.Tensor.__matmul__, torch.Tensor.bmm}


def _round16(v):
    return v.half().float() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else v


class AutocastEmulation(TorchFunctionMode):
    def __init__(self, round_results=True):
        super().__init__()
        self.round_results = round_results
        self.calls = 0

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func in _OPS:
            self.calls += 1
            out = func(*[_round16(a) for a in args], **{k: _round16(v) for k, v in kwargs.items()})
            return _round16(out) if self.round_results else out
        return func(*args, **kwargs)


def distance(a, b):
    """(max-norm, root-mean-square) of a - b, as Python floats (float64 arithmetic)."""
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


def gate(got, want_fp32, e_max, e_rms, what=""):
    """Asserts the acceptance rule of compute="f16" for `got` against the fp32 values; prints the figures first."""
    d_max, d_rms = distance(got, want_fp32)
    print(f"f16 gate {what}: max|d| {d_max:.3e} (E_max {e_max:.3e}, ratio {d_max / e_max:.2f})  "
          f"rms {d_rms:.3e} (E_rms {e_rms:.3e}, ratio {d_rms / e_rms:.2f})")
    assert np.isfinite(d_max) and d_max <= MAX_FACTOR * e_max, (what, d_max, e_max)
    assert d_rms <= RMS_FACTOR * e_rms, (what, d_rms, e_rms)
    return d_max, d_rms
