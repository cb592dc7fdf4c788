"""CPU-only: mi_denoise and mi_denoise_seeded are mi_denoise_rule with a NULL rule (include/midd.h), so whatever argument a call
breaks, the two spellings refuse it with the same return code and the same mi_last_error text -- one broken argument at a time, and
one case per adjacent pair of each call's order of checks with two broken at once.  On an unfinalized plan, as in
test_batched_call_order_cpu.py, so nothing reaches the GPU: what a call judges before the plan's state is reported as itself (the
null plan; seeded: the counter range), everything after it as the state."""
import ctypes as C

import numpy as np
import pytest

from midd_amd import native
from tests.test_batched_call_order_cpu import plan  # noqa: F401  (the unfinalized cddpm plan)

# non-null "device pointers" for calls that must fail before anything reads them; WS is 256-byte aligned
NOISY, X_OUT, WS = 0x100000, 0x200000, 0x600000
FP = C.POINTER(C.c_float)
TAB = np.linspace(1e-4, 0.02, 50, dtype=np.float32)

# one broken argument each, in the order in which a call judges them (the seeded rules sit between the null plan and the rest)
NULL_PLAN = dict(null_plan=True)
UNIFORM = [NULL_PLAN, dict(noisy=None), dict(x_out=NOISY), dict(tables=False), dict(n_iters=-1), dict(t_list=(40, 50, 0)),
           dict(noise_steps=2000), dict(ws=None), dict(ws=WS + 4), dict(ws_bytes=0), dict()]      # dict(): the unfinalized plan alone
SEEDED_ONLY = [dict(sample_offset=-2), dict(H=65536, W=65536)]
SEEDED = UNIFORM[:1] + SEEDED_ONLY + UNIFORM[1:]


def _pairs(order):
    return order + [dict(a, **b) for a, b in zip(order, order[1:])]


def _call(plan, seeded, through_rule, null_plan=False, noisy=NOISY, x_out=X_OUT, B=2, H=32, W=32, t_list=(40, 20, 0), n_iters=None,
          tables=True, noise_steps=50, sample_offset=0, ws=WS, ws_bytes=1 << 20):
    """-> (rc, mi_last_error) of the call through its own entry, or through mi_denoise_rule(rule=NULL, seeded=...)."""
    lib = native.lib()
    t = np.asarray(t_list, dtype=np.int32)
    tab = TAB.ctypes.data_as(FP) if tables else None
    head = (None if null_plan else plan, noisy, x_out, B, H, W, t.ctypes.data_as(C.POINTER(C.c_int32)),
            len(t) if n_iters is None else n_iters, tab, tab, tab, noise_steps)
    tail = (0, ws, ws_bytes, None)
    if through_rule:
        rc = lib.mi_denoise_rule(*head, None, seeded, 5 if seeded else 0, sample_offset if seeded else 0, tail[0], None, *tail[1:])
    elif seeded:
        rc = lib.mi_denoise_seeded(*head, 5, sample_offset, *tail)
    else:
        rc = lib.mi_denoise(*head, None, *tail)
    return rc, lib.mi_last_error().decode()


@pytest.mark.parametrize("kw", _pairs(UNIFORM), ids=lambda kw: ",".join(kw) or "unfinalized")
def test_mi_denoise_refuses_as_the_null_rule_does(plan, kw):
    own, rule = _call(plan, 0, False, **kw), _call(plan, 0, True, **kw)
    assert own == rule
    assert own[0] == (-1 if "null_plan" in kw else -2), own
    assert ("null plan" if "null_plan" in kw else "finalize") in own[1], own


@pytest.mark.parametrize("kw", _pairs(SEEDED), ids=lambda kw: ",".join(kw) or "unfinalized")
def test_mi_denoise_seeded_refuses_as_the_seeded_null_rule_does(plan, kw):
    own, rule = _call(plan, 1, False, **kw), _call(plan, 1, True, **kw)
    assert own == rule
    # the first broken rule of the order is the one reported
    word = "null plan" if "null_plan" in kw else "sample_offset -2" if "sample_offset" in kw else "2^32" if "H" in kw else "finalize"
    assert own[0] == (-2 if word == "finalize" else -1), own
    assert word in own[1], own
