"""numpy restatement of the per-slot rows of the DDIM(eta) and DPMPP2M updates (include/midd.h: mi_update_row, mi_denoise_slots_rule):
a row is a function of a timestep and its neighbours in the slot's own list, -1 = none, so it is the row of the list restatements
(tests/ddim_update_reference.py, tests/dpm_update_reference.py) for the shortest list that holds the triple.  Also what a session
hands a call for a slot at position ``pos`` of its list when the call runs ``k`` rows.  Nothing here imports the package."""
import numpy as np

from tests import ddim_update_reference as ddim
from tests import dpm_update_reference as dpm

COLUMNS = dpm.COLUMNS


def row(t_before, t, t_after, alpha_hat, eta):
    """float32 [8]: (k0, k1, r0, r1, a, b, s, g).  Columns 0 .. 6 depend on (t, t_after) alone, g on the whole triple."""
    out = np.empty(8, np.float32)
    out[:7] = ddim.coefficients([t] + ([t_after] if t_after >= 0 else []), alpha_hat, eta)[0]
    out[7] = dpm.weight([t_before, t, t_after], alpha_hat, 1) if t_before >= 0 and t_after >= 0 else 0.0
    return out


def neighbours(t_list, pos, k):
    """(t_before, t_after) of a call that runs rows pos .. pos + k - 1 of a slot's list."""
    return (t_list[pos - 1] if pos > 0 else -1), (t_list[pos + k] if pos + k < len(t_list) else -1)


def session_calls(lists, joins, slots, max_rows):
    """The calls of a session of ``slots`` slots: ticket j (its list ``lists[j]``) is submitted before step ``joins[j]`` (ascending).
    -> per call, a list of (ticket, pos, k) for the active slots in slot order -- admission in submission order into the prefix,
    k = the shortest remaining list capped at max_rows, compaction by moving the last active slot into the highest hole first."""
    queue, active, calls, step, nxt = [], [], [], 0, 0
    while nxt < len(lists) or queue or active:
        while nxt < len(lists) and joins[nxt] <= step:
            queue.append(nxt)
            nxt += 1
        while queue and len(active) < slots:
            active.append([queue.pop(0), 0])
        if active:
            k = min(len(lists[j]) - pos for j, pos in active)
            k = k if max_rows is None else min(k, max_rows)
            calls.append([(j, pos, k) for j, pos in active])
            for s in active:
                s[1] += k
            for i in reversed([i for i, (j, pos) in enumerate(active) if pos == len(lists[j])]):
                if i != len(active) - 1:
                    active[i] = active[-1]
                active.pop()
        step += 1
    return calls
