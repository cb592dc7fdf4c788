"""CPU-only checks of the update rules in the slot path (include/midd.h: mi_update_row, mi_denoise_slots_rule; midd_amd.SamplerRule,
run_slots_rule, SamplerSession(rule=), DiffusionService(slot_update=)): the row function against the list tables and the float64
restatements, the C call's argument rules on an unfinalized plan, the session's bookkeeping against a recording stand-in for
run_slots_rule, and the Python argument rules.  What the device computes is judged in tests/test_gpu_slots_rule.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from midd_amd import DiffusionDenoiser, SamplerRule, SamplerSession, UNetDiffusion, native
from midd_amd.server import DiffusionService
from tests import ddim_update_reference as ddim_ref
from tests import dpm_update_reference as dpm_ref
from tests import slots_rule_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
COND, X, X0, NOISE = 0x100000, 0x200000, 0x300000, 0x400000      # non-null "device pointers" of calls that fail before anything reads them
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)
_, _, ALPHA_HAT = ddim_ref.schedule(50)
LISTS = {n: ddim_ref.timestep_list(50, k) for n, k in ((50, 50), (25, 25), (13, 12), (9, 8), (5, 5), (2, 2), (1, 1))}


def test_the_lists_have_the_lengths_their_names_say():
    assert {n: len(t) for n, t in LISTS.items()} == {n: n for n in LISTS}


# ------------------------------------------------------------------------------ 1. mi_update_row
def _row(tb, t, ta, eta=0.0, alpha_hat=ALPHA_HAT, noise_steps=50):
    out = np.full(8, np.nan, np.float32)
    rc = native.lib().mi_update_row(tb, t, ta, alpha_hat.ctypes.data_as(FP), noise_steps, eta, out.ctypes.data_as(FP))
    return rc, out


def _table(fn, t_list, cols, *eta):
    steps = np.asarray(t_list, np.int32)
    out = np.empty((len(steps), cols), np.float32)
    native.check(fn(steps.ctypes.data_as(IP), len(steps), ALPHA_HAT.ctypes.data_as(FP), 50, *eta, out.ctypes.data_as(FP)))
    return out


@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("n", sorted(LISTS))
def test_update_row_equals_the_list_tables_and_the_restatement_bit_for_bit(n, eta):
    t = LISTS[n]
    lib = native.lib()
    ddim_tab = _table(lib.mi_ddim_coefficients, t, 7, C.c_double(eta))
    dpm_tab = _table(lib.mi_dpm_coefficients, t, 8)
    assert np.array_equal(ddim_tab.view(np.uint32), ddim_ref.coefficients(t, ALPHA_HAT, eta).view(np.uint32))
    assert np.array_equal(dpm_tab.view(np.uint32), dpm_ref.coefficients(t, ALPHA_HAT).view(np.uint32))
    for i in range(n):
        tb, ta = ref.neighbours(t, i, 1)
        rc, got = _row(tb, t[i], ta, eta)
        assert rc == 0, native.lib().mi_last_error()
        assert np.array_equal(got[:7].view(np.uint32), ddim_tab[i].view(np.uint32)), (n, eta, i)
        assert got[7].view(np.uint32) == dpm_tab[i, 7].view(np.uint32), (n, i)
        assert np.array_equal(got.view(np.uint32), ref.row(tb, t[i], ta, ALPHA_HAT, eta).view(np.uint32)), (n, eta, i)
    if n >= 3:
        assert np.count_nonzero(dpm_tab[:, 7]) == n - 2      # (the comparison of column 7 is not one of zeros)


def test_update_row_edges_and_refusals():
    rc, first = _row(-1, 24, 18, 0.5)
    assert rc == 0 and first[7] == 0.0 and first[6] > 0.0                            # no history: g = 0
    rc, last = _row(30, 24, -1, 0.5)
    assert rc == 0 and tuple(last[4:]) == (1.0, 0.0, 0.0, 0.0)                       # the list ends: a = 1, b = 0, s = 0, g = 0
    rc, mid = _row(30, 24, 18, 0.0)
    assert rc == 0 and mid[7] != 0.0 and mid[6] == 0.0
    flat = ALPHA_HAT.copy()
    flat[18] = flat[24]
    for args, words in (((-1, 24, 24), ["strictly decreasing"]), ((24, 24, 18), ["strictly decreasing"]), ((18, 24, -1), ["strictly decreasing"]),
                        ((-1, 50, -1), ["t=50", "[0,50)"]), ((-1, -1, -1), ["t=-1"]), ((-2, 24, -1), ["t_before=-2", "-1 = none"]),
                        ((-1, 24, 50), ["t_after=50"])):
        rc, _ = _row(*args)
        assert rc == -1, args
        msg = native.lib().mi_last_error().decode()
        assert all(w in msg for w in words), (args, msg)
    for eta in (-0.1, 1.5, float("nan")):
        assert _row(-1, 24, -1, eta)[0] == -1 and b"eta" in native.lib().mi_last_error()
    assert _row(-1, 24, 18, alpha_hat=flat)[0] == -1 and b"alpha_hat" in native.lib().mi_last_error()
    assert _row(-1, 24, -1, noise_steps=0)[0] == -1 and b"noise_steps" in native.lib().mi_last_error()
    assert native.lib().mi_update_row(-1, 24, -1, None, 50, 0.0, np.zeros(8, np.float32).ctypes.data_as(FP)) == -1


# ------------------------------------------------------------------------------ 2. argument rules of mi_denoise_slots_rule
@pytest.fixture()
def plan():
    """An unfinalized plan: every host-side rule can be checked on it, no GPU call can succeed."""
    m = UNetDiffusion(variant="cddpm", **SMALL)
    cfg, c = native.UNetCfg(), m.cfg
    cfg.in_channels, cfg.model_channels, cfg.num_levels = c.in_channels, c.model_channels, len(c.channel_mult)
    for i, v in enumerate(c.channel_mult):
        cfg.channel_mult[i] = v
    cfg.num_res_blocks, cfg.num_attention_levels = c.num_res_blocks, len(c.attention_resolutions)
    for i, v in enumerate(c.attention_resolutions):
        cfg.attention_levels[i] = v
    cfg.time_emb_dim, cfg.variant, cfg.compute_mode = c.time_emb_dim, native.MI_VARIANT["cddpm"], native.MI_COMPUTE["f16x3"]
    h = C.c_void_p()
    native.check(native.lib().mi_unet_plan_create(C.byref(cfg), C.byref(h)))
    yield h
    native.lib().mi_plan_destroy(h)


DDIM, DPM, REFERENCE = (1, 0.5, 1), (2, 0.0, 1), (0, 0.0, 1)


def _call(plan, rule=DDIM, rows=((40, 40), (20, 20), (0, 0)), t_before=None, t_after=None, x0=None, seeded=0, step_noise=None, x=X, B=2):
    t = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
    tb = None if t_before is None else (C.c_int32 * B)(*t_before)
    ta = None if t_after is None else (C.c_int32 * B)(*t_after)
    r = None if rule is None else C.byref(native.UpdateRule(*rule))
    tab = ALPHA_HAT.ctypes.data_as(FP)
    return native.lib().mi_denoise_slots_rule(plan, COND, x, B, 32, 32, t.ctypes.data_as(IP), len(rows), None, None, None, None, tb, ta, x0,
                                              tab, tab, tab, 50, step_noise, seeded, 5, 0, r, None, 0, None)


@pytest.mark.parametrize("kw,words", [
    (dict(rows=((40, 40), (40, 20), (0, 0))), ["t_rows[1][0]=40", "strictly decreasing"]),                  # a non-decreasing column
    (dict(rows=((40, 40), (20, 44), (0, 0))), ["t_rows[1][1]=44", "strictly decreasing"]),
    (dict(t_before=(-1, 40)), ["t_rows[0][1]=40", "t_before=40", "strictly decreasing"]),                   # ... across the first seam
    (dict(t_after=(0, -1)), ["t_after[0]=0", "t_rows[2][0]=0", "strictly decreasing"]),                     # ... across the last one
    (dict(rows=((40, 40), (20, 20), (10, -1)), t_after=(5, 5)), ["t_after[1]=5", "went idle"]),             # t_after after an idle row
    (dict(rows=((-1, 40), (-1, 20), (-1, 10)), t_after=(5, 5)), ["t_after[0]=5", "went idle"]),
    (dict(t_before=(50, -1)), ["t_before[0]=50", "[-1,50)"]),
    (dict(t_after=(-1, -2)), ["t_after[1]=-2", "[-1,50)"]),
    (dict(rule=DPM), ["MI_UPDATE_DPMPP2M without x0_hist"]),
    (dict(rule=DPM, x0=X0, seeded=1), ["seeded with MI_UPDATE_DPMPP2M", "deterministic"]),
    (dict(rule=DPM, x0=X0, step_noise=NOISE), ["step_noise with MI_UPDATE_DPMPP2M", "deterministic"]),
    (dict(rule=DDIM, x0=X0), ["x0_hist with MI_UPDATE_DDIM"]),
    (dict(rule=REFERENCE, x0=X0), ["x0_hist with the reference's update"]),
    (dict(rule=None, t_before=(-1, -1)), ["t_before with the reference's update"]),
    (dict(rule=None, t_after=(-1, -1)), ["t_after with the reference's update"]),
    (dict(rule=DPM, x0=X), ["x and x0_hist alias"]),
    (dict(rule=DPM, x0=X + 4096), ["x and x0_hist alias"]),                                                 # overlapping, not equal
    (dict(rule=DPM, x0=COND), ["cond and x0_hist alias"]),
    (dict(rule=(1, 1.5, 1)), ["eta 1.5"]),
    (dict(rule=(7, 0.0, 1)), ["unknown update rule 7"]),
    # two broken rules: the kind's own comes first, the table's before the alias
    (dict(rule=DPM, rows=((40, 40), (40, 20), (0, 0))), ["without x0_hist"]),
    (dict(rule=DPM, x0=X, rows=((40, 40), (40, 20), (0, 0))), ["t_rows[1][0]=40"]),
])
def test_every_argument_rule_is_einval_and_names_itself(plan, kw, words):
    assert _call(plan, **kw) == -1, kw
    msg = native.lib().mi_last_error().decode()
    for w in words:
        assert w in msg, (kw, msg)


def test_valid_arguments_reach_the_state_check(plan):
    """Inside every rule the unfinalized plan stops the call: a state error, after every MI_EINVAL rule and before any GPU work."""
    lib = native.lib()
    for kw in (dict(), dict(rule=DPM, x0=X0), dict(rule=None), dict(rule=REFERENCE, seeded=1),
               dict(t_before=(46, -1), t_after=(-1, -1)),
               dict(rows=((40, 40), (20, 20), (10, 10)), t_before=(46, 45), t_after=(5, 0)),
               dict(rows=((40, 40), (20, -1), (10, -1)), t_after=(5, -1), rule=DPM, x0=X0),
               dict(rows=((-1, 40), (-1, 20), (-1, 10)), t_before=(30, -1))):                               # (an idle slot's t_before is not read)
        assert _call(plan, **kw) == -2 and b"finalize" in lib.mi_last_error(), (kw, lib.mi_last_error())
    assert _call(None) == -1 and b"null plan" in lib.mi_last_error()


def test_header_and_binding_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in native.SYMBOLS}
    for name in ("mi_update_row", "mi_denoise_slots_rule"):
        assert name in declared and name in bound and getattr(native.lib(), name) is not None
    assert "NOT BUILT: mi_denoise_slots" not in header and "NOT BUILT under this rule: mi_denoise_slots" not in header
    assert "16 bytes per sample" in header


# ------------------------------------------------------------------------------ 3. the session's bookkeeping
class Recorder:
    """Stands in for UNetDiffusion.run_slots_rule: records every call, adds 1 to an active slot's x per row and, under dpmpp2m,
    writes 100 * index + iteration into the slot's x0 per row (so the history says whose it is and how far it ran)."""

    def __init__(self):
        self.calls = []

    def __call__(self, cond, x, t_rows, beta, alpha, alpha_hat, clamp_eps, iter_base=None, sample_index=None, step_noise=None,
                 seed=None, no_split=False, max_slots=None, *, rule=None, t_before=None, t_after=None, x0=None, member=None, frame=None):
        B = cond.shape[0]
        rows = np.asarray(t_rows, dtype=np.int64).reshape(-1, B)
        assert (x0 is not None) == (rule.update == "dpmpp2m") and (x0 is None or x0.shape == x.shape)
        seen = None if x0 is None else [float(x0[b].flatten()[0]) for b in range(B)]
        self.calls.append(dict(rows=rows.T.tolist(), iter_base=list(iter_base), index=list(sample_index), seed=seed, rule=rule,
                               t_before=list(t_before), t_after=list(t_after), x0_in=seen, member=member, frame=frame))
        for i, r in enumerate(rows):
            for b, t in enumerate(r):
                if t >= 0:
                    x[b] += 1.0
                    if x0 is not None:
                        x0[b] = 100.0 * sample_index[b] + iter_base[b] + i
        return x


def _session(rule, variant="ddim", **kw):
    model = UNetDiffusion(variant=variant, **SMALL)
    rec = Recorder()
    model.run_slots_rule = rec
    model.run_slots = None                  # a session under a rule never calls it
    return SamplerSession(DiffusionDenoiser(model, noise_steps=50), 16, 24, rule=rule, **kw), rec


STEPS = (8, 5, 2, 1, 8, 5)                  # lists of 9, 5, 2, 1, 9 and 5 entries
JOINS = (0, 0, 0, 1, 1, 2)                  # ticket j is submitted before step JOINS[j]


@pytest.mark.parametrize("max_rows", [None, 1, 2])
@pytest.mark.parametrize("update", ["ddim", "dpmpp2m"])
def test_the_session_hands_every_slot_its_neighbours_and_moves_its_history(update, max_rows):
    rule = SamplerRule(update)
    s, rec = _session(rule, slots=3, max_rows=max_rows)
    lists = [ddim_ref.timestep_list(50, k) for k in STEPS]
    images = [torch.full((1, 1, 16, 24), float(j)) for j in range(len(STEPS))]
    tickets, step = [], 0
    while len(tickets) < len(STEPS) or s.pending():
        tickets += [s.submit(images[j], STEPS[j]) for j in range(len(STEPS)) if JOINS[j] == step]
        s.step()
        step += 1
    want = ref.session_calls(lists, JOINS, 3, max_rows)
    assert len(rec.calls) == len(want) and len(want) > 3
    moved, slot_of = 0, {}
    for call, slots in zip(rec.calls, want):
        assert call["rule"] is rule and call["seed"] is None and call["member"] is None and call["frame"] is None
        assert call["index"] == [j for j, _, _ in slots] and call["iter_base"] == [pos for _, pos, _ in slots]
        for b, (j, pos, k) in enumerate(slots):
            assert call["rows"][b] == lists[j][pos:pos + k], (j, pos, k)
            assert (call["t_before"][b], call["t_after"][b]) == ref.neighbours(lists[j], pos, k), (j, pos, k)
            if update == "dpmpp2m" and pos > 0:
                # the history a slot reads is the one ITS ticket wrote in its previous row, wherever compaction has put the slot since
                assert call["x0_in"][b] == 100.0 * j + pos - 1, (j, pos, call["x0_in"])
            moved += pos > 0 and slot_of[j] != b
            slot_of[j] = b
    assert moved > 0                                    # compaction did move a ticket mid-list
    for j, t in enumerate(tickets):
        assert torch.equal(t.result(), images[j] + float(len(lists[j])))
    assert (s._x0 is not None) == (update == "dpmpp2m")
    s.close()
    assert s._x0 is None


def test_compaction_moves_a_history_mid_list():
    """Two slots, lists of 1 and 9 entries, then a third ticket: slot 1's ticket moves into slot 0 after the first call, mid-list."""
    s, rec = _session(SamplerRule("dpmpp2m"), slots=2, max_rows=2)
    a, b = s.submit(torch.zeros(1, 16, 24), 1), s.submit(torch.ones(1, 16, 24), 8)
    s.step()
    c = s.submit(torch.zeros(1, 16, 24), 2)
    s.drain()
    first, second = rec.calls[0], rec.calls[1]
    assert first["index"] == [0, 1] and first["rows"] == [[0], [48]]
    assert second["index"] == [1, 2] and second["iter_base"] == [1, 0] and second["x0_in"][0] == 100.0       # ticket 1's history, now in slot 0
    assert (second["t_before"], second["t_after"]) == ([48, -1], [30, -1])
    assert all(t.done() for t in (a, b, c))


# ------------------------------------------------------------------------------ 4. Python argument rules
def test_sampler_rule_is_a_checked_frozen_value():
    r = SamplerRule()
    assert (r.update, r.eta, r.clip_x0, r.draws) == ("ddim", 0.0, True, False)
    assert SamplerRule("ddim", 0.5) == SamplerRule("ddim", eta=0.5, clip_x0=True) and SamplerRule("ddim", 0.5).draws
    assert SamplerRule("dpmpp2m", clip_x0=False).kwargs() == dict(update="dpmpp2m", eta=0.0, clip_x0=False)
    assert not SamplerRule("dpmpp2m").draws and len({SamplerRule("ddim", 1), SamplerRule("ddim", 1.0)}) == 1
    with pytest.raises(Exception):
        r.eta = 0.5
    for args in (("reference",), ("dpm",), ("ddim", 1.5), ("ddim", float("nan")), ("ddim", True), ("dpmpp2m", 0.5), ("ddim", 0.0, "yes")):
        with pytest.raises(ValueError):
            SamplerRule(*args)
    native_rule = SamplerRule("ddim", 0.25, False).native()
    assert (native_rule.kind, native_rule.eta, native_rule.clip_x0) == (1, 0.25, 0)


def test_ticket_kinds_under_a_rule():
    img = torch.zeros(1, 16, 24)
    for rule in (SamplerRule("ddim"), SamplerRule("dpmpp2m")):
        for variant in ("ddim", "cddpm"):
            s, _ = _session(rule, variant=variant, seed=7)            # a seed is allowed and nothing is drawn
            assert s.seed is None and not s.stochastic
            with pytest.raises(ValueError, match="deterministic"):
                s.submit_ensemble(img, 3, members=3)
            s.submit(img, 3)
            s.submit_tiled(torch.zeros(1, 40, 40), 3, overlap=4)
            s.close()
    for variant in ("ddim", "cddpm"):
        s, rec = _session(SamplerRule("ddim", 0.5), variant=variant, seed=7)
        assert s.seed == 7 and s.stochastic
        s.submit_ensemble(img, 1, members=2, member_offset=3)
        s.reduce = lambda samples: (samples.mean(dim=1), None)
        s.step()
        assert rec.calls[0]["seed"] == 7 and rec.calls[0]["member"] == [3, 4] and rec.calls[0]["frame"] == [(24, 384, 0)] * 2
        s.close()
        drawn, _ = _session(SamplerRule("ddim", 0.5), variant=variant)
        assert isinstance(drawn.seed, int)                             # always seeded, as a cddpm session is
    d = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    for bad in ("ddim", native.UpdateRule(1, 0.0, 1)):
        with pytest.raises(ValueError, match="SamplerRule"):
            SamplerSession(d, 16, 24, rule=bad)
        with pytest.raises(ValueError, match="SamplerRule"):
            d.denoise_ragged(torch.zeros(1, 1, 32, 32), [3], rule=bad)
    # the refusals of update= stand and name the new spelling
    for call in (lambda: SamplerSession(d, 16, 24, update="ddim"), lambda: d.denoise_ragged(torch.zeros(1, 1, 32, 32), [3], update="dpmpp2m")):
        with pytest.raises(ValueError, match=r"reference's update only.*rule=SamplerRule"):
            call()


def test_run_slots_rule_argument_rules():
    d = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    x = torch.zeros(2, 1, 32, 32)
    tabs = (d.beta, d.alpha, d.alpha_hat)
    run = d.model.run_slots_rule
    with pytest.raises(ValueError, match="x0"):
        run(x, x.clone(), [[3, 3]], *tabs, clamp_eps=True, rule=SamplerRule("dpmpp2m"))
    with pytest.raises(ValueError, match="x0"):
        run(x, x.clone(), [[3, 3]], *tabs, clamp_eps=True, rule=SamplerRule("ddim"), x0=x.clone())
    with pytest.raises(ValueError, match="x0"):
        run(x, x.clone(), [[3, 3]], *tabs, clamp_eps=True, x0=x.clone())
    with pytest.raises(ValueError, match="deterministic"):
        run(x, x.clone(), [[3, 3]], *tabs, clamp_eps=True, rule=SamplerRule("dpmpp2m"), x0=x.clone(), seed=3)
    with pytest.raises(ValueError, match="t_before"):
        run(x, x.clone(), [[3, 3]], *tabs, clamp_eps=True, t_before=[-1, -1])
    with pytest.raises(ValueError, match="x0 must match x"):
        run(x, x.clone(), [[3, 3]], *tabs, clamp_eps=True, rule=SamplerRule("dpmpp2m"), x0=torch.zeros(1, 1, 32, 32))
    for rule, kw in ((SamplerRule("ddim", 0.5), dict(seed=1)), (SamplerRule("dpmpp2m"), dict(x0=x.clone())), (None, {})):
        with pytest.raises(RuntimeError, match="no CPU fallback"):     # valid arguments, CPU tensors: never a silent fall-back
            run(x, x.clone(), [[3, 3]], *tabs, clamp_eps=True, rule=rule, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.denoise_ragged(x, [3, 1], rule=SamplerRule("dpmpp2m"))


def test_service_slot_update(monkeypatch):
    for name in ("MIDD_UPDATE", "MIDD_ETA", "MIDD_SLOT_UPDATE", "MIDD_SLOT_ETA", "MIDD_BATCH_SLOTS"):
        monkeypatch.delenv(name, raising=False)
    cpu = torch.device("cpu")
    svc = DiffusionService(device=cpu, batch_slots=4)
    assert (svc.slot_update, svc.slot_eta, svc.slot_rule) == ("reference", 0.0, None)
    svc = DiffusionService(device=cpu, batch_slots=4, slot_update="ddim", slot_eta=0.5)
    assert svc.slot_rule == SamplerRule("ddim", 0.5) and svc.update == "reference"
    assert DiffusionService(device=cpu, batch_slots=4, slot_update="dpmpp2m").slot_rule == SamplerRule("dpmpp2m")
    with pytest.raises(ValueError, match="batch_slots > 0"):
        DiffusionService(device=cpu, slot_update="ddim")
    with pytest.raises(ValueError, match="deterministic"):
        DiffusionService(device=cpu, batch_slots=4, slot_update="dpmpp2m", slot_eta=0.5)
    with pytest.raises(ValueError):
        DiffusionService(device=cpu, batch_slots=4, slot_eta=0.5)                      # eta belongs to a rule
    for update in ("ddim", "dpmpp2m"):                                                 # update= with batch_slots stays refused
        with pytest.raises(ValueError, match=r"reference's update only.*slot_update"):
            DiffusionService(device=cpu, batch_slots=4, update=update)
        with pytest.raises(ValueError, match="reference's update only"):
            DiffusionService(device=cpu, batch_slots=4, update=update, slot_update="ddim")
    monkeypatch.setenv("MIDD_SLOT_UPDATE", "ddim")
    monkeypatch.setenv("MIDD_SLOT_ETA", "1")
    monkeypatch.setenv("MIDD_BATCH_SLOTS", "2")
    svc = DiffusionService(device=cpu)
    assert (svc.batch_slots, svc.slot_rule) == (2, SamplerRule("ddim", 1.0))
    monkeypatch.setenv("MIDD_SLOT_UPDATE", "dpm")
    with pytest.raises(ValueError):
        DiffusionService(device=cpu)
    monkeypatch.setenv("MIDD_SLOT_UPDATE", "dpmpp2m")
    with pytest.raises(ValueError, match="deterministic"):                             # (MIDD_SLOT_ETA is still 1)
        DiffusionService(device=cpu)
    monkeypatch.delenv("MIDD_SLOT_ETA")
    monkeypatch.setenv("MIDD_BATCH_SLOTS", "0")
    with pytest.raises(ValueError, match="batch_slots > 0"):
        DiffusionService(device=cpu)
    monkeypatch.setenv("MIDD_BATCH_SLOTS", "3")

    # the session the service builds carries the rule, and /health reports it beside the keys it had
    made = {}

    class Den:
        pass

    import midd_amd.session as session_mod
    monkeypatch.setattr(session_mod, "SamplerSession", lambda den, H, W, **kw: made.update(kw, shape=(H, W)) or "session")
    svc = DiffusionService(device=cpu)
    svc.diffusion_denoiser = Den()
    assert svc._make_session() == "session" and made["rule"] == SamplerRule("dpmpp2m") and made["slots"] == 3
    from fastapi.testclient import TestClient
    from midd_amd.server import create_app
    svc = DiffusionService(device=cpu, denoise_fn=lambda x: x)
    with TestClient(create_app(service=svc)) as client:
        health = client.get("/health").json()
    assert health["slot_update"] == "dpmpp2m" and health["update"] == "reference" and health["batch_slots"] == 3
