"""CPU-only checks of the DDIM(eta) update rule (include/midd.h: THE DDIM UPDATE): the exported coefficient table against the
float64 closed form, its anchor to the reference's rule on the stride-1 list, the fixed point of the restated loop
(tests/ddim_update_reference.py) and the argument rules of the C ABI, the Python calls, the CLI and the service.  What the
device computes is judged in test_gpu_ddim_update.py."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, SamplerSession, UNetDiffusion, native, timestep_list
from midd_amd.sampler import check_update, ddim_coefficients, refuse_update
from tests import ddim_update_reference as ref

SMALL = dict(model_channels=16, time_emb_dim=64)
LISTS = [(50, 8), (50, 25), (50, 5), (100, 10)]
I32, F32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("noise_steps,inference_steps", LISTS)
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_exported_table_is_the_float64_closed_form_rounded_once(noise_steps, inference_steps, eta):
    _, _, alpha_hat = ref.schedule(noise_steps)
    t_list = timestep_list(noise_steps, inference_steps)
    assert t_list == ref.timestep_list(noise_steps, inference_steps)
    got = ddim_coefficients(t_list, alpha_hat, eta)
    want = ref.coefficients(t_list, alpha_hat, eta)
    assert got.dtype == np.float32 and got.shape == (len(t_list), 7)
    assert np.array_equal(_bits(got), _bits(want))
    # independent of the restatement's own order of operations: the closed form in plain float64
    for i, t in enumerate(t_list):
        A, P = float(alpha_hat[t]), float(alpha_hat[t_list[i + 1]]) if i + 1 < len(t_list) else 1.0
        sg = eta * math.sqrt((1 - P) / (1 - A)) * math.sqrt(1 - A / P)
        closed = [1 / math.sqrt(A), math.sqrt(1 - A), math.sqrt(A), 1 / math.sqrt(1 - A), math.sqrt(P),
                  math.sqrt(max(0.0, 1 - P - sg * sg)), 2 * sg]
        assert np.array_equal(_bits(got[i]), _bits(np.array(closed, np.float64).astype(np.float32))), (i, t)
    a, b, s = (got[:, ref.COLUMNS.index(c)] for c in "abs")
    assert a[-1] == 1.0 and b[-1] == 0.0 and s[-1] == 0.0
    if eta == 0.0:
        assert not s.any()
    else:
        assert (s[:-1] > 0).all()


# ------------------------------------------------------------------------------ 2. anchor: stride 1, eta = 1 is the reference's rule
@pytest.mark.parametrize("noise_steps", [50, 100])
def test_stride_one_eta_one_is_the_ancestral_rule(noise_steps):
    """On the stride-1 list A / P = alpha_t, so sigma^2 is the ancestral posterior variance (1-P)/(1-A) * beta_t and the update's
    coefficients on x and eps are the reference's c1 and -c1 * c2.  Relative tolerance 1e-3: the table's alpha = 1 - beta carries
    one fp32 rounding (6e-8) of a value whose distance from 1 is the smallest beta (1e-4), i.e. 6e-4 on beta as read back from
    alpha, hence on sigma^2 and c2.  Measured on the 50-step table: 5.6e-5."""
    beta, alpha, alpha_hat = (v.astype(np.float64) for v in ref.schedule(noise_steps))
    t_list = list(range(noise_steps - 1, -1, -1))
    tab = ddim_coefficients(t_list, alpha_hat.astype(np.float32), 1.0).astype(np.float64)
    k0, k1, _, _, a, b, s = tab.T
    worst = 0.0
    for i, t in enumerate(t_list):
        A, P = alpha_hat[t], alpha_hat[t - 1] if t > 0 else 1.0
        c1, c2 = 1 / math.sqrt(alpha[t]), (1 - alpha[t]) / math.sqrt(1 - alpha_hat[t])
        pairs = [((s[i] / 2) ** 2, (1 - P) / (1 - A) * beta[t]), (a[i] * k0[i], c1), (b[i] - a[i] * k0[i] * k1[i], -c1 * c2)]
        for got, want in pairs:
            if want == 0.0:
                assert got == 0.0
            else:
                worst = max(worst, abs(got - want) / abs(want))
    print(f"stride-1 eta=1 anchor, noise_steps {noise_steps}: max relative deviation {worst:.2e}")
    assert worst < 1e-3


# ------------------------------------------------------------------------------ 3. fixed point of the restated loop
@pytest.mark.parametrize("noise_steps,inference_steps", LISTS)
@pytest.mark.parametrize("eta", [0.0, 1.0])
@pytest.mark.parametrize("clip_x0", [True, False])
def test_restated_loop_returns_the_image_a_perfect_predictor_points_at(noise_steps, inference_steps, eta, clip_x0):
    """eps(x, t) = (x - sqrt(A) x*) / sqrt(1 - A) predicts x0 = x* at every step: whatever the start, the noise and the clip, the
    loop ends at x* within 1 fp32 ulp of 1.0 (1.2e-7; measured 6e-8)."""
    _, _, alpha_hat = ref.schedule(noise_steps)
    t_list = timestep_list(noise_steps, inference_steps)
    rng = np.random.default_rng(7)
    star = rng.random((2, 1, 40, 24)).astype(np.float32)
    star[0, 0, :3] = 0.0
    star[1, 0, -3:] = 1.0                                # the ends of the range: the clip's own values
    start = (star + 0.3 * rng.standard_normal(star.shape)).astype(np.float32)
    noise = (0.5 * rng.standard_normal((len(t_list),) + star.shape)).astype(np.float32)

    def eps(x, t):
        A = np.float64(alpha_hat[t])
        return ((x.astype(np.float64) - np.sqrt(A) * star) / np.sqrt(1.0 - A)).astype(np.float32)

    out = ref.loop(start, t_list, alpha_hat, eta, eps, clamp_eps=False, clip_x0=clip_x0, step_noise=noise)
    err = float(np.abs(out.astype(np.float64) - star).max())
    print(f"fixed point ({noise_steps}, {inference_steps}) eta {eta} clip {clip_x0}: max|x - x*| = {err:.2e}")
    assert out.dtype == np.float32 and err <= 1.2e-7


# ------------------------------------------------------------------------------ 4. argument rules
def _coefficients_rc(t_list, eta, noise_steps=50):
    _, _, alpha_hat = ref.schedule(noise_steps)
    steps = np.asarray(t_list, np.int32)
    out = np.zeros((max(1, len(steps)), 7), np.float32)
    rc = native.lib().mi_ddim_coefficients(steps.ctypes.data_as(I32), len(steps), alpha_hat.ctypes.data_as(F32), noise_steps,
                                           C.c_double(eta), out.ctypes.data_as(F32))
    return rc, native.lib().mi_last_error().decode()


@pytest.mark.parametrize("t_list,eta,words", [
    ([24, 24], 0.0, ["strictly decreasing"]),
    ([24, 48], 0.0, ["strictly decreasing"]),
    ([48, 24, 30], 0.0, ["strictly decreasing"]),
    ([48, 50], 0.0, ["outside [0,50)"]),
    ([48, 24], -0.1, ["eta", "[0, 1]"]),
    ([48, 24], 1.5, ["eta", "[0, 1]"]),
    ([48, 24], float("nan"), ["eta", "[0, 1]"]),
    ([48, 24], float("inf"), ["eta", "[0, 1]"]),
])
def test_native_rules_are_einval_before_any_gpu_work(t_list, eta, words):
    rc, msg = _coefficients_rc(t_list, eta)
    assert rc == -1, msg
    for w in words:
        assert w in msg, msg
    # the same rule through a sampler call: judged first, with no plan at all
    _, _, alpha_hat = ref.schedule(50)
    steps = np.asarray(t_list, np.int32)
    rule = native.UpdateRule(native.MI_UPDATE["ddim"], eta, 1)
    tabs = (alpha_hat.ctypes.data_as(F32),) * 3
    rc = native.lib().mi_denoise_rule(None, None, None, 1, 32, 32, steps.ctypes.data_as(I32), len(steps), *tabs, 50,
                                      None, 0, 0, 0, 0, C.byref(rule), None, 0, None)
    assert rc == -1 and all(w in native.lib().mi_last_error().decode() for w in words)


def test_native_accepts_what_the_rule_allows():
    assert _coefficients_rc([48, 24, 0], 1.0)[0] == 0
    assert _coefficients_rc([7], 0.25)[0] == 0
    assert _coefficients_rc([], 0.0)[0] == 0
    bad = native.UpdateRule(7, 0.0, 1)
    rc = native.lib().mi_denoise_rule(None, None, None, 1, 32, 32, None, 0, None, None, None, 50, None, 0, 0, 0, 0, C.byref(bad), None, 0, None)
    assert rc == -1 and "unknown update rule" in native.lib().mi_last_error().decode()
    # a NULL rule and the reference kind are the old calls: a missing plan is what they report
    for rule in (None, C.byref(native.UpdateRule(native.MI_UPDATE["reference"], 0.5, 0))):
        rc = native.lib().mi_denoise_rule(None, None, None, 1, 32, 32, None, 0, None, None, None, 50, None, 0, 0, 0, 0, rule, None, 0, None)
        assert rc == -1 and "null plan" in native.lib().mi_last_error().decode()


def test_python_rules():
    assert check_update() is None and check_update("reference", 0.0, True) is None
    rule = check_update("ddim", 0.5, False)
    assert (rule.kind, rule.eta, rule.clip_x0) == (1, 0.5, 0)
    for kw in (dict(update="dpm"), dict(update="ddim", eta=-0.5), dict(update="ddim", eta=1.01), dict(update="ddim", eta=float("nan")),
               dict(update="ddim", eta="1"), dict(update="reference", eta=0.5), dict(update="reference", clip_x0=False), dict(eta=1.0)):
        with pytest.raises(ValueError):
            check_update(**kw)
    refuse_update("reference", "x")
    with pytest.raises(ValueError, match="reference's update only"):
        refuse_update("ddim", "x")

    den = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    x = torch.zeros(1, 1, 32, 32)
    for d in (den, ddim):
        with pytest.raises(ValueError, match="update='ddim'"):
            d.denoise(x, 3, update="reference", eta=0.5)
        with pytest.raises(ValueError, match="update='ddim'"):
            d.denoise_tiled(x, 3, tile=32, update="reference", clip_x0=False)
        with pytest.raises(ValueError, match="eta"):
            d.denoise(x, 3, update="ddim", eta=2.0)
        with pytest.raises(ValueError, match="deterministic"):
            d.denoise_ensemble(x, 3, members=2, seed=1, update="ddim")
        # the calls the rule is not built for name the limitation
        for call in (lambda: d.denoise_ragged(x, [3], update="ddim"),
                     lambda: d.denoise_tiled_ensemble(x, 3, members=2, tile=32, seed=1, update="ddim"),
                     lambda: d.denoise_self_ensemble(x, 3, update="ddim"),
                     lambda: SamplerSession(d, 32, 32, update="ddim"),
                     lambda: d.model.run_slots(x, x.clone(), [[3]], d.beta, d.alpha, d.alpha_hat, clamp_eps=False, update="ddim")):
            with pytest.raises(ValueError, match="reference's update only"):
                call()
        # valid arguments, CPU tensors: never a silent fall-back
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            d.denoise(x, 3, update="ddim", eta=1.0, seed=3)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            d.denoise_ensemble(x, 3, members=2, seed=1, update="ddim", eta=0.5)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            d.denoise_tiled(x, 3, tile=32, update="ddim")
    with pytest.raises(ValueError, match="deterministic"):          # the reference rule's refusal stands
        ddim.denoise_ensemble(x, 3, members=2, seed=1)


def test_cli_flags_parse(monkeypatch):
    from midd_amd import cli
    seen = {}

    class Saved:
        def save(self, *a, **k):
            pass

    def stand_in(*args, **kw):
        seen.update(kw)
        return Saved()

    monkeypatch.setattr(cli, "denoise_image_diffusion", stand_in)
    cli.main(["--image", "nowhere.png"])
    assert (seen["update"], seen["eta"], seen["clip_x0"]) == ("reference", 0.0, True)
    cli.main(["--image", "nowhere.png", "--update", "ddim", "--eta", "0.5", "--no-clip-x0", "--variant", "ddim", "--samples", "4"])
    assert (seen["update"], seen["eta"], seen["clip_x0"], seen["samples"]) == ("ddim", 0.5, False, 4)
    for argv in (["--update", "dpm"], ["--eta", "0.5"], ["--no-clip-x0"], ["--update", "ddim", "--eta", "1.5"],
                 ["--update", "ddim", "--self-ensemble"], ["--update", "ddim", "--variant", "ddim", "--samples", "4"]):
        with pytest.raises(SystemExit):
            cli.main(argv + ["--image", "nowhere.png"])
    monkeypatch.undo()
    with pytest.raises(ValueError, match="update='ddim'"):
        cli.denoise_image_diffusion(None, "nowhere.png", update="reference", eta=0.5)
    with pytest.raises(ValueError, match="self-ensemble"):
        cli.denoise_image_diffusion(None, "nowhere.png", update="ddim", self_ensemble="auto")


def test_service_keeps_the_reference_rule_by_default(monkeypatch):
    from midd_amd.server import DiffusionService
    monkeypatch.delenv("MIDD_UPDATE", raising=False)
    monkeypatch.delenv("MIDD_ETA", raising=False)
    svc = DiffusionService(device=torch.device("cpu"))
    assert (svc.update, svc.eta) == ("reference", 0.0)
    svc = DiffusionService(device=torch.device("cpu"), update="ddim", eta=0.5)
    assert (svc.update, svc.eta) == ("ddim", 0.5)
    monkeypatch.setenv("MIDD_UPDATE", "ddim")
    monkeypatch.setenv("MIDD_ETA", "1")
    svc = DiffusionService(device=torch.device("cpu"))
    assert (svc.update, svc.eta) == ("ddim", 1.0)
    with pytest.raises(ValueError, match="reference's update only"):
        DiffusionService(device=torch.device("cpu"), batch_slots=4)
    monkeypatch.setenv("MIDD_UPDATE", "reference")
    with pytest.raises(ValueError):                                 # eta belongs to update="ddim"
        DiffusionService(device=torch.device("cpu"))

    # the call the service makes: no rule keywords by default, the rule's when it is set
    calls = []

    class Den:
        def denoise(self, x, **kw):
            calls.append(kw)
            return x

    monkeypatch.delenv("MIDD_UPDATE")
    monkeypatch.delenv("MIDD_ETA")
    for kw, want in ((dict(), {"inference_steps": 8}), (dict(update="ddim", eta=0.25), {"inference_steps": 8, "update": "ddim", "eta": 0.25})):
        svc = DiffusionService(device=torch.device("cpu"), **kw)
        svc.diffusion_denoiser = Den()
        svc.process_diffusion(torch.zeros(1, 1, 16, 16), (16, 16))
        assert calls[-1] == want


def test_header_and_binding_declare_the_rule():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    new = {"mi_ddim_coefficients", "mi_denoise_rule", "mi_denoise_ensemble_rule", "mi_denoise_tiled_rule"}
    bound = {n: a for n, _, a in native.SYMBOLS}
    assert new <= declared and new <= set(bound)
    assert "THE DDIM UPDATE" in header and "typedef struct mi_update_rule" in header
    # each *_rule call is its twin plus the rule pointer in front of the workspace
    rule_ptr = C.POINTER(native.UpdateRule)
    for twin in ("mi_denoise_ensemble", "mi_denoise_tiled"):
        assert bound[twin + "_rule"] == bound[twin][:-3] + [rule_ptr] + bound[twin][-3:]
    assert C.sizeof(native.UpdateRule) == 24 and native.UpdateRule.eta.offset == 8 and native.UpdateRule.clip_x0.offset == 16
    assert midd_amd.ddim_coefficients is ddim_coefficients
