"""CPU-only checks of the second-order multistep update rule (include/midd.h: THE DPMPP2M UPDATE): the exported coefficient
table against the DDIM table and the numpy restatement (tests/dpm_update_reference.py), the restated loop against an exact
solution on Gaussian data and on a perfect predictor, and the argument rules of the C ABI, the Python calls, the CLI and the
service.  What the device computes is judged in test_gpu_dpm_update.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, SamplerSession, SamplerTrajectory, UNetDiffusion, native, timestep_list
from midd_amd.sampler import check_update, ddim_coefficients, dpm_coefficients, refuse_update
from tests import ddim_update_reference as ddim_ref
from tests import dpm_update_reference as ref

SMALL = dict(model_channels=16, time_emb_dim=64)
I32, F32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
_, _, ALPHA_HAT = ref.schedule(50)
TABLE_LISTS = [[24], [48, 24], [48, 36, 24], [48, 24, 18], timestep_list(50, 5), timestep_list(50, 8), timestep_list(50, 50)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("t_list", TABLE_LISTS, ids=lambda t: f"n{len(t)}_{t[0]}_{t[-1]}")
def test_exported_table_against_the_ddim_table_and_the_restatement(t_list):
    """Columns 0-6 are mi_ddim_coefficients at eta = 0 bit for bit; g is the restatement's within 1 fp32 ulp -- two `log`
    implementations may differ in the last place of a double, every other operation is correctly rounded on both sides."""
    got = dpm_coefficients(t_list, ALPHA_HAT)
    want = ref.coefficients(t_list, ALPHA_HAT)
    assert got.dtype == np.float32 and got.shape == (len(t_list), 8)
    assert np.array_equal(_bits(got[:, :7]), _bits(ddim_coefficients(t_list, ALPHA_HAT, 0.0)))
    assert np.array_equal(_bits(got[:, :7]), _bits(want[:, :7])) and not got[:, 6].any()
    g, wg = got[:, 7], want[:, 7]
    ulps = np.abs(_bits(g).astype(np.int64) - _bits(wg).astype(np.int64))
    print(f"list of {len(t_list)}: g = {g.tolist()}, max ulp distance to the restatement {int(ulps.max())}")
    assert int(ulps.max()) <= 1
    assert _bits(g[:1])[0] == 0 and _bits(g[-1:])[0] == 0              # exactly +0 on the first and the last row
    assert (g[1:-1] > 0).all()


def test_the_bound_on_the_extrapolation_weight():
    """[48, 36, 24]: r = 0.78 < 1, the bound is in force; [48, 24, 18]: r = 2.66, it is free."""
    assert ref.timestep_list(50, 8) == timestep_list(50, 8) and len(timestep_list(50, 8)) == 9
    r = float(ref.step_ratio([48, 36, 24], ALPHA_HAT, 1))
    g = float(dpm_coefficients([48, 36, 24], ALPHA_HAT)[1, 7])
    free = float(ref.weight([48, 36, 24], ALPHA_HAT, 1, bounded=False))
    assert abs(r - 0.78) < 0.005 and abs(g - 0.16575) < 5e-6 and abs(g * 1.0 - free * r) < 1e-7 and free > g
    r = float(ref.step_ratio([48, 24, 18], ALPHA_HAT, 1))
    g = float(dpm_coefficients([48, 24, 18], ALPHA_HAT)[1, 7])
    free = float(ref.weight([48, 24, 18], ALPHA_HAT, 1, bounded=False))
    assert abs(r - 2.66) < 0.005 and abs(g - 0.04596) < 5e-6 and abs(g - free) < 1e-8
    # the jump in log-SNR at t = 0 that the bound answers: the last real step of the 9-entry list
    served = timestep_list(50, 8)
    assert float(ref.step_ratio(served, ALPHA_HAT, len(served) - 2)) < 0.3


def _coefficients_rc(t_list, noise_steps=50, out=True, tab=True):
    steps = np.asarray(t_list, np.int32)
    buf = np.zeros((max(1, len(steps)), 8), np.float32)
    rc = native.lib().mi_dpm_coefficients(steps.ctypes.data_as(I32), len(steps), ALPHA_HAT.ctypes.data_as(F32) if tab else None,
                                          noise_steps, buf.ctypes.data_as(F32) if out else None)
    return rc, native.lib().mi_last_error().decode()


@pytest.mark.parametrize("t_list,words", [
    ([24, 24], ["strictly decreasing"]),
    ([24, 48], ["strictly decreasing"]),
    ([48, 24, 30], ["strictly decreasing"]),
    ([48, 50], ["outside [0,50)"]),
    ([-1], ["outside [0,50)"]),
])
def test_native_list_rules_are_einval_before_any_gpu_work(t_list, words):
    rc, msg = _coefficients_rc(t_list)
    assert rc == -1 and all(w in msg for w in words), msg
    # the same rule through the sampler calls: judged first, with no plan at all
    steps = np.asarray(t_list, np.int32)
    tabs = (ALPHA_HAT.ctypes.data_as(F32),) * 3
    rc = native.lib().mi_denoise_dpm(None, None, None, None, 1, 1, 32, 32, steps.ctypes.data_as(I32), len(steps), *tabs, 50, 0, 1, None, 0, None)
    assert rc == -1 and all(w in native.lib().mi_last_error().decode() for w in words)
    rc = native.lib().mi_denoise_tiled_dpm(None, None, None, None, None, 1, 32, 32, 32, 32, 0, 0, steps.ctypes.data_as(I32), len(steps),
                                           *tabs, 50, 1, 0, 1, None, 0, None)
    assert rc == -1 and all(w in native.lib().mi_last_error().decode() for w in words)


def test_native_argument_rules():
    assert _coefficients_rc([48, 24, 0])[0] == 0 and _coefficients_rc([7])[0] == 0 and _coefficients_rc([])[0] == 0
    assert _coefficients_rc([48, 24], out=False)[0] == -1 and _coefficients_rc([48, 24], tab=False)[0] == -1
    assert _coefficients_rc([48, 24], noise_steps=0)[0] == -1
    lib = native.lib()
    steps = np.asarray([48, 36, 24], np.int32)
    tabs = (ALPHA_HAT.ctypes.data_as(F32),) * 3
    # x0_slots: 1 or n_iters, nothing else
    for slots in (0, 2, 4, -1):
        rc = lib.mi_denoise_dpm(None, None, None, None, slots, 1, 32, 32, steps.ctypes.data_as(I32), 3, *tabs, 50, 0, 1, None, 0, None)
        assert rc == -1 and "x0_slots" in lib.mi_last_error().decode()
    for slots in (1, 3):                                    # allowed: the missing plan is what is reported
        rc = lib.mi_denoise_dpm(None, None, None, None, slots, 1, 32, 32, steps.ctypes.data_as(I32), 3, *tabs, 50, 0, 1, None, 0, None)
        assert rc == -1 and "null plan" in lib.mi_last_error().decode()
    # the rule handed to the calls that have no buffer: MI_EINVAL, naming the new calls; kind 7 stays unknown
    for fn, args in ((lib.mi_denoise_rule, (None, None, None, 1, 32, 32, steps.ctypes.data_as(I32), 3, *tabs, 50, None, 0, 0, 0, 0)),
                     (lib.mi_denoise_ensemble_rule, (None, None, None, None, None, 1, 2, 32, 32, steps.ctypes.data_as(I32), 3, *tabs, 50, 0, 0, 0, 2, 0)),
                     (lib.mi_denoise_tiled_rule, (None, None, None, None, 1, 32, 32, 32, 32, 0, 0, steps.ctypes.data_as(I32), 3, *tabs, 50, 0, 0, 0, 1, 0))):
        rc = fn(*args, C.byref(native.UpdateRule(native.MI_UPDATE["dpmpp2m"], 0.0, 1)), None, 0, None)
        msg = lib.mi_last_error().decode()
        assert rc == -1 and "mi_denoise_dpm" in msg and "mi_denoise_tiled_dpm" in msg, msg
        rc = fn(*args, C.byref(native.UpdateRule(7, 0.0, 1)), None, 0, None)
        assert rc == -1 and "unknown update rule" in lib.mi_last_error().decode()
    assert native.MI_UPDATE["dpmpp2m"] == 2


# ------------------------------------------------------------------------------ 2. the restated loop on Gaussian data
XT_CASES = [0.9, 0.05]
DATA_CASES = [(0.4, 0.25), (0.7, 0.1), (0.2, 0.5)]
RATIO_BOUND = {5: 0.8, 8: 0.6, 12: 0.45, 25: 0.2, 50: 0.15}


def _gaussian_errors(inference_steps):
    """Data N(mu, s^2): the network's exact answer is eps = sqrt(1-A) (x - sqrt(A) mu) / (A s^2 + 1-A), and the probability-flow
    ODE started at x_T ends at mu + (x_T - sqrt(A_T) mu) s / sqrt(A_T s^2 + 1-A_T).  -> per case (|error| under this rule, under
    DDIM eta = 0, under the textbook 2M weight), no clip."""
    t_list = ref.timestep_list(50, inference_steps)
    A_T = np.float64(ALPHA_HAT[t_list[0]])
    out = []
    for x_T in XT_CASES:
        for mu, s in DATA_CASES:
            def eps(x, t):
                A = np.float64(ALPHA_HAT[t])
                return (np.sqrt(1.0 - A) * (x.astype(np.float64) - np.sqrt(A) * mu) / (A * s * s + 1.0 - A)).astype(np.float32)

            exact = mu + (x_T - np.sqrt(A_T) * mu) * s / np.sqrt(A_T * s * s + 1.0 - A_T)
            start = np.full((1,), x_T, np.float32)
            mine = float(ref.loop(start, t_list, ALPHA_HAT, eps, clamp_eps=False, clip_x0=False)[0][0])
            first = float(ddim_ref.loop(start, t_list, ALPHA_HAT, 0.0, eps, clamp_eps=False, clip_x0=False)[0])
            book = float(ref.loop(start, t_list, ALPHA_HAT, eps, clamp_eps=False, clip_x0=False, bounded=False)[0][0])
            out.append((abs(mine - exact), abs(first - exact), abs(book - exact)))
    return out


@pytest.mark.parametrize("inference_steps", sorted(RATIO_BOUND))
def test_restated_loop_beats_ddim_on_gaussian_data(inference_steps):
    """Endpoint error under this rule / under DDIM eta = 0, in each of the 6 cases, below 0.8 / 0.6 / 0.45 / 0.2 / 0.15 on the
    lists of inference_steps 5 / 8 / 12 / 25 / 50 (conditions; the restatement gives 0.72 / 0.53 / 0.37 / 0.16 / 0.10)."""
    errs = _gaussian_errors(inference_steps)
    ratios = [m / f for m, f, _ in errs]
    book = [b / f for _, f, b in errs]
    print(f"inference_steps {inference_steps}: worst error ratio to DDIM {max(ratios):.3f} (textbook weight: {max(book):.3f}); "
          f"worst |error| {max(m for m, _, _ in errs):.2e} against DDIM's {max(f for _, f, _ in errs):.2e}")
    assert all(f > 1e-4 for _, f, _ in errs)               # DDIM's own error is far above fp32 rounding: the ratio means something
    assert max(ratios) < RATIO_BOUND[inference_steps]


def test_textbook_weight_is_worse_than_ddim_on_the_short_lists():
    """Why the weight is bounded: unbounded, the rule loses to DDIM in some case of the 5- and 9-entry lists."""
    for steps in (5, 8):
        assert max(b / f for _, f, b in _gaussian_errors(steps)) > 1.0


# ------------------------------------------------------------------------------ 3. the perfect predictor
@pytest.mark.parametrize("inference_steps", [5, 8, 50])
@pytest.mark.parametrize("clip_x0", [True, False])
def test_restated_loop_returns_the_image_a_perfect_predictor_points_at(inference_steps, clip_x0):
    """eps(x, t) = (x - sqrt(A) x*) / sqrt(1 - A) predicts x0 = x* at every step, so x0 - x0_prev is rounding alone and the loop
    ends at x* within 1e-6 (measured 6e-8); every slot of the trajectory is x* within the same bound."""
    t_list = timestep_list(50, inference_steps)
    rng = np.random.default_rng(7)
    star = rng.random((2, 1, 40, 24)).astype(np.float32)
    star[0, 0, :3] = 0.0
    star[1, 0, -3:] = 1.0                                # the ends of the range: the clip's own values
    start = (star + 0.3 * rng.standard_normal(star.shape)).astype(np.float32)

    def eps(x, t):
        A = np.float64(ALPHA_HAT[t])
        return ((x.astype(np.float64) - np.sqrt(A) * star) / np.sqrt(1.0 - A)).astype(np.float32)

    out, traj = ref.loop(start, t_list, ALPHA_HAT, eps, clamp_eps=False, clip_x0=clip_x0)
    err = float(np.abs(out.astype(np.float64) - star).max())
    err_traj = float(np.abs(traj.astype(np.float64) - star).max())
    print(f"fixed point, list of {len(t_list)}, clip {clip_x0}: max|x - x*| = {err:.2e}, over the trajectory {err_traj:.2e}")
    assert out.dtype == np.float32 and traj.shape == (len(t_list),) + star.shape
    assert err <= 1e-6 and err_traj <= 1e-6


# ------------------------------------------------------------------------------ 4. interfaces
def test_python_rules():
    rule = check_update("dpmpp2m", 0.0, False)
    assert (rule.kind, rule.eta, rule.clip_x0) == (2, 0.0, 0)
    assert check_update("dpmpp2m").clip_x0 == 1
    with pytest.raises(ValueError, match="deterministic"):
        check_update("dpmpp2m", 0.5)
    with pytest.raises(ValueError):
        check_update(update="dpm")                       # the rule's name is dpmpp2m
    with pytest.raises(ValueError, match="update='ddim'"):
        check_update("reference", 0.5)
    with pytest.raises(ValueError, match="update='ddim'"):
        check_update("reference", 0.0, False)
    with pytest.raises(ValueError, match="reference's update only"):
        refuse_update("dpmpp2m", "x")

    x = torch.zeros(1, 1, 32, 32)
    for variant in ("cddpm", "ddim"):
        d = DiffusionDenoiser(UNetDiffusion(variant=variant, **SMALL), noise_steps=50)
        for kw in (dict(eta=0.5), dict(seed=3), dict(step_noise=torch.zeros(4, 1, 1, 32, 32)), dict(seed=3, member=1), dict(member=1)):
            with pytest.raises(ValueError, match="deterministic"):
                d.denoise(x, 3, update="dpmpp2m", **kw)
        for kw in (dict(), dict(update="ddim"), dict(update="ddim", eta=1.0, seed=1)):
            with pytest.raises(ValueError, match="return_x0"):
                d.denoise(x, 3, return_x0=True, **kw)
        with pytest.raises(ValueError, match="deterministic"):
            d.denoise_ensemble(x, 3, members=2, seed=1, update="dpmpp2m")
        with pytest.raises(ValueError, match="deterministic"):
            d.model.run_ensemble(x, [24, 12], d.beta, d.alpha, d.alpha_hat, False, members=2, seed=1, update="dpmpp2m")
        with pytest.raises(ValueError, match="deterministic"):
            d.denoise_tiled(x, 3, tile=32, update="dpmpp2m", seed=1)
        with pytest.raises(ValueError, match="deterministic"):
            d.denoise_tiled(x, 3, tile=32, update="dpmpp2m", eta=0.5)
        for call in (lambda: d.denoise_ragged(x, [3], update="dpmpp2m"),
                     lambda: d.denoise_tiled_ensemble(x, 3, members=2, tile=32, seed=1, update="dpmpp2m"),
                     lambda: d.denoise_self_ensemble(x, 3, update="dpmpp2m"),
                     lambda: SamplerSession(d, 32, 32, update="dpmpp2m"),
                     lambda: d.model.run_slots(x, x.clone(), [[3]], d.beta, d.alpha, d.alpha_hat, clamp_eps=False, update="dpmpp2m")):
            with pytest.raises(ValueError, match="reference's update only"):
                call()
        # valid arguments, CPU tensors: never a silent fall-back
        for call in (lambda: d.denoise(x, 3, update="dpmpp2m"), lambda: d.denoise(x, 3, update="dpmpp2m", clip_x0=False, return_x0=True),
                     lambda: d.denoise_tiled(x, 3, tile=32, update="dpmpp2m")):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_cli_flags_parse(monkeypatch, tmp_path):
    from midd_amd import cli
    seen = {}

    class Saved:
        def save(self, *a, **k):
            pass

    def stand_in(*args, **kw):
        seen.clear()
        seen.update(kw)
        return Saved()

    monkeypatch.setattr(cli, "denoise_image_diffusion", stand_in)
    cli.main(["--image", "nowhere.png", "--update", "dpmpp2m"])
    assert (seen["update"], seen["eta"], seen["clip_x0"]) == ("dpmpp2m", 0.0, True) and "x0_out" not in seen
    cli.main(["--image", "nowhere.png", "--update", "dpmpp2m", "--no-clip-x0", "--x0-out", "traj.npy", "--variant", "ddim"])
    assert (seen["update"], seen["clip_x0"], seen["x0_out"]) == ("dpmpp2m", False, "traj.npy")
    cli.main(["--image", "nowhere.png", "--update", "dpmpp2m", "--tile", "64"])
    assert (seen["update"], seen["tile"]) == ("dpmpp2m", 64)
    for argv in (["--update", "dpm"], ["--update", "dpmpp2m", "--eta", "0.5"], ["--update", "dpmpp2m", "--seed", "3"],
                 ["--update", "dpmpp2m", "--samples", "4"], ["--update", "dpmpp2m", "--self-ensemble"],
                 ["--x0-out", "traj.npy"], ["--update", "ddim", "--x0-out", "traj.npy"],
                 ["--update", "dpmpp2m", "--tile", "64", "--x0-out", "traj.npy"]):
        with pytest.raises(SystemExit):
            cli.main(argv + ["--image", "nowhere.png"])
    monkeypatch.undo()
    with pytest.raises(ValueError, match="deterministic"):
        cli.denoise_image_diffusion(None, "nowhere.png", update="dpmpp2m", eta=0.5)
    with pytest.raises(ValueError, match="deterministic"):
        cli.denoise_image_diffusion(None, "nowhere.png", update="dpmpp2m", seed=3)
    with pytest.raises(ValueError, match="self-ensemble"):
        cli.denoise_image_diffusion(None, "nowhere.png", update="dpmpp2m", self_ensemble="auto")
    with pytest.raises(ValueError, match="x0-out"):
        cli.denoise_image_diffusion(None, "nowhere.png", update="ddim", x0_out=str(tmp_path / "t.npy"))


def test_service_takes_the_rule(monkeypatch):
    from midd_amd.server import DiffusionService, create_app
    monkeypatch.delenv("MIDD_UPDATE", raising=False)
    monkeypatch.delenv("MIDD_ETA", raising=False)
    svc = DiffusionService(device=torch.device("cpu"), update="dpmpp2m")
    assert (svc.update, svc.eta) == ("dpmpp2m", 0.0)
    with pytest.raises(ValueError, match="deterministic"):
        DiffusionService(device=torch.device("cpu"), update="dpmpp2m", eta=0.5)
    with pytest.raises(ValueError, match="reference's update only"):
        DiffusionService(device=torch.device("cpu"), update="dpmpp2m", batch_slots=4)
    monkeypatch.setenv("MIDD_UPDATE", "dpmpp2m")
    svc = DiffusionService(device=torch.device("cpu"))
    assert svc.update == "dpmpp2m"
    monkeypatch.setenv("MIDD_UPDATE", "dpm")
    with pytest.raises(ValueError):
        DiffusionService(device=torch.device("cpu"))
    monkeypatch.delenv("MIDD_UPDATE")

    # the call the service makes: the rule alone, no eta
    calls = []

    class Den:
        def denoise(self, x, **kw):
            calls.append(kw)
            return x

    svc = DiffusionService(device=torch.device("cpu"), update="dpmpp2m")
    svc.diffusion_denoiser = Den()
    svc.process_diffusion(torch.zeros(1, 1, 16, 16), (16, 16))
    assert calls[-1] == {"inference_steps": 8, "update": "dpmpp2m"}

    # /health reports the rule
    import asyncio
    for update in ("dpmpp2m", "reference"):
        app = create_app(DiffusionService(device=torch.device("cpu"), update=update))
        route = next(r for r in app.routes if getattr(r, "path", None) == "/health")
        assert asyncio.run(route.endpoint())["update"] == update


def test_header_and_binding_declare_the_rule():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    new = {"mi_dpm_coefficients", "mi_denoise_dpm", "mi_denoise_tiled_dpm"}
    bound = {n: a for n, _, a in native.SYMBOLS}
    assert new <= declared and new <= set(bound)
    assert "THE DPMPP2M UPDATE" in header and re.search(r"#define\s+MI_UPDATE_DPMPP2M\s+2\b", header)
    # mi_denoise_dpm is mi_denoise with the buffer and its slot count after x_out, and clip_x0 in the place of step_noise's slot
    plain = bound["mi_denoise"]
    assert bound["mi_denoise_dpm"] == plain[:3] + [C.c_void_p, C.c_int] + plain[3:-5] + [C.c_int, C.c_int] + plain[-3:]
    assert midd_amd.dpm_coefficients is dpm_coefficients and SamplerTrajectory._fields == ("image", "x0")
