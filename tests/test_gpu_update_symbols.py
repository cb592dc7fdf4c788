"""GPU: the out-conv kernel symbol a profiled sampler call reports, for every update the sampler can run (mi_profile_begin /
mi_profile_end; out_conv.hip: out_conv_symbol).  The names feed tools/ddim_update_ab.py and tools/dpm_update_ab.py.

One two-iteration call, the list 40, 20 of a 50-step schedule (both t > 0, so both rows of the reference rule draw), with
MI_NO_SPLIT (one program: a launch per iteration), is bracketed per update.  Its out-conv entries must be exactly the expected
symbols with the expected instantiation, <1> for one image channel and <0> for the run-time channel count, 2 launches in all.
Five of the six updates run one symbol twice.  The seeded DDIM(eta) call cannot: after the last entry of a list sigma is 0 whatever
eta is (include/midd.h: THE DDIM UPDATE), nothing is drawn there, and that row runs out_conv_ddim_kernel -- so its two launches are
one of out_conv_ddim_seeded_kernel and one of out_conv_ddim_kernel.

Networks: the 16-wide one-channel network at 8 x 8, the smallest image its four levels accept (tests/test_gpu_parity.py runs it
there), B = 2; and NET2 of tests/test_gpu_multichannel.py at that module's 40 x 24."""
import pytest
import torch

from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion
from midd_amd.weights import make_state_dict, synthetic_xray
from tests.test_gpu_multichannel import NETS, images_np

pytestmark = pytest.mark.gpu

SEED = 0x1234567890ABCDEF
NOISE_STEPS = 50
T_LIST = [40, 20]
CASES = {"SMALL": (dict(model_channels=16, time_emb_dim=64), (2, 8, 8), "<1>"), "NET2": (NETS["NET2"], (2, 40, 24), "<0>")}
SYMBOLS = ["out_conv_kernel", "out_conv_seeded_kernel", "out_conv_ddim_kernel", "out_conv_ddim_seeded_kernel", "out_conv_dpm_kernel",
           "out_conv_slots_kernel"]

_dens = {}


def _den(net):
    if net not in _dens:
        kw = CASES[net][0]
        sd = make_state_dict(UNetConfig(variant="cddpm", **kw), seed=42)
        m = UNetDiffusion(variant="cddpm", **kw)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        _dens[net] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=NOISE_STEPS)
    return _dens[net]


def _out_conv_launches(den, call):
    """-> {symbol with its instantiation: launches} of the out-conv entries of one profiled call."""
    den.model.profile_begin()
    try:
        call()
        torch.cuda.synchronize()
    finally:
        entries = den.model.profile_end()
    return {e["name"].split("midd::")[-1]: e["launches"] for e in entries if "out_conv" in e["name"]}


@pytest.mark.parametrize("update,expected", [
    ("reference_tensor", {"out_conv_kernel": 2}),
    ("reference_seeded", {"out_conv_seeded_kernel": 2}),
    ("ddim_tensor", {"out_conv_ddim_kernel": 2}),
    ("ddim_seeded", {"out_conv_ddim_seeded_kernel": 1, "out_conv_ddim_kernel": 1}),      # (the last row draws nothing: module docstring)
    ("dpm", {"out_conv_dpm_kernel": 2}),
    ("slots", {"out_conv_slots_kernel": 2}),
])
@pytest.mark.parametrize("net", list(CASES))
def test_profile_reports_the_out_conv_symbol_that_ran(net, update, expected):
    den = _den(net)
    _, (B, H, W), inst = CASES[net]
    channels = den.model.cfg.in_channels
    cond = torch.from_numpy(images_np(channels, B, H, W) if channels > 1 else synthetic_xray(B, H, W, seed=77)).cuda()
    tabs = (den.beta, den.alpha, den.alpha_hat)
    gen = torch.Generator().manual_seed(11)
    noise = (0.5 * torch.randn((len(T_LIST),) + tuple(cond.shape), generator=gen)).cuda()
    run = den.model.run_sampler
    calls = {
        "reference_tensor": lambda: run(cond, T_LIST, *tabs, clamp_eps=False, step_noise=noise, no_split=True),
        "reference_seeded": lambda: run(cond, T_LIST, *tabs, clamp_eps=False, seed=SEED, no_split=True),
        "ddim_tensor": lambda: run(cond, T_LIST, *tabs, clamp_eps=False, step_noise=noise, no_split=True, update="ddim", eta=0.5),
        "ddim_seeded": lambda: run(cond, T_LIST, *tabs, clamp_eps=False, seed=SEED, no_split=True, update="ddim", eta=0.5),
        "dpm": lambda: run(cond, T_LIST, *tabs, clamp_eps=False, no_split=True, update="dpmpp2m"),
        "slots": lambda: den.model.run_slots(cond, cond.clone(), [[t] * B for t in T_LIST], *tabs, clamp_eps=False, seed=SEED, no_split=True),
    }
    got = _out_conv_launches(den, calls[update])
    print(f"{net} {update}: {got}")
    assert got == {name + inst: n for name, n in expected.items()}, got
    assert sum(got.values()) == 2 and all(k[:-3] in SYMBOLS for k in got)
