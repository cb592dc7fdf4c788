#!/usr/bin/env python3
"""Records the Python surface of the package as JSON: tests/golden/python_surface.json, which tests/test_python_surface_cpu.py
replays against the working tree.  CPU only: no GPU and no compute call of libmidd.so (the host-only tile geometry is called).

    python tools/dump_python_surface.py [OUT.json]        # default: tests/golden/python_surface.json

Three parts.
  modules   every name of ``midd_amd`` and ``midd_amd.sampler`` that does not start with ``__``: callables with their signature
            and the SHA-256 of their docstring, NamedTuples with their ``_fields`` as well, modules by their name, everything else
            (the constants) by its ``repr`` -- except a ``torch.device``, which depends on the machine and is recorded as a kind only.
  classes   ``DiffusionDenoiser`` and ``UNetDiffusion``: every public method the class itself defines (the ``run_*`` and
            ``*_workspace_bytes`` methods among them), signature and docstring hash.
  refusals  calls on CPU tensors -- ``UNetDiffusion(**SMALL)`` of both variants, ``noise_steps=50`` -- as Python expressions over the
            names of ``namespace()``, each with the exception type and the whole message it raises.  Per call: every argument broken
            alone, every adjacent pair of the call's order of checks broken together (the first of the two is the one reported: that
            pins the order), and the call with nothing broken, which ends at "no CPU fallback".  Stored as ``calls`` (a call's valid
            keywords), ``outcomes`` (the distinct [type, message] pairs) and ``refusals`` (rows [call, outcome, cases]: every case,
            put over the valid keywords, raises that outcome); ``replay`` turns the rows back into expressions.

The file is a record of the commit it was generated at (``generated_at``); it is never regenerated from code it is meant to judge.

Raises of ``DiffusionDenoiser`` and of the ``run_*`` preambles that no CPU tensor reaches, because ``_check_image`` refuses the
tensor's device first:
  * ``_check_image``: "must be float32";
  * ``run_sampler`` / ``_run_slots`` / ``_step_noise``: the step_noise shape rule, and everything of ``_run_slots`` after
    ``_check_image(cond)`` (x against cond, iter_base, sample_index, member, frame, t_before / t_after);
  * ``run_slots_rule``: nothing (its own rules come before the image check);
  * ``run_denoising_loss``: "noisy must match clean", and ``check_loss_source`` / ``loss_table_args`` / ``loss_counter_args`` through
    it (they are reached through the stand-alone ``noise_images`` instead);
  * ``run_self_ensemble`` and ``run_tiled_self_ensemble``: "nothing to return" (they judge the image before the outputs);
  * ``run_tiled``, ``run_tiled_ensemble``, ``run_tiled_self_ensemble``: the tiling's own refusals (``tiling`` follows the image
    check; the ``*_workspace_bytes`` methods, which take no tensor, reach them);
  * ``run_sampler``: "pass either seed or step_noise" is reachable only by a direct call (``denoise`` refuses first): recorded so;
  * ``denoise_tiled`` / ``run_tiled``: "it takes no seed" of run_tiled likewise.
"""
from __future__ import annotations

import hashlib
import inspect
import json
import os
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "python_surface.json")
SMALL = dict(model_channels=16, time_emb_dim=64)
MODULES = ("midd_amd", "midd_amd.sampler")
CLASSES = ("DiffusionDenoiser", "UNetDiffusion")


def load():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import midd_loader
    return midd_loader.load()


def _doc_hash(obj):
    doc = inspect.getdoc(obj)
    return None if doc is None else hashlib.sha256(doc.encode()).hexdigest()


def _signature(obj):
    try:
        return str(inspect.signature(obj))
    except (TypeError, ValueError):
        return None


def describe(obj) -> dict:
    import torch
    if isinstance(obj, types.ModuleType):
        return {"kind": "module", "name": obj.__name__}
    if isinstance(obj, torch.device):
        return {"kind": "torch.device"}
    if isinstance(obj, property):
        return {"kind": "property", "doc": _doc_hash(obj)}
    if isinstance(obj, (staticmethod, classmethod)):
        obj = obj.__func__
    if inspect.isclass(obj) and issubclass(obj, tuple) and hasattr(obj, "_fields"):
        return {"kind": "namedtuple", "fields": list(obj._fields), "signature": _signature(obj), "doc": _doc_hash(obj)}
    if inspect.isclass(obj) or inspect.isroutine(obj):
        return {"kind": "callable", "signature": _signature(obj), "doc": _doc_hash(obj)}
    return {"kind": "constant", "repr": repr(obj)}


def module_names(name: str) -> dict:
    mod = sys.modules[name]
    return {n: describe(v) for n, v in sorted(vars(mod).items()) if not n.startswith("__")}


def class_methods(cls) -> dict:
    return {n: describe(v) for n, v in sorted(vars(cls).items()) if not n.startswith("_")}


# ------------------------------------------------------------------------------ the refusal table
def namespace() -> dict:
    """The names the refusal expressions are written over."""
    load()
    import torch
    from midd_amd import DiffusionDenoiser, SamplerRule, UNetDiffusion, timestep_list
    import midd_amd
    ns = {"torch": torch, "m": midd_amd, "SamplerRule": SamplerRule, "nan": float("nan")}
    for variant in ("ddim", "cddpm"):
        ns[variant] = DiffusionDenoiser(UNetDiffusion(variant=variant, **SMALL), noise_steps=50)
    ns.update(X=torch.zeros(2, 1, 16, 24), XS=torch.zeros(2, 1, 16, 16), X3=torch.zeros(2, 16, 24), XC=torch.zeros(2, 3, 16, 24),
              X64=torch.zeros(2, 1, 16, 24, dtype=torch.float64), T=timestep_list(50, 3),
              BETA=ns["ddim"].beta, ALPHA=ns["ddim"].alpha, AHAT=ns["ddim"].alpha_hat)
    return ns


def _cases(target: str, base: dict, order: list, extra: list = ()) -> list:
    """The cases (target, base, keywords) of one call: each entry of ``order`` (keywords as source text) alone, each adjacent pair
    together, the ``extra`` ones (off the main order: another branch of the call), and the call with nothing broken."""
    return [(target, base, kw) for kw in list(order) + [dict(a, **b) for a, b in zip(order, order[1:])] + list(extra) + [{}]]


def expression(target: str, base, kw) -> str:
    """The Python expression of a case: ``base`` with the keywords ``kw`` put over it, or, for a ``base`` of None, ``kw`` as the
    argument text itself."""
    if base is None:
        return f"{target}({kw})"
    return f"{target}({', '.join(f'{k}={v}' for k, v in dict(base, **kw).items())})"


UPDATE = [dict(update="'bogus'"), dict(eta="2.0"), dict(clip_x0="'yes'"), dict(eta="0.5"), dict(update="'dpmpp2m'", eta="0.25")]
REFUSED = [dict(update="'bogus'"), dict(update="'dpmpp2m'"), dict(update="'ddim'")]
LEVELS = [dict(quantiles="'x'"), dict(quantiles="()"), dict(quantiles="(0.5, 2.0)")]
MEMBERS = [dict(members="0"), dict(member_offset="-1"), dict(max_batch="0"), dict(member_offset="2**32 - 1", members="2")]
OFFSETS = [dict(member_offset="-1"), dict(max_batch="0"), dict(member_offset="2**32 - 1")]
SEED = [dict(seed="-1"), dict(seed="1", sample_offset="-1")]
VIEWS = [dict(views="'bogus'"), dict(views="7"), dict(views="()"), dict(views="(0, True)"), dict(views="(0, 9)"), dict(views="(1, 1)")]


def refusal_cases() -> list:
    img = dict(noisy_img="X", inference_steps="3")
    run = dict(noisy="X", t_list="T", beta="BETA", alpha="ALPHA", alpha_hat="AHAT")
    out = []
    # ---- DiffusionDenoiser.denoise
    order = UPDATE + [dict(return_x0="True"), dict(seed="1", step_noise="torch.zeros(1)"), dict(seed="-1"), dict(seed="1", sample_offset="-1"),
                      dict(inference_steps="0"), dict(seed="1", member="-1"), dict(member="1"), dict(seed="1", noisy_img="X3")]
    extra = [dict(noisy_img="None"), dict(seed="1"), dict(seed="1", member="2"), dict(seed="1", member="2", noisy_img="X3"),
             dict(update="'ddim'"), dict(update="'ddim'", eta="0.5"), dict(update="'ddim'", eta="0.5", seed="1", member="1"),
             dict(update="'ddim'", return_x0="True"),
             dict(update="'dpmpp2m'"), dict(update="'dpmpp2m'", return_x0="True"), dict(update="'dpmpp2m'", seed="1"),
             dict(update="'dpmpp2m'", step_noise="torch.zeros(1)"), dict(update="'dpmpp2m'", member="1"),
             dict(update="'dpmpp2m'", inference_steps="0"), dict(update="'dpmpp2m'", noisy_img="X3"), dict(update="'dpmpp2m'", clip_x0="False")]
    for v in ("cddpm", "ddim"):
        out += _cases(f"{v}.denoise", img, order, extra)
    # ---- denoise_ensemble
    order = LEVELS + UPDATE[:3] + [dict(update="'dpmpp2m'"), dict(update="'ddim'"), dict(seed="-1"), dict(quantiles="(0.5,)", members="65"),
                                    dict(quantiles="(0.5,)", members="0"), dict(inference_steps="0"), dict(seed="1", sample_offset="-1")] \
        + MEMBERS + [dict(noisy_img="X3")]
    extra = [dict(update="'ddim'", eta="0.5"), dict(update="'ddim'", eta="0.5", members="0"), dict(quantiles="(0.1, 0.9)", return_samples="True")]
    out += _cases("cddpm.denoise_ensemble", img, order, extra)
    out += _cases("ddim.denoise_ensemble", img, [dict(quantiles="'x'"), dict(update="'bogus'"), dict(update="'ddim'"), dict(seed="-1")],
                  [dict(update="'ddim'", eta="0.5"), dict(update="'ddim'", eta="0.5", seed="-1")])
    # ---- denoise_tiled
    tiled = dict(img, tile="8", overlap="2")
    order = UPDATE + [dict(update="'dpmpp2m'", seed="1"), dict(step_noise="torch.zeros(1)"), dict(seed="-1"), dict(seed="1", sample_offset="-1"),
                      dict(inference_steps="0"), dict(max_batch="0"), dict(noisy_img="X3")]
    extra = [dict(update="'dpmpp2m'"), dict(update="'ddim'"), dict(update="'ddim'", eta="0.5"), dict(update="'ddim'", eta="0.5", seed="-1"),
             dict(seed="1"), dict(tile="0"), dict(tile="64"), dict(overlap="-1"), dict(sample_offset="-1")]
    out += _cases("cddpm.denoise_tiled", tiled, order, extra)
    order = UPDATE + [dict(update="'dpmpp2m'", seed="1"), dict(step_noise="torch.zeros(1)"), dict(seed="1"), dict(inference_steps="0"),
                      dict(max_batch="0"), dict(noisy_img="X3")]
    out += _cases("ddim.denoise_tiled", tiled, order, extra)
    # ---- denoise_tiled_ensemble
    order = REFUSED + LEVELS + [dict(step_noise="torch.zeros(1)"), dict(seed="-1"), dict(quantiles="(0.5,)", members="65"),
                                dict(inference_steps="0"), dict(seed="1", sample_offset="-1")] + MEMBERS + [dict(noisy_img="X3")]
    out += _cases("cddpm.denoise_tiled_ensemble", tiled, order, [dict(tile="0"), dict(quantiles="(0.5,)", return_tiles="True")])
    out += _cases("ddim.denoise_tiled_ensemble", tiled, [dict(update="'ddim'"), dict(quantiles="'x'"), dict(step_noise="torch.zeros(1)"), dict(seed="-1")])
    # ---- denoise_self_ensemble
    order = REFUSED + LEVELS + VIEWS + [dict(views="(4,)"), dict(seed="-1"), dict(inference_steps="0"), dict(sample_offset="-1"),
                                        dict(noisy_img="X3")] + OFFSETS + [dict(noisy_img="XC")]
    extra = [dict(noisy_img="XS", views="(4,)"), dict(noisy_img="XS", views="'d4'"), dict(views="'d4'"), dict(views="'flips'"),
             dict(noisy_img="X3", views="'bogus'"), dict(quantiles="(0.5,)"), dict(noisy_img="None")]
    out += _cases("cddpm.denoise_self_ensemble", img, order, extra)
    order = REFUSED + LEVELS + [dict(seed="1")] + VIEWS + [dict(views="(4,)"), dict(inference_steps="0"), dict(sample_offset="-1"),
                                                          dict(noisy_img="X3")] + OFFSETS + [dict(noisy_img="XC")]
    out += _cases("ddim.denoise_self_ensemble", img, order, extra)
    # ---- denoise_tiled_self_ensemble
    order = UPDATE[:3] + [dict(update="'dpmpp2m'")] + LEVELS + [dict(tile="0"), dict(overlap="-1")] + VIEWS \
        + [dict(tile="(8, 16)", views="(4,)"), dict(seed="-1"), dict(seed="1", sample_offset="-1"), dict(inference_steps="0"), dict(noisy_img="X3")] \
        + OFFSETS + [dict(noisy_img="XC")]
    extra = [dict(eta="0.5"), dict(views="(4,)"), dict(overlap="(2, 4)", views="'d4'"), dict(update="'ddim'"), dict(update="'ddim'", eta="0.5"),
             dict(update="'ddim'", eta="0.5", seed="-1"), dict(noisy_img="X3", views="'bogus'"), dict(tile="64"), dict(quantiles="(0.5,)")]
    out += _cases("cddpm.denoise_tiled_self_ensemble", tiled, order, extra)
    order = UPDATE[:3] + [dict(update="'dpmpp2m'")] + LEVELS + [dict(seed="1"), dict(tile="0"), dict(overlap="-1")] + VIEWS \
        + [dict(tile="(8, 16)", views="(4,)"), dict(inference_steps="0"), dict(sample_offset="-1"), dict(noisy_img="X3")] + OFFSETS + [dict(noisy_img="XC")]
    out += _cases("ddim.denoise_tiled_self_ensemble", tiled, order, extra + [dict(update="'ddim'", seed="1")])
    # ---- score_ensemble, ensemble_nps
    score = dict(clean="X", noisy="X", inference_steps="3")
    order = [dict(quantiles="(0.5, 2.0)"), dict(members="0"), dict(members="65"), dict(clean="X3"), dict(clean="X64"), dict(seed="-1"),
             dict(sample_offset="-1"), dict(max_batch="0")]
    extra = [dict(clean="None"), dict(quantiles="None"), dict(quantiles="()"), dict(tile="8", overlap="2"), dict(tile="8", overlap="2", seed="-1"),
             dict(tile="8", overlap="2", member_offset="-1"), dict(tile="0")]
    out += _cases("cddpm.score_ensemble", score, order, extra)
    out += _cases("ddim.score_ensemble", score, [dict(members="65")], [dict(tile="8", overlap="2")])
    nps = dict(noisy="X", inference_steps="3")
    order = [dict(members="0"), dict(members="1"), dict(roi="48"), dict(step="0"), dict(detrend="'bogus'"), dict(window="'bogus'"),
             dict(window="(1.0, 2.0)"), dict(seed="-1"), dict(sample_offset="-1"), dict(max_batch="0")]
    out += _cases("cddpm.ensemble_nps", nps, order, extra[3:])
    out += _cases("ddim.ensemble_nps", nps, [dict(members="1")], [dict(tile="8", overlap="2")])
    # ---- the training objective
    order = [dict(x="X3"), dict(x="X64"), dict(seed="1", noise="X"), dict(seed="1", sample_offset="-1"), dict(seed="1", draw="-1"),
             dict(seed="-1"), dict(noise="XS"), dict(t="(1,)"), dict(t="(1, 50)")]
    out += _cases("ddim.noise_images", dict(x="X", t="(1, 2)"), order, [dict(x="None"), dict(x="None", seed="1"), dict(seed="1"), dict(noise="X")])
    order = [dict(clean="X3"), dict(seed="1", noise="X"), dict(edge_weight="nan"), dict(clean="XC")]
    extra = [dict(clean="None"), dict(t="(1, 2)"), dict(seed="1"), dict(noise="X"), dict(edge_weight="0.5"), dict(return_maps="True")]
    for v in ("ddim", "cddpm"):
        out += _cases(f"{v}.denoising_loss", dict(clean="X", noisy="X"), order, extra)
    order = [dict(clean="X3"), dict(timesteps="(1, 50)"), dict(timesteps="(1, True)"), dict(max_batch="0"), dict(seed="-1"), dict(sample_offset="-1"),
             dict(edge_weight="nan"), dict(clean="XC", noisy="XC")]
    out += _cases("ddim.loss_profile", dict(clean="X", noisy="X", timesteps="(1, 2)"), order, [dict(clean="None"), dict(timesteps="None")])
    # ---- denoise_ragged
    ragged = dict(noisy_img="X", inference_steps="(3, 5)")
    order = REFUSED + [dict(rule="'ddim'"), dict(inference_steps="(3,)"), dict(seed="-1"), dict(sample_offset="-1"), dict(inference_steps="(3, -1)"),
                       dict(inference_steps="(3, 0)")]
    extra = [dict(noisy_img="X3"), dict(noisy_img="None"), dict(noisy_img="torch.zeros(())"), dict(rule="SamplerRule()"),
             dict(rule="SamplerRule('ddim', 0.5)"), dict(rule="SamplerRule('ddim', 0.5)", seed="-1"), dict(rule="SamplerRule('dpmpp2m')"),
             dict(rule="SamplerRule('dpmpp2m')", seed="-1"), dict(rule="SamplerRule()", sample_offset="-1"), dict(noisy_img="XC", inference_steps="(3, 5)")]
    out += _cases("cddpm.denoise_ragged", ragged, order, extra)
    order = REFUSED + [dict(rule="'ddim'"), dict(inference_steps="(3,)"), dict(sample_offset="-1"), dict(inference_steps="(3, -1)"),
                       dict(inference_steps="(3, 0)")]
    out += _cases("ddim.denoise_ragged", ragged, order, extra + [dict(seed="-1")])
    # ---- UNetDiffusion.run_*: the five batched calls
    ens = dict(run, clamp_eps="False", members="4", seed="1")
    order = UPDATE + [dict(update="'dpmpp2m'"), dict(seed="-1"), dict(sample_offset="-1")] + MEMBERS \
        + [dict(want_mean="False", want_std="False"), dict(noisy="X3")]
    extra = [dict(members="1", want_mean="False"), dict(want_mean="False", want_std="False", want_samples="True"), dict(seed="None"),
             dict(update="'ddim'"), dict(update="'ddim'", eta="0.5"), dict(noisy="XC"), dict(noisy="None")]
    out += _cases("cddpm.model.run_ensemble", ens, order, extra)
    selfe = dict(run, clamp_eps="True")
    order = REFUSED + [dict(seed="-1"), dict(sample_offset="-1"), dict(noisy="X3")] + VIEWS + [dict(views="(4,)")] + OFFSETS + [dict(noisy="XC")]
    extra = [dict(want_mean="False", want_std="False"), dict(seed="1"), dict(levels="(0.5,)"), dict(noisy="XS", views="'d4'"), dict(noisy="None"),
             dict(views="(3,)", member_offset="2**32 - 1")]
    for v in ("ddim", "cddpm"):
        out += _cases(f"{v}.model.run_self_ensemble", selfe, order, extra)
    til = dict(run, clamp_eps="True", tile="8", overlap="2")
    order = UPDATE + [dict(update="'dpmpp2m'", seed="1"), dict(seed="-1"), dict(seed="1", sample_offset="-1"), dict(max_batch="0"), dict(noisy="X3")]
    extra = [dict(sample_offset="-1"), dict(update="'dpmpp2m'"), dict(update="'ddim'", eta="0.5", seed="1"), dict(tile="0"), dict(tile="64"),
             dict(want_tiles="True"), dict(noisy="XC"), dict(noisy="None")]
    out += _cases("ddim.model.run_tiled", til, order, extra)
    tens = dict(til, clamp_eps="False", members="3", seed="1")
    order = REFUSED + [dict(seed="-1"), dict(sample_offset="-1")] + MEMBERS \
        + [dict(want_mean="False", want_std="False"), dict(noisy="X3")]
    extra = [dict(members="1", want_mean="False"), dict(want_mean="False", want_std="False", want_tiles="True"), dict(seed="None"), dict(tile="0"),
             dict(noisy="XC"), dict(noisy="None")]
    out += _cases("cddpm.model.run_tiled_ensemble", tens, order, extra)
    order = UPDATE[:3] + [dict(update="'dpmpp2m'"), dict(seed="-1"), dict(sample_offset="-1"), dict(noisy="X3"), dict(tile="0"), dict(overlap="-1")] \
        + VIEWS + [dict(tile="(8, 16)", views="(4,)")] + OFFSETS + [dict(noisy="XC")]
    extra = [dict(eta="0.5"), dict(want_mean="False", want_std="False"), dict(seed="1"), dict(update="'ddim'", eta="0.5", seed="1"), dict(tile="64"),
             dict(views="(4,)"), dict(noisy="None")]
    for v in ("ddim", "cddpm"):
        out += _cases(f"{v}.model.run_tiled_self_ensemble", til, order, extra)
    # ---- the workspace queries (no tensor: the tiling is judged, then the model's device)
    out += ["ddim.model.workspace_bytes(2, 16, 24)", "ddim.model.ensemble_workspace_bytes(2, 4, 16, 24)",
            "ddim.model.self_ensemble_workspace_bytes(2, 4, 16, 24)"]
    for name, head in (("tiled_workspace_bytes", "2"), ("tiled_ensemble_workspace_bytes", "2, 3"), ("tiled_self_ensemble_workspace_bytes", "2, 4")):
        out += [f"ddim.model.{name}({head}, 16, 24, {t})" for t in ("tile=8, overlap=2", "tile=0", "tile=64", "tile=8, overlap=-1", "tile=8, overlap=5")]
    # ---- the other run_* calls
    samp = dict(run, clamp_eps="True")
    order = UPDATE + [dict(return_x0="True"), dict(update="'dpmpp2m'", seed="1"), dict(seed="1", member="-1"), dict(seed="1", step_noise="torch.zeros(1)"),
                      dict(seed="-1"), dict(seed="1", sample_offset="-1"), dict(member="1"), dict(noisy="X3")]
    extra = [dict(seed="1"), dict(seed="1", member="2"), dict(update="'dpmpp2m'"), dict(update="'dpmpp2m'", return_x0="True"),
             dict(update="'ddim'", eta="0.5", seed="1", member="2"), dict(noisy="XC"), dict(noisy="None")]
    out += _cases("cddpm.model.run_sampler", samp, order, extra)
    slots = dict(cond="X", x="X.clone()", t_rows="[[40, 40], [20, 20]]", beta="BETA", alpha="ALPHA", alpha_hat="AHAT", clamp_eps="True")
    order = REFUSED + [dict(seed="1", step_noise="torch.zeros(1)"), dict(seed="-1"), dict(cond="X3"), dict(x="X3")]
    out += _cases("ddim.model.run_slots", slots, order, [dict(seed="1"), dict(max_slots="4")])
    order = [dict(rule="'ddim'"), dict(rule="SamplerRule('dpmpp2m')", x0="X.clone()", seed="1"), dict(rule="SamplerRule('dpmpp2m')"),
             dict(t_before="[-1, -1]"), dict(rule="SamplerRule('dpmpp2m')", x0="XS"), dict(rule="SamplerRule('dpmpp2m')", x0="X.clone()", x="X3"),
             dict(seed="1", step_noise="torch.zeros(1)"), dict(seed="-1"), dict(cond="X3")]
    extra = [dict(rule="SamplerRule()", x0="X.clone()"), dict(rule="SamplerRule()"), dict(rule="SamplerRule('dpmpp2m')", x0="X.clone()"),
             dict(rule="SamplerRule('dpmpp2m')", x0="None", member="[0, 0]"), dict(rule="SamplerRule('ddim', 0.5)", seed="1", t_after="[-1, -1]")]
    out += _cases("ddim.model.run_slots_rule", slots, order, extra)
    loss = dict(clean="X", noisy="X", t="(1, 2)", alpha_hat="AHAT", clamp_eps="True", edge_weight="0.2", seed="1")
    out += _cases("ddim.model.run_denoising_loss", loss, [dict(clean="X3"), dict(clean="XC")], [dict(seed="None", noise="X"), dict(seed="None")])
    out += ["ddim.model.forward(X, X, torch.zeros(2))", "ddim.model.forward(X3, X, torch.zeros(2))", "ddim.model(X, X, torch.zeros(2))"]
    # ---- the stand-alone operators: their tensor rules (the tile-count rule follows the device rule: no CPU tensor reaches it)
    t5, t6, v5 = "torch.zeros(2, 6, 1, 8, 8)", "torch.zeros(4, 2, 6, 1, 8, 8)", "torch.zeros(2, 4, 1, 16, 24)"
    out += ["m.step_noise(1, 3, (2, 1, 16, 24), device='cpu')", "m.step_noise(-1, 3, (2, 1, 16, 24), device='cpu')",
            "m.step_noise(1, 3, (2, 1, 16, 24), member=-1, device='cpu')", "m.step_noise(1, 3, (2, 1, 16), device='cpu')",
            "m.ensemble_reduce(X)", "m.ensemble_reduce(X3[0])", "m.ensemble_reduce(None)", "m.ensemble_reduce(X64)", "m.ensemble_reduce(X[:0])",
            "m.ensemble_quantiles(X, (0.5,))", "m.ensemble_quantiles(X, 'x')", "m.ensemble_quantiles(X3[0], (0.5,))", "m.ensemble_quantiles(None, (0.5,))",
            "m.ensemble_quantiles(torch.zeros(1, 65, 4), 0.5)", "m.ensemble_quantiles(X64, 0.5)",
            "m.ensemble_scores(X, X[:, 0])", "m.ensemble_scores(X3[0], X)", "m.ensemble_scores(X, X)", "m.ensemble_scores(X, X[:, 0], (2.0,))",
            "m.ensemble_scores(torch.zeros(1, 65, 4), torch.zeros(1, 4))", "m.ensemble_scores(X64, X64[:, 0])",
            "m.noise_power_spectrum(torch.zeros(64, 64))", "m.noise_power_spectrum(torch.zeros(64, 64), roi=48)", "m.noise_power_spectrum(X3)",
            "m.noise_power_spectrum(X, roi=32)", "m.noise_power_spectrum(torch.zeros(64, 64), X)", "m.noise_power_spectrum(torch.zeros(64, 64), scale=nan)",
            "m.tile_extract(X, 8, 2)", "m.tile_extract(X3, 8, 2)", "m.tile_extract(None, 8)", "m.tile_extract(X[:0], 8)", "m.tile_extract(X64, 8)",
            f"m.tile_blend({t5}, 16, 24, 2)", "m.tile_blend(X, 16, 24, 2)", "m.tile_blend(None, 16, 24)",
            f"m.tile_blend_reduce({t6}, 16, 24, 2)", f"m.tile_blend_reduce({t5}, 16, 24, 2)",
            f"m.tile_blend_quantiles({t6}, 16, 24, 2, (0.5,))", f"m.tile_blend_quantiles({t6}, 16, 24, 2)", f"m.tile_blend_quantiles({t6}, 16, 24, 2, 'x')",
            f"m.tile_blend_quantiles({t5}, 16, 24, 2, (0.5,))", "m.tile_blend_quantiles(torch.zeros(65, 1, 1, 1, 8, 8), 8, 8, 2, (0.5,))",
            "m.dihedral_views(X)", "m.dihedral_views(X3)", "m.dihedral_views(None)", "m.dihedral_views(X, 'bogus')", "m.dihedral_views(X, 'd4')",
            "m.dihedral_views(X64)", "m.dihedral_views(X[:0])",
            f"m.dihedral_reduce({v5})", f"m.dihedral_reduce({v5}, (0, 1))", f"m.dihedral_reduce({v5}, 'd4')", "m.dihedral_reduce(X)", "m.dihedral_reduce(None)",
            f"m.dihedral_quantiles({v5}, q=(0.5,))", f"m.dihedral_quantiles({v5})", f"m.dihedral_quantiles({v5}, q='x')",
            f"m.dihedral_quantiles({v5}, (0, 1), (0.5,))", "m.dihedral_quantiles(X, q=(0.5,))",
            f"m.tile_blend_unview_reduce({t6}, 16, 24, 2)", f"m.tile_blend_unview_reduce({t6}, 16, 24, 2, (0, 1))", f"m.tile_blend_unview_reduce({t5}, 16, 24, 2)",
            f"m.tile_blend_unview_reduce({t6}, 16, 24, (2, 4), (4,) * 4)", f"m.tile_blend_unview_reduce({t6}, 0, 24, 2)",
            f"m.tile_blend_unview_quantiles({t6}, 16, 24, 2, q=(0.5,))", f"m.tile_blend_unview_quantiles({t6}, 16, 24, 2)",
            f"m.tile_blend_unview_quantiles({t6}, 16, 24, 2, q='x')", f"m.tile_blend_unview_quantiles({t6}, 16, 24, 2, (0, 1), (0.5,))",
            "m.noise_images(X, (1, 2), AHAT, seed=1)", "m.noise_images(X3, (1, 2), AHAT, seed=1)", "m.noise_images(X, (1, 2), AHAT)",
            "m.noise_images(X, (1, 2), AHAT, seed=1, sample_index=(0,))", "m.noise_images(X, (1, 2), AHAT, noise=X, draws=(0, 0))",
            "m.noise_images(X, (1, 2), AHAT, seed=1, draws=(0, -1))",
            "m.loss_terms(X, X, (1, 2), AHAT, seed=1)", "m.loss_terms(X, XS, (1, 2), AHAT, seed=1)", "m.loss_terms(X, X64, (1, 2), AHAT, seed=1)",
            "m.loss_terms(X, X, (1, 2), AHAT, seed=1, x_t=X)", "m.loss_terms(X, X, (1, 2), AHAT, noise=X)", "m.loss_terms(X, X, (1, 2), AHAT, noise=X, x_t=XS)",
            "m.loss_terms(X, X, (1, 2), AHAT, noise=X, x_t=X)", "m.loss_terms(X3, X, (1, 2), AHAT, seed=1)"]
    seen, uniq = set(), []
    for c in out:
        if isinstance(c, str):      # a call written out: its name and its argument text
            target, _, args = c.partition("(")
            c = (target, None, args[:-1])
        if expression(*c) not in seen:
            seen.add(expression(*c))
            uniq.append(c)
    return uniq


def evaluate(expr: str, ns: dict) -> list:
    """One refusal: [the exception type, its whole message] (a call that returns: [None, None])."""
    try:
        eval(expr, dict(ns))
    except Exception as e:      # noqa: BLE001  (the type is what is recorded)
        return [type(e).__name__, str(e)]
    return [None, None]


def refusal_table(outcome_of) -> dict:
    """The refusal table as the file holds it.  ``calls``: every call's valid keywords (None: its cases are argument text);
    ``outcomes``: the distinct [exception type, message] pairs; ``refusals``: rows [call, outcome index, cases], each case the
    keywords put over the valid ones -- every case of a row raises that row's outcome.  ``outcome_of(expression)`` answers."""
    calls, outcomes, rows = {}, [], {}
    for target, base, kw in refusal_cases():
        assert calls.setdefault(target, base) == base, target
        got = outcome_of(expression(target, base, kw))
        if got not in outcomes:
            outcomes.append(got)
        rows.setdefault((target, outcomes.index(got)), []).append(kw)
    return {"calls": calls, "outcomes": outcomes, "refusals": [[t, i, kws] for (t, i), kws in rows.items()]}


def replay(golden: dict):
    """-> (call expression, recorded outcome) of every case in a recorded table."""
    for target, index, cases in golden["refusals"]:
        for kw in cases:
            yield expression(target, golden["calls"][target], kw), golden["outcomes"][index]


def snapshot() -> dict:
    load()
    import midd_amd
    import midd_amd.sampler      # noqa: F401
    ns = namespace()
    return dict({"modules": {m: module_names(m) for m in MODULES},
                 "classes": {c: class_methods(getattr(midd_amd, c)) for c in CLASSES}}, **refusal_table(lambda e: evaluate(e, ns)))


def write(snap: dict, path: str) -> None:
    """One line per name, method, call, outcome and refusal row: a diff of the file reads as a list of what changed."""
    def one(v):
        return json.dumps(v)      # (keywords keep their order: it is the order of the call's arguments)
    parts = [f' "generated_at": {one(snap["generated_at"])}']
    for part in ("modules", "classes"):
        owners = [f"  {one(o)}: {{\n" + ",\n".join(f"   {one(n)}: {one(d)}" for n, d in names.items()) + "\n  }" for o, names in snap[part].items()]
        parts.append(f' "{part}": {{\n' + ",\n".join(owners) + "\n }")
    parts.append(' "calls": {\n' + ",\n".join(f"  {one(t)}: {one(b)}" for t, b in snap["calls"].items()) + "\n }")
    for part in ("outcomes", "refusals"):
        parts.append(f' "{part}": [\n' + ",\n".join(f"  {one(r)}" for r in snap[part]) + "\n ]")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(parts) + "\n}\n")


def _generated_at() -> str:
    def git(*a):
        return subprocess.run(("git", "-C", ROOT) + a, capture_output=True, text=True, check=True).stdout.strip()
    try:
        dirty = git("status", "--porcelain", "--", "medical-image-denoising-using-diffusion_amd")
        return git("rev-parse", "HEAD") + (" (package modified)" if dirty else "")
    except (OSError, subprocess.CalledProcessError):
        return "unknown"


def main(argv) -> int:
    out = argv[1] if len(argv) > 1 else DEFAULT_OUT
    snap = dict(generated_at=_generated_at(), **snapshot())
    write(snap, out)
    print(f"{out}: " + ", ".join(f"{len(v)} names in {m}" for m, v in snap["modules"].items())
          + f"; {sum(len(r[2]) for r in snap['refusals'])} refusals, {len(snap['outcomes'])} distinct outcomes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
