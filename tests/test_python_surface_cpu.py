"""CPU-only: the Python surface of the package is what tests/golden/python_surface.json recorded (tools/dump_python_surface.py, run
at the commit the file names in ``generated_at``): every name of ``midd_amd`` and ``midd_amd.sampler`` with its signature, fields,
value and docstring, the public methods of ``DiffusionDenoiser`` and ``UNetDiffusion``, and for every recorded call on CPU tensors
the exception type and the whole message.  Nothing here may be skipped: an entry that cannot be replayed fails."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_spec = importlib.util.spec_from_file_location("dump_python_surface", os.path.join(ROOT, "tools", "dump_python_surface.py"))
surface = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(surface)

with open(os.path.join(ROOT, "tests", "golden", "python_surface.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_record_is_whole():
    assert len(GOLDEN["modules"]["midd_amd.sampler"]) == 85 and len(GOLDEN["modules"]["midd_amd"]) == 53
    assert set(GOLDEN["classes"]) == {"DiffusionDenoiser", "UNetDiffusion"}
    calls = [call for call, _ in surface.replay(GOLDEN)]
    assert len(calls) == len(set(calls)) > 800
    assert all(raises is not None for raises, _ in GOLDEN["outcomes"])      # nothing on a CPU tensor returns


@pytest.mark.parametrize("module", sorted(GOLDEN["modules"]))
def test_every_recorded_name_is_there_and_unchanged(module):
    surface.load()
    import midd_amd.sampler      # noqa: F401
    now = surface.module_names(module)
    want = GOLDEN["modules"][module]
    missing = sorted(set(want) - set(now))
    assert not missing, f"{module} lost {missing}"
    changed = {n: (want[n], now[n]) for n in want if now[n] != want[n]}
    assert not changed, changed


@pytest.mark.parametrize("cls", sorted(GOLDEN["classes"]))
def test_every_recorded_method_is_there_and_unchanged(cls):
    surface.load()
    import midd_amd
    now = surface.class_methods(getattr(midd_amd, cls))
    want = GOLDEN["classes"][cls]
    missing = sorted(set(want) - set(now))
    assert not missing, f"{cls} lost {missing}"
    changed = {n: (want[n], now[n]) for n in want if now[n] != want[n]}
    assert not changed, changed


@pytest.fixture(scope="module")
def namespace():
    return surface.namespace()


def test_every_recorded_refusal_is_raised_again(namespace):
    wrong = [(call, want, got) for call, want in surface.replay(GOLDEN) for got in [surface.evaluate(call, namespace)] if got != want]
    assert not wrong, f"{len(wrong)} refusals changed; the first: {wrong[:3]}"


def test_the_tool_still_writes_the_calls_of_the_record():
    """The table's expressions are the tool's: a case dropped from the tool would otherwise go on being replayed from the file only."""
    assert sorted(surface.expression(*c) for c in surface.refusal_cases()) == sorted(call for call, _ in surface.replay(GOLDEN))


def test_modules_imports_without_sampler():
    """``midd_amd.modules`` stands on the rules, tiling and views modules: a fresh interpreter can import it with ``midd_amd.sampler``
    absent (a None entry in sys.modules makes any import of it fail), and no package module is imported inside a function."""
    code = ("import sys, types, importlib.util, midd_loader\n"
            "spec = importlib.util.spec_from_file_location(midd_loader.ALIAS, midd_loader.PKG_DIR + '/__init__.py',\n"
            "                                              submodule_search_locations=[midd_loader.PKG_DIR])\n"
            "pkg = importlib.util.module_from_spec(spec)      # the package without running its __init__, which imports the sampler\n"
            "sys.modules[midd_loader.ALIAS] = pkg\n"
            "sys.modules['midd_amd.sampler'] = None\n"
            "import midd_amd.modules\n"
            "m = midd_amd.modules.UNetDiffusion(model_channels=16, time_emb_dim=64)\n"
            "try:\n"
            "    m.tiled_workspace_bytes(1, 16, 16, tile=0)\n"
            "except ValueError as e:\n"
            "    print('refused:', e)\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert "refused: tile must be in [1, 2**31) (got 0)" in out.stdout
    plain = subprocess.run([sys.executable, "-c", "import midd_loader; midd_loader.load(); import midd_amd.modules"], cwd=ROOT,
                           capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    with open(os.path.join(ROOT, "medical-image-denoising-using-diffusion_amd", "modules.py")) as f:
        lines = f.read().splitlines()
    assert not [ln for ln in lines if "from .sampler import" in ln]
    assert not [ln for ln in lines if ln.startswith(" ") and ln.lstrip().startswith(("from . import", "from .", "import midd_amd"))]
