"""The gfx950 assembly of one translation unit of csrc/, for the static ISA checks of the CPU test modules: a test compiles only the
units whose kernels it looks at, and a unit is compiled once per process however many modules ask for it."""
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "medical-image-denoising-using-diffusion_amd", "csrc")


@functools.lru_cache(maxsize=None)
def isa_dump(unit):
    """Assembly text of csrc/<unit> (e.g. "ensemble.hip"), compiled device-only.  A missing hipcc fails: no silent skip."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found: the ISA checks cannot run (they must not be skipped)"
    with tempfile.TemporaryDirectory(prefix="isa") as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-S", "--cuda-device-only", os.path.join(CSRC, unit), "-o", out],
                       check=True, capture_output=True, timeout=1200)
        with open(out) as f:
            return f.read()
