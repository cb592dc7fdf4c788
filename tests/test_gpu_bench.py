"""bench.py on the GPU: a plain run prints the headline fields only, and --dump-outputs writes what the timed path returned
(checked against the CPU oracle on the same seeded weights and images)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from midd_amd import UNetConfig, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_timed_output(tmp_path):
    out_dir = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "0",
           "--batch-per-gpu", "2", "--size", "64", "--inference-steps", "2", "--dump-outputs", str(out_dir)]
    proc = subprocess.run(cmd, cwd=str(tmp_path), stdout=subprocess.PIPE, text=True, timeout=300)
    assert proc.returncode == 0
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    res = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in res, key
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["unit"] == "images/s"
    assert not {"roofline", "cpu_baseline", "latency_batch1"} & set(res)          # --full legs only

    got = np.load(out_dir / "denoised.npy")
    assert got.dtype == np.float32 and got.shape == (2, 1, 64, 64)
    cfg = UNetConfig()
    sd = make_state_dict(cfg, seed=42)
    noisy = torch.from_numpy(synthetic_xray(2, 64, 64, seed=1234))
    want = orc.denoise(orc.to_torch(sd), topology(cfg), noisy, noise_steps=50, inference_steps=2)
    assert float(np.abs(got - want.numpy()).max()) < 1e-3
