"""bench.py's plain run and its --dump-outputs files: the lean headline line, and what the last timed step left its caller."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PARAMS_E1 = 4464961          # RDST-E1 x4 (the flat bucket of tests/test_bench_dp_gpu.py: 4 * 4464961 bytes)


def test_dump_outputs_float32_within_budget_and_repeatable(tmp_path):
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {"loss": torch.tensor(0.25), "params": torch.rand(3000, generator=g), "grads": torch.rand(5000, generator=g).double()}
    bench.dump_outputs(str(tmp_path / "all"), arrays)
    for n, t in arrays.items():
        a = np.load(tmp_path / "all" / f"{n}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, t.float().reshape(-1).numpy())
    budget = 4000 * 4             # half of the data: every array keeps a fixed sample of its elements
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    total = 0
    for n, t in arrays.items():
        a, b = np.load(tmp_path / "s1" / f"{n}.npy"), np.load(tmp_path / "s2" / f"{n}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, b)
        assert np.isin(a, t.float().reshape(-1).numpy()).all()
        total += a.nbytes
    assert total <= budget


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "patches/s" and d["higher_is_better"] is True and d["dtype"] == "bf16" and d["metric"]
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["hip_graph"] is True
    assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) <= 0.01 * d["value"]
    # a plain run measures the headline only: the rest of the line belongs to --full
    for k in ("kernels", "roofline", "roofline_bwd", "fp32_mode", "parity_mode", "configs", "cpu_baseline"):
        assert k not in d, k
    files = {n: np.load(out / f"{n}.npy") for n in ("loss", "params", "grads")}
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(os.path.getsize(out / f"{n}.npy") for n in files) <= 64 * 10 ** 6
    assert files["loss"].shape == (1,) and abs(float(files["loss"][0]) - d["loss"]) <= 1e-5
    assert files["params"].shape == files["grads"].shape == (N_PARAMS_E1,)
    assert np.isfinite(files["params"]).all() and np.isfinite(files["grads"]).all() and np.abs(files["grads"]).max() > 0
