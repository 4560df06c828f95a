"""bench.py's result line and --dump-outputs.  CPU tier: the dump of the timed path's outputs (dtypes, the fixed sample of a batch
too large to write whole).  GPU tier: a plain run prints the headline line only, and two runs with the same arguments dump the same
outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _outputs(torch, B, nx=6, nu=2):
    return {"next_state": torch.arange(B * 13, dtype=torch.float32).reshape(B, 13), "status": torch.zeros(B, dtype=torch.int32),
            "iters": torch.arange(B, dtype=torch.int32), "dz": torch.ones(B, nx, nx, dtype=torch.float32), "du": None}


def test_dump_outputs_whole_batch(tmp_path):
    torch = pytest.importorskip("torch")
    import bench
    bench.dump_outputs(str(tmp_path), 0, _outputs(torch, 8), bench.DUMP_LIMIT)
    assert sorted(os.listdir(tmp_path)) == ["dz.npy", "iters.npy", "next_state.npy", "status.npy"]
    assert np.load(tmp_path / "next_state.npy").dtype == np.float32 and np.load(tmp_path / "iters.npy").dtype == np.float64
    assert np.array_equal(np.load(tmp_path / "iters.npy"), np.arange(8))
    bench.dump_outputs(str(tmp_path / "r"), 3, _outputs(torch, 8), bench.DUMP_LIMIT // 4)
    assert "iters.rank3.npy" in os.listdir(tmp_path / "r")


def test_dump_outputs_samples_a_large_batch(tmp_path):
    torch = pytest.importorskip("torch")
    import bench
    B = 1000
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, _outputs(torch, B), 4096)
    envs = np.load(tmp_path / "a" / "envs.npy")
    assert 0 < len(envs) < B and np.all(np.diff(envs) > 0) and np.array_equal(envs, np.load(tmp_path / "b" / "envs.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "iters.npy"), envs)                         # the same environments in every array
    assert np.array_equal(np.load(tmp_path / "a" / "next_state.npy")[:, 0], 13 * envs)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a") if f != "envs.npy") <= 4096 + 5 * 128   # (+ .npy headers)


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_reproducible_outputs(tmp_path):
    lines, B, K = [], 256, 3
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1", "--batch", str(B),
                            "--dump-outputs", str(tmp_path / d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        lines.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    res = lines[0]
    assert res["steps"] == K and res["higher_is_better"] is True and res["unit"] == "env-steps/s" and res["dtype"] == "f64"
    assert abs(res["value"] - B * K / (res["ms_per_step"] * K * 1e-3)) < 1e-6 * res["value"]
    assert not {"roofline", "grad_inf_err_vs_cpu", "cpu_baseline"} & set(res) and "sync_per_step_value" not in res["config"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["du.npy", "dz.npy", "iters.npy", "next_state.npy", "status.npy"] and names == sorted(os.listdir(tmp_path / "b"))
    assert np.load(tmp_path / "a" / "dz.npy").shape[0] == B and np.load(tmp_path / "a" / "dz.npy").dtype == np.float32
    for f in names:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f), equal_nan=True), f
