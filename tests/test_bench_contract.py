"""Driver contract: bench.py must emit ONE JSON line with the agreed
schema (BASELINE.json metric/config) from rank 0, CPU fallback included."""

import json
import os
import subprocess
import sys

import pytest


@pytest.fixture(autouse=True)
def _cpu_only_bench(monkeypatch):
    """These tests pin the CPU fallback of bench.py: the child processes
    inherit an environment that hides any GPU, so they run the same way
    on a machine that has one."""
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "-1")


def test_bench_json_contract():
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "1", "--warmup", "0",
         "--batch-size", "8"],
        cwd=repo, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "train_samples_per_s"
    assert d["unit"] == "samples/s"
    assert isinstance(d["value"], float) and d["value"] > 0
    assert d["n_gpus"] == 1 and d["steps"] == 1 and d["warmup"] == 0
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["vs_baseline"] is None
    assert d["data"] == "synthetic"
    assert d["config"]["model"] == "tiger-amazon-beauty"
    assert d["config"]["global_batch"] == 8
    assert d["config"]["parallelism"] == "dp1"
    assert d["config"]["hip_graph"] is False  # no GPU here
    assert d["config"]["seq_len"] == 61
    assert isinstance(d["ms_per_step"], float)


def test_bench_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's loss/grads/params as
    float32 .npy (<= 64 MB in all); same arguments => same arrays. --full
    is accepted and keeps the one-line result contract."""
    import numpy as np

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
             "--warmup", "1", "--batch-size", "4", "--full",
             "--dump-outputs", str(d)],
            cwd=repo, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout
        res = json.loads(lines[0])
        assert res["steps"] == 2 and res["ms_per_step"] > 0
        assert sorted(os.listdir(d)) == ["grads.npy", "loss.npy",
                                         "params.npy"]
        dumps.append({f[:-4]: np.load(d / f) for f in os.listdir(d)})
    a, b = dumps
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    for k in a:
        assert a[k].dtype == np.float32 and a[k].size > 0
        assert np.isfinite(a[k]).all()
        # fp32 on CPU: allow only a few ulps for thread-order effects
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-6,
                                   err_msg=k)
    assert a["loss"].shape == (1,) and np.abs(a["grads"]).max() > 0


def test_bench_world2_gloo_contract():
    """The driver's torchrun launch shape: 2 ranks over gloo on CPU; ONE
    JSON line from rank 0 with n_gpus=2 and the global batch."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29531", "bench.py", "--gpus", "2",
         "--steps", "1", "--warmup", "0", "--batch-size", "4"],
        cwd=repo, capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 8
