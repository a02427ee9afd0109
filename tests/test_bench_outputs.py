"""bench.py --dump-outputs: what the last timed step computed, written as .npy so that two builds can be compared output for output; and a
plain run (no --full) measures the headline only."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_outputs_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_whole_arrays_under_the_limit(tmp_path):
    bench = load_bench()
    rng = np.random.default_rng(1)
    pos, rho = rng.random((1000, 3), dtype=np.float32), rng.random(1000, dtype=np.float32)
    bench.dump_outputs(str(tmp_path), {"pos": pos, "rho": rho}, {"delta_time": 0.004, "iterations": (2, 9, 3)})
    assert sorted(os.listdir(tmp_path)) == ["delta_time.npy", "iterations.npy", "pos.npy", "rho.npy"]
    assert np.array_equal(np.load(tmp_path / "pos.npy"), pos) and np.load(tmp_path / "pos.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "rho.npy"), rho)
    assert np.load(tmp_path / "iterations.npy").tolist() == [2.0, 9.0, 3.0] and np.load(tmp_path / "delta_time.npy").dtype == np.float64


def test_dump_samples_the_same_particles_above_the_limit(tmp_path, monkeypatch):
    """Over the limit: one fixed, seeded sample of particles for every array, its ids stored next to them, the total within the limit."""
    bench = load_bench()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20000)
    n = 5000
    pos = np.arange(3 * n, dtype=np.float32).reshape(n, 3)
    rho = np.arange(n, dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"pos": pos, "rho": rho}, {"delta_time": 0.004})
    idx = np.load(tmp_path / "a" / "sample_index.npy")
    assert idx.dtype == np.float64 and 0 < len(idx) < n and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "rho.npy"), rho[idx.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "pos.npy"), pos[idx.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 20000          # .npy headers included
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_outputs_repeat(tmp_path):
    """Two plain runs of the same small workload: one line each with the headline fields and none of the --full objects, the
    requested number of timed steps, and the same bits in every dumped array."""
    lines = []
    for d in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "dfsph_small", "--steps", "3", "--warmup", "1",
               "--preroll", "2", "--dump-outputs", str(tmp_path / d)]
        p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        js = [l for l in p.stdout.splitlines() if l.startswith("{")]
        assert len(js) == 1, p.stdout[-2000:]
        lines.append(json.loads(js[0]))
    for d in lines:
        assert d["steps"] == 3 and d["config"]["timed_steps"] == "4-6" and d["ms_per_step"] > 0 and d["dtype"] == "f32"
        assert d["higher_is_better"] is True and d["unit"] == "Mparticle-steps/s" and d["metric"].startswith("million particle-steps/sec")
        assert abs(d["value"] - d["config"]["particles"] * 3 / (d["ms_per_step"] * 3e-3) / 1e6) < 1e-6 * d["value"]
        for key in ("roofline", "kernel_breakdown_us", "relaxed", "strong_scaling_base", "cpu_baseline", "vs_cpu_baseline"):
            assert key not in d, key
    n = lines[0]["config"]["particles"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and {"pos.npy", "vel.npy", "rho.npy", "delta_time.npy", "iterations.npy"} <= set(names)
    assert np.load(tmp_path / "a" / "pos.npy").shape == (n, 3) and np.load(tmp_path / "a" / "rho.npy").shape == (n,)
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.all(np.isfinite(a))
        assert np.array_equal(a, b), f
