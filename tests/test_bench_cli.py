"""bench.py's launch contract on CPU: `--gpus N` never silently runs fewer GPUs
(`--gpus` was parsed and ignored).  Without torchrun it spawns N rank
processes itself, which here (no GPU) must stop with a non-zero status before any
rank starts; under a launcher whose WORLD_SIZE disagrees it refuses."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _run(args, env_extra=None):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=300)


def test_gpus_more_than_visible_fails_loudly():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert "GPU" in r.stderr and "--gpus 2" in r.stderr


def test_gpus_disagreeing_with_launcher_world_size_fails():
    r = _run(["--gpus", "4", "--steps", "1"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


def test_full_and_dump_outputs_are_options_and_zero_steps_is_refused():
    r = _run(["--help"])
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs DIR" in r.stdout
    r = _run(["--gpus", "1", "--steps", "0"])
    assert r.returncode == 2 and "--steps" in r.stderr


HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"}
FULL_ONLY = {"p50_ms", "roofline", "pipeline_ms", "roofline_timing", "cpu_baseline", "serving",
             "metric_workload_10m_x_128", "config_c3", "config_c4", "config_c5"}


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_steps_outputs(tmp_path):
    """A plain run (here c1, 10K x 384, batch 1) times exactly --steps steps, carries none of the
    --full figures, and --dump-outputs writes what the timed search returned: the dumped row ids
    and scores are the CPU oracle's exact top-k over the same seeded inputs."""
    import bench
    from oracle import ref_cpu
    out = tmp_path / "dump"
    r = _run(["--gpus", "1", "--config", "c1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert HEADLINE <= set(rec) and not (FULL_ONLY & set(rec)), sorted(rec)
    assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["unit"] == "queries/s" and rec["higher_is_better"] is True
    N, D, B, k, metric, _ = bench.CONFIGS["c1"]
    # value and ms_per_step describe the same 7 timed steps
    assert rec["value"] == pytest.approx(B * 1e3 / rec["ms_per_step"], rel=1e-9)
    assert sorted(p.name for p in out.iterdir()) == ["indices.npy", "scores.npy"]
    idx, sc = np.load(out / "indices.npy"), np.load(out / "scores.npy")
    assert idx.dtype == np.float64 and sc.dtype == np.float32 and idx.shape == sc.shape == (B, k)
    V = bench.corpus_rows(N, D, 0, N)
    Q = np.random.default_rng(1).random((B, D), dtype=np.float32)
    es, ei, _ = ref_cpu.exact_search(Q, V, k, metric)
    np.testing.assert_array_equal(idx, ei.astype(np.float64))
    np.testing.assert_array_equal(sc, es)
