"""bench.py's own contract: a plain run times the headline alone, --dump-outputs writes what its last timed pass computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_dump_outputs_writes_small_arrays_whole_and_samples_large_ones(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1 << 20)
    field = np.random.default_rng(3).random((1024, 1024, 3), dtype=np.float32)        # 12 MB: past the cap
    steps = np.array([123456789.0])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"field": field, "walk_steps": steps})
    assert np.array_equal(np.load(tmp_path / "a" / "walk_steps.npy"), steps)
    assert not (tmp_path / "a" / "field.npy").exists()
    rows = np.load(tmp_path / "a" / "field_sample_rows.npy")
    sample = np.load(tmp_path / "a" / "field_sample.npy")
    assert rows.dtype == np.float64 and sample.dtype == np.float32 and sample.shape == (len(rows), 3) and len(rows) > 1000
    assert np.array_equal(sample, field.reshape(-1, 3)[rows.astype(np.int64)])
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 1 << 20
    # the same arguments, the same files
    for f in os.listdir(tmp_path / "a"):
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes(), f


def test_steps_must_be_positive():
    import bench
    assert bench.parse_args(["--steps", "5"]).steps == 5 and not bench.parse_args([]).full
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_last_pass(tmp_path, oracle, ladybug):
    """a plain run: no extras, probes or baselines in the line; --steps timed passes; the dumped field and walk-step count
    are the oracle's, bit for bit"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--frame", "64",
                          "--spp", "4", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["metric"] == "walk-steps/s" and r["higher_is_better"] and r["dtype"] == "f32" and r["steps"] == 2
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert not {"configs", "cpu_baseline", "rel_l2_vs_oracle", "time_to_1spp_ms"} & set(r)
    field = np.load(tmp_path / "field.npy")
    assert field.dtype == np.float32 and field.shape == (64, 64, 3)
    ref = oracle.solve(ladybug.as_dict(), 64, 64, 4, ladybug.default_max_depth, ladybug.default_eps, threads=8)
    assert np.array_equal(field.reshape(-1, 3), ref["field"].reshape(-1, 3))
    assert np.load(tmp_path / "walk_steps.npy").tolist() == [float(ref["walk_steps"])]
    assert r["config"]["walk_steps_per_pass"] == ref["walk_steps"]
