"""bench.py --dump-outputs and --full: the dump writes float32 arrays (token ids as float64), keeps within its 64 MB budget by a fixed,
seeded sample, and a plain run of the decode workload dumps the last timed step's logits beside the ids they choose; two plain runs
with the same arguments dump the same arrays."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_writes_float32_and_float64_ids(tmp_path):
    b = _bench()
    b.dump_outputs(str(tmp_path), {"logits": np.arange(12, dtype=np.float32).reshape(3, 4).astype(np.float16), "next_ids": [7, 2**40 + 1]})
    lo, ids = np.load(tmp_path / "logits.npy"), np.load(tmp_path / "next_ids.npy")
    assert lo.dtype == np.float32 and lo.shape == (3, 4) and np.array_equal(lo, np.arange(12, dtype=np.float32).reshape(3, 4))
    assert ids.dtype == np.float64 and ids.tolist() == [7.0, float(2**40 + 1)]


def test_dump_samples_an_output_beyond_the_budget_the_same_way_every_time(tmp_path):
    b = _bench()
    big = np.random.default_rng(3).normal(size=(b.DUMP_LIMIT_BYTES // 4 + 1000,)).astype(np.float32)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), {"hidden": big})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["hidden_sample.npy", "hidden_sample_index.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= b.DUMP_LIMIT_BYTES
    s, idx = np.load(tmp_path / "a" / "hidden_sample.npy"), np.load(tmp_path / "a" / "hidden_sample_index.npy")
    assert np.array_equal(s, big[idx.astype(np.int64)]) and np.all(np.diff(idx) > 0)
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


def test_full_and_dump_outputs_are_options():
    p = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout


def _plain(out_dir):
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "6", "--warmup", "2", "--layers", "2", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_and_repeats_it(tmp_path):
    a = _plain(tmp_path / "a")
    assert a["steps"] == 6 and a["ms_per_step"] > 0 and a["runner"].startswith("host") and a["blocks"]["count"] == 1
    assert a.get("roofline") is None and "cpu_baseline" not in a and "extra" not in a   # --full only
    lo, ids = np.load(tmp_path / "a" / "logits.npy"), np.load(tmp_path / "a" / "next_ids.npy")
    assert lo.dtype == np.float32 and lo.shape[0] == ids.shape[0] == a["config"]["global_batch"] and np.isfinite(lo).all()
    assert ids.tolist() == lo.argmax(axis=1).astype(np.float64).tolist()           # greedy: the dumped logits chose the dumped ids
    _plain(tmp_path / "b")
    for f in ("logits.npy", "next_ids.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
