"""bench.py on the GPU at a small size: a plain run times the steps and prints the headline line only; `--full` adds
the roofline, cold-evaluation, CPU-baseline and validation legs; `--dump-outputs DIR` writes the last timed step's rows
as float64 .npy files, identical from run to run and equal to what the CPU restatement computes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = ["--gpus", "1", "--segments", "2", "--rows", str(1 << 18), "--steps", "2", "--warmup", "1"]
FULL_ONLY = ("roofline", "cold_eval", "cold_eval_ms", "cpu_baseline", "validated", "lib_sha16")


def _bench(extra, out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SIZE + ["--dump-outputs", str(out_dir)] + extra,
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]   # one JSON result line
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}
    return json.loads(lines[0]), arrays, r.stderr


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    return (_bench([], tmp_path_factory.mktemp("plain")), _bench(["--full"], tmp_path_factory.mktemp("full")))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_only(runs):
    (line, _, err), _ = runs
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "rows/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(2 * (1 << 18) / (line["ms_per_step"] / 1e3))
    assert line["full"] is False
    for k in FULL_ONLY:
        assert k not in line, k
    assert "cpu baseline" not in err and "cold eval" not in err


@pytest.mark.gpu
def test_full_run_keeps_every_leg(runs):
    _, (line, _, _) = runs
    assert line["full"] is True
    for k in FULL_ONLY:
        assert line[k] is not None, k
    assert line["validated"]["ok"] is True, line["validated"]
    assert line["roofline"]["plan_bytes_per_launch"] > 0 and line["roofline"]["stream_copy_gbs"] > 0
    assert line["cpu_baseline"]["value"] > 0


@pytest.mark.gpu
def test_dumped_outputs_are_the_rows_of_the_last_step(runs):
    (line, a, _), (_, b, _) = runs
    assert sorted(a) == ["globs", "tag_hash", "timestamps", "values"]
    n = line["output_rows"]
    assert n > 0
    for name, arr in a.items():
        assert arr.dtype == np.float64 and arr.shape == (n,), name
        assert np.array_equal(arr, b[name]), name   # same arguments, same inputs, same rows (integer-valued sums)
    assert np.all(np.diff(a["timestamps"]) >= 0)   # merged rows ascend by timestamp
    assert np.all(a["timestamps"] % 60000 == 0)   # 1m buckets
    assert np.all(a["values"] == np.round(a["values"])) and a["values"].sum() > 0
