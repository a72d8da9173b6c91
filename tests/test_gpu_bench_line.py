"""GPU: the plain bench.py line (no --full) and --dump-outputs.  A plain run times exactly --steps steps in one region and prints
the headline fields only; --dump-outputs writes the last timed step's probabilities, which must be the float64 oracle's on the
seeded inputs of that step (the same inputs on every run)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.util import assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _last_json_line(text):
    for line in reversed(text.strip().splitlines()):
        line = line.strip()
        if line.startswith("{") and line.endswith("}"):
            return json.loads(line)
    raise AssertionError("no JSON line in:\n" + text[-2000:])


def test_plain_bench_line_and_dumped_outputs(device, tmp_path):
    import torch
    import bench
    from oracle import ref_models
    K = 6
    out = tmp_path / "dump"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(K), "--warmup", "2", "--dump-outputs", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = _last_json_line(r.stdout)
    assert line["metric"] == bench.WORKLOADS["c2"]["metric"] and line["unit"] == "samples/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == K and line["warmup"] == 2 and line["full"] is False
    assert len(line["regions_ms"]) == 1 and line["value"] > 0
    assert abs(line["ms_per_step"] * K - line["regions_ms"][0]) <= 1e-9 * line["regions_ms"][0]
    assert not any(k in line for k in ("parity", "roofline", "kernels", "long_run", "cpu_baseline", "cold_one_shot"))
    y = np.load(str(out / "predictions.npy"))
    assert y.shape == (bench.B, 1) and y.dtype == np.float32
    # the last step's ids: batch K - 1 of the seeded ring (K <= 256: one launch of K batches from the start of a ring of whole launches)
    bench.set_workload("c2")
    model, cols = bench.build_model(torch.device("cpu"))
    ring = (64 + K - 1) // K * K
    feed = bench.synthetic_feed(ring * bench.B, 1000)
    rows = slice((K - 1) * bench.B, K * bench.B)
    ref = ref_models.deepfm(cols, cols, model.get_weights_by_name(), {k: v[rows] for k, v in feed.items()},
                            dnn_hidden_units=bench.HIDDEN, dtype=np.float64)
    assert_close(y, ref, rtol=1e-4, atol=1e-6, what="bench --dump-outputs vs float64 oracle")
