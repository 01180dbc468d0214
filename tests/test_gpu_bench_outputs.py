"""-m gpu: the plain bench.py run (only the timed steps and the result line), `--dump-outputs DIR` (the last timed step's outputs,
on inputs fixed by the arguments) and `--full` (the side measurements, as a plain run made them before they moved there)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--gaussians", "30000", "--size", "128", "--views", "16"]


def _bench(args):
    r = subprocess.run([sys.executable, "bench.py"] + SMALL + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_run_dumps_the_last_step_and_repeats_it(gpu, tmp_path):
    runs = []
    for i in range(2):
        d = tmp_path / f"out{i}"
        j = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(d), "--dump-scores", str(tmp_path / f"s{i}.npy")])
        runs.append((j, {n: np.load(d / f"{n}.npy") for n in ("scores", "vis_count", "num_rendered")}))
        assert sorted(os.listdir(d)) == ["num_rendered.npy", "scores.npy", "vis_count.npy"]
    (j, o), (_, o2) = runs
    assert j["metric"] == "candidate-views/sec" and j["unit"] == "candidate-views/s" and j["higher_is_better"] is True
    assert j["dtype"] == "f32" and j["steps"] == 3 and j["warmup"] == 1
    assert j["ms_per_step"] > 0 and abs(j["value"] - 16 / (j["ms_per_step"] * 1e-3)) <= 1e-6 * j["value"]
    assert j["roofline"]["kernel_ms"] > 0 and "seeded weights" in j["config"]["workload"]
    # a plain run measures nothing beside the timed steps
    assert j["cpu_baseline"] is None and j["roofline"]["valu_ceiling"] is None and j["roofline"]["pmc"] is None
    for k in ("parity", "serial_loop", "config4", "columns_11", "api_pose_eval", "gpu_occupancy_frontier", "cpu_occupancy_frontier"):
        assert k not in j
    assert "measured_copy_GBps" not in j["roofline"]
    assert o["scores"].dtype == np.float32 and o["vis_count"].dtype == np.float64 and o["num_rendered"].dtype == np.float64
    assert all(v.shape == (16,) for v in o.values())
    assert np.isfinite(o["scores"]).all() and (o["scores"] > 0).all() and (o["vis_count"] > 0).all()
    assert (o["num_rendered"] >= o["vis_count"]).all()
    assert np.array_equal(o["scores"], np.load(tmp_path / "s0.npy"))          # the scores the step copied to the host
    assert abs(float(o["vis_count"].mean()) - j["config"]["visible_per_view"]) < 1e-6 * j["config"]["visible_per_view"]
    for n in o:                                                                 # same arguments, same inputs, same outputs
        assert np.array_equal(o[n], o2[n]), n


def test_full_run_keeps_the_side_measurements(gpu):
    j = _bench(["--steps", "2", "--warmup", "1", "--full", "--cpu-views", "2"])
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and "H_inv from 16 keyframes" in j["config"]["workload"]
    assert j["cpu_baseline"]["value"] > 0 and j["cpu_occupancy_frontier"]["ms_per_update"] > 0
    assert j["parity"]["ok"] and j["parity"]["views"] >= 2
    assert j["serial_loop"]["value"] > 0 and j["vs_serial_loop"] > 0 and j["compute_hessian_v1_ms"] > 0
    assert j["api_pose_eval"]["ms_per_call"] > 0 and j["config4"]["ms_per_step"] > 0 and j["columns_11"]["value"] > 0
    assert j["gpu_occupancy_frontier"]["ms_per_update"] > 0 and j["roofline"]["measured_copy_GBps"] > 0
    assert j["roofline"]["valu_ceiling"] is not None and j["roofline"]["pmc"] is not None
