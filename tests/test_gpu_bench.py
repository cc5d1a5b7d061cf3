"""The benchmark's plain run (`bench.py --steps K --warmup W` without --full): it times the headline step and writes its
outputs, and leaves every measurement that takes runs of its own to `--full`."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_carries_the_headline_alone(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["metric"] == "ROI-tiles/sec (teacher+student distill step)" and res["unit"] == "tiles/s"
    assert res["higher_is_better"] is True and res["dtype"] == "bf16"
    assert res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["value"] > 0 and res["ms_per_step"] > 0
    assert abs(res["value"] - 64 * 1000.0 / res["ms_per_step"]) <= 1e-3 * res["value"] + 0.02
    assert res["config"]["launch"] == "one captured HIP graph per step", res["config"]["launch"]
    for key in ("north_star_b256", "parity_mode", "value_tolerance_compliant", "variants", "cpu_baseline", "north_star_global_256"):
        assert key not in res, key
    assert set(res["roofline"]) == {"bound", "step_frac", "peak", "unit"}
    dumped = sorted(os.listdir(tmp_path))
    assert "loss.npy" in dumped and "logit_path.npy" in dumped, dumped
