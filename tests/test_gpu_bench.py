"""bench.py end to end on the metric's workload: a plain run prints the headline line and measures nothing the headline does not
need; ``--full`` adds the repeated regions, the roofline block and the forward / preparation timings (the CPU baseline is left out
here with --no-cpu-baseline: it takes minutes of host time)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = {"ms_per_step_median", "ms_per_step_repeats", "roofline", "gpu_forward_only_ms", "gpu_forward_only_molecules_per_s",
             "per_batch_prep_ms", "cpu_baseline", "gpu_vs_cpu_forward"}


def _result(*extra):
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", *extra],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, run.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_nothing_it_does_not_need():
    r = _result()
    assert r["metric"] == "molecules/s forward+backward, QM9 config_energy batch" and r["unit"] == "molecules/s"
    assert r["higher_is_better"] is True and r["dtype"] == "f32" and r["steps"] == 4 and r["warmup"] == 2
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert abs(r["value"] * r["ms_per_step"] - 256 * 1e3) <= 1e-3 * 256 * 1e3      # the same K steps, rounded
    assert not FULL_ONLY & set(r), sorted(FULL_ONLY & set(r))


@pytest.mark.gpu
def test_full_run_adds_the_measurements_behind_the_headline():
    r = _result("--full", "--no-cpu-baseline")
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert r["ms_per_step_repeats"]["regions"] == 5 and r["ms_per_step_median"] > 0
    assert r["roofline"]["kernel"] == "e3k::tp_fwd_kernel" and r["roofline"]["launches"] > 0 and r["roofline"]["kernels"]
    assert r["gpu_forward_only_ms"] > 0 and r["per_batch_prep_ms"] > 0
    assert "cpu_baseline" not in r
