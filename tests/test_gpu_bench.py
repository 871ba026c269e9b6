"""bench.py end to end on the GPU at a few steps: a plain run times the headline and nothing else; --full adds the other
measurements to the same line (side legs and the oracle legs left out here: they take most of a minute)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("t16_ms_per_step", "h3_ms_per_step", "f32_arith_ms_per_step", "consensus_ms", "consensus_frac_of_iteration",
             "ops_path_ms_per_step", "autograd_route_ms_per_step", "decoder_op", "render_ms_per_frame",
             "reference_default_ms_per_iteration", "side_legs_error", "cpu_baseline", "arith_evidence")


def _line(*flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *flags],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_times_the_headline_only():
    line = _line()
    assert line["full"] is False and line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "rays/s" and line["higher_is_better"] is True
    assert line["dtype"] and line["metric"].startswith("training rays/s per GPU")
    assert line["roofline"]["kernels"]   # from the timed steps' own section times
    assert "ceiling_live_Gps" not in line["roofline"].get("fabric_requests", {})
    assert [k for k in FULL_ONLY if k in line] == []


def test_full_run_adds_the_other_measurements():
    line = _line("--full", "--no-side-legs", "--no-cpu-baseline")
    assert line["full"] is True and line["value"] > 0
    assert all(line[k] > 0 for k in ("t16_ms_per_step", "h3_ms_per_step", "f32_arith_ms_per_step", "consensus_ms"))
    if "fabric_requests" in line["roofline"]:
        assert line["roofline"]["fabric_requests"]["ceiling_live_Gps"] > 0
