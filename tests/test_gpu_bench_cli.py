"""bench.py on the MI355X, as a command: a plain run prints the headline line and runs none of the secondary measurements; `--full` runs them.

The small configuration (tinyllama-1.1b shapes, a 12-frame stream, the last 4 frames timed) keeps both runs to seconds; what is checked is which
measurements ran (their keys in the result line), not their values."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--model", "tinyllama-1.1b", "--stream-frames", "12", "--prefetch-frames", "4"]
CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SECONDARY = ("roofline", "encode_stage", "live_feed", "prefill", "cpu_baseline")


def _bench(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, env=env, capture_output=True, text=True, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-500:], r.stderr[-1500:])
    return json.loads(lines[0]), r.stderr


def test_plain_run_measures_the_headline_only():
    d, err = _bench([])
    assert all(k in d for k in CONTRACT) and d["value"] > 0 and d["steps"] == 4 and d["config"]["preroll_frames"] == 8
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]        # one GPU: frames/s is the reciprocal of the step time
    assert not [k for k in SECONDARY if k in d], sorted(d)
    assert "cpu_baseline" not in err and "live_feed" not in err and "prefill probe" not in err


def test_full_run_adds_the_secondary_measurements():
    d, _ = _bench(["--full", "--cpu-budget-s", "2", "--cpu-sample-frames", "2"])
    assert all(k in d for k in CONTRACT) and d["value"] > 0
    assert not [k for k in SECONDARY if k not in d], sorted(d)
    assert d["roofline"]["launches_timed"] > 0 and d["encode_stage"]["ms_per_frame"] > 0 and "error" not in d["prefill"]
    assert all(k in d["live_feed"] for k in ("no_lookahead", "recorded_file_lookahead", "real_greedy_path"))
    assert d["cpu_baseline"].get("value"), d["cpu_baseline"]
