"""-m gpu: a plain `bench.py` run does only what its headline figure needs -- untimed setup, warm-up, timed steps, the line -- and `--full` adds the
legs measured beside it.  Small launch sets and the 8-bit MSM table keep each run to seconds; the CPU baseline and the commitment / proof legs of
`--full` are left out here (they take tens of seconds), the single-batch latency and the host-input leg stand for the rest."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batches-per-step", "4"]


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "KZG355_BENCH_ECHO")}
    env["KZG355_MSM_BITS"] = "8"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(args), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    return line, dict(line["config"], **line["config"].get("detail", {}))


def test_plain_run_is_the_headline_alone():
    line, cfg = _bench()
    assert cfg["full"] is False
    assert cfg["latency_ms_single_batch"] is None and cfg["latency_ms_single_batch_min"] is None
    assert cfg["host_inputs"] is None and cfg["mid_size_sets"] is None
    assert line["cpu_baseline"] is None
    assert "msm_legs" not in cfg and "coexistence" not in cfg and "value_host_single_call" not in line
    # the roofline comes from the HIP events of the timed steps themselves; the stream-copy rate needs a run of its own
    assert line["roofline"]["avg_launch_ms"] > 0 and line["roofline"]["measured_stream_copy_gbps"] is None
    assert 0 < cfg["setup_s"] <= cfg["wall_s"]


def test_full_run_adds_the_legs_beside_the_headline():
    line, cfg = _bench("--full", "--no-cpu-baseline", "--no-msm-legs")
    assert cfg["full"] is True
    assert cfg["latency_ms_single_batch"] > 0 and cfg["latency_ms_single_batch_min"] > 0
    assert cfg["host_inputs"]["single_call_ms"] > 0 and line["value_host_single_call"] > 0
    assert line["roofline"]["measured_stream_copy_gbps"] > 0
    assert line["cpu_baseline"] is None and "msm_legs" not in cfg                # (turned off by their own flags)
