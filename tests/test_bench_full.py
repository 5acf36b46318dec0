"""`bench.py` plain and with `--full`: a plain run carries the headline and nothing that takes a run of its own;
`--full` adds the CPU baseline with its parity check, the settle blocks and (here skipped: it runs the BASELINE
configurations at their full sizes) the table of configurations, around the same timed region."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
ARGS = ["--gpus", "1", "--steps", "12", "--warmup", "3", "--nr", "64", "--nphi", "512"]
FULL_ONLY = ("cpu_baseline", "configs", "strong_scaling")


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["FCPT_BENCH_SETTLE_STEPS"], env["FCPT_BENCH_SETTLE_MS"] = "20", "1"
    return env


def _line(extra):
    r = subprocess.run([sys.executable, BENCH] + ARGS + extra, env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_full_is_an_option_and_off_by_default():
    sys.path.insert(0, ROOT)
    import bench
    argv = sys.argv
    try:
        sys.argv = ["bench.py"] + ARGS
        assert bench.parse_args().full is False
        sys.argv = ["bench.py"] + ARGS + ["--full"]
        assert bench.parse_args().full is True
    finally:
        sys.argv = argv


def test_full_reaches_the_ranks_of_a_plain_n_gpu_invocation():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--dry-run-ranks", "--full"], env=dict(_env(), OMP_NUM_THREADS="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout)["n_gpus"] == 2


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone():
    rec = _line([])
    assert rec["full"] is False and rec["steps"] == 12 and rec["warmup"] == 3
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in rec, k
    assert rec["value"] == pytest.approx(64 * 512 / (rec["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in rec] and rec["ms_per_step_blocks"] == []
    assert "second context" not in rec["untimed_other"]   # no parity leg queued ahead of the settle steps
    # the options that choose among --full's legs change nothing without it
    rec = _line(["--settle-blocks", "2", "--no-configs"])
    assert not [k for k in FULL_ONLY if k in rec] and rec["ms_per_step_blocks"] == []


@pytest.mark.gpu
def test_full_adds_the_cpu_baseline_and_the_blocks():
    rec = _line(["--full", "--no-configs", "--settle-blocks", "2"])
    assert rec["full"] is True and rec["steps"] == 12
    assert rec["value"] == pytest.approx(64 * 512 / (rec["ms_per_step"] * 1e-3), rel=1e-9)
    assert len(rec["ms_per_step_blocks"]) == 2 and min(rec["ms_per_step_blocks"]) > 0
    assert rec["cpu_baseline"]["parity_ok"] is True and rec["cpu_baseline"]["value"] > 0
    assert "configs" not in rec and "second context" in rec["untimed_other"]
