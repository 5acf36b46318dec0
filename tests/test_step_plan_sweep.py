"""The step planner (fcpt_plan.cpp, with fcpt_schedule.cpp for source_march_applies) alone, under the address and
undefined-behaviour sanitizers: tests/step_plan_sweep.cpp is a program of its own that links nothing else, is run directly,
and holds every plan of its sweep to properties stated without the planner (what a fold, a ride in the CFL launch and a merge
with the gated launch require; the recorded plans of the headline grids).  No GPU, no Python loading of the code under test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
SOURCES = [os.path.join(ROOT, "tests", "step_plan_sweep.cpp"), os.path.join(ROOT, "fargocpt_amd", "csrc", "fcpt_plan.cpp"),
           os.path.join(ROOT, "fargocpt_amd", "csrc", "fcpt_schedule.cpp")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_every_plan_of_the_sweep_keeps_its_properties(tmp_path):
    exe = str(tmp_path / "step_plan_sweep")
    base = [CLANG, "-std=c++17", "-O1", "-g", "-Wall", *SOURCES, "-o", exe]
    sanitized = subprocess.run(base + SANITIZE, capture_output=True, text=True)
    if sanitized.returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    if sanitized.returncode != 0:
        pytest.skip("the sanitizer build failed here, the sweep passed as a plain build: " + sanitized.stderr[-300:])
