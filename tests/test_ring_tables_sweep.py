"""The per-ring tables of fcpt_create (fcpt_tables.cpp, with fcpt_host.cpp's split and geometry) alone, under the address and
undefined-behaviour sanitizers: tests/ring_tables_sweep.cpp is a program of its own that links nothing else, is run
directly, and checks every table of its sweep (sizes, finite entries, damping ranges inside the slab).  No GPU, no Python
loading of the code under test."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
SOURCES = [os.path.join(ROOT, "tests", "ring_tables_sweep.cpp")] + [os.path.join(ROOT, "fargocpt_amd", "csrc", f)
                                                                    for f in ("fcpt_tables.cpp", "fcpt_host.cpp")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def test_every_table_of_the_sweep_is_well_formed(tmp_path):
    exe = str(tmp_path / "ring_tables_sweep")
    base = [CLANG, "-std=c++17", "-O1", "-g", "-Wall", *SOURCES, "-o", exe]
    sanitized = subprocess.run(base + SANITIZE, capture_output=True, text=True)
    if sanitized.returncode != 0:
        subprocess.run(base, check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    if sanitized.returncode != 0:
        pytest.skip("the sanitizer build failed here, the sweep passed as a plain build: " + sanitized.stderr[-300:])
