"""The per-iteration rows of k_transport_fused (TfRow, built by fcpt_tables.cpp:build_tf_rows) against the per-type tables
they were packed from, on the CPU: for slabs of 8, 33 and 2048 rings and every iteration m = -3 .. nr + 1 of the marching
loop each field equals, bit for bit, the field of RadRow / ThetaRow / DampRow at the index the kernel's clamped loads
used before (interface max(m - 1, -1); ring m - 2 and ring m + 1, each replaced by ring 0 outside the grid).  Once through
the library's test hook, and once as tests/transport_rows_sweep.cpp: a program of its own that links the two host
sources and nothing else, run as a plain build and under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from fargocpt_amd import binding as B, setups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
SOURCES = [os.path.join(ROOT, "tests", "transport_rows_sweep.cpp")] + [os.path.join(ROOT, "fargocpt_amd", "csrc", f)
                                                                      for f in ("fcpt_tables.cpp", "fcpt_host.cpp")]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# columns of FCPT_TABLE_TF (include/fargocpt_hip.h)
TF = {n: c for c, n in enumerate(("dr_lo", "dr_hi", "idr_up", "invsurf", "dxtheta", "inv_dxtheta", "invr", "r_omega", "r_next",
                                  "romega_next", "tvr", "tva", "tsg", "ten", "gphi", "dr_invsurf"))}
RAD = {"dr_lo": 0, "dr_hi": 1, "gphi": 2, "idr_up": 3}
THETA = {"invsurf": 0, "dxtheta": 1, "inv_dxtheta": 2, "dr_invsurf": 3, "invr": 4, "r_omega": 5}
DAMP = {"tvr": 4, "tva": 5, "tsg": 6, "ten": 7}


@pytest.mark.parametrize("nr", [8, 33, 2048])
@pytest.mark.parametrize("damping", [0, 1])
def test_every_field_is_the_per_type_table_at_the_kernels_index(product, nr, damping):
    d = setups.planet_disk(product, nr, 64)
    d.damping = damping
    radii = product.radii(d)
    tf, rad, theta, damp = (product.selftest_ring_tables(d, radii, t) for t in (B.TABLE_TF, B.TABLE_RAD, B.TABLE_THETA, B.TABLE_DAMP))
    assert tf.shape == (nr + 5, 16) and rad.shape[0] == nr + 2 and theta.shape[0] == nr and damp.shape[0] == nr + 1
    m = np.arange(-3, nr + 2)
    k, i = m - 1, m - 2
    rk = rad[np.maximum(k, -1) + 1]
    inside = (i >= 0) & (i < nr)
    ti, di = theta[np.where(inside, i, 0)], damp[np.where(inside, i, 0)]
    tn = theta[np.where((m + 1 >= 0) & (m + 1 < nr), m + 1, 0)]
    same = lambda a, b: np.array_equal(a.view(np.uint64), b.view(np.uint64))   # bit for bit
    for name, col in RAD.items():
        assert same(tf[:, TF[name]], np.ascontiguousarray(rk[:, col])), name
    for name, col in THETA.items():
        assert same(tf[:, TF[name]], np.ascontiguousarray(ti[:, col])), name
    for name, col in DAMP.items():
        assert same(tf[:, TF[name]], np.ascontiguousarray(di[:, col])), name
    assert same(tf[:, TF["r_next"]], np.ascontiguousarray(tn[:, 6])) and same(tf[:, TF["romega_next"]], np.ascontiguousarray(tn[:, 5]))
    if damping:
        assert (tf[:, TF["tvr"]:TF["ten"] + 1] != 0).any(), "no row lies in a damping zone"


def _build_and_run(tmp_path, flags):
    exe = str(tmp_path / "transport_rows_sweep")
    subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-Wall", *SOURCES, "-o", exe, *flags], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-4000:]
    assert " 0 failures" in r.stdout


def test_the_stand_alone_sweep_passes(tmp_path):
    _build_and_run(tmp_path, [])


def test_the_stand_alone_sweep_passes_under_the_sanitizers(tmp_path):
    _build_and_run(tmp_path, SANITIZE)
