"""The reference's own self-gravity test (test/self_gravity/setup.yml, committed verbatim as
tests/golden/setups/self_gravity.yml) through the host driver: the written a_sg_rad.dat against the reference's
known answer with the reference's threshold, the initial v_phi of a self-gravitating disk, and a restart."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import selfgravity_ref as R
from tests.test_selfgravity_host import ACCEL_CGS, known_answer_deviation

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fargocpt_amd", "bin", "fargocpt_hip")
SETUP = os.path.join(ROOT, "tests", "golden", "setups", "self_gravity.yml")
NR, NPHI = 128, 256


def run_driver(tmp, outname, changes=None, args=("start",)):
    changes = dict(changes or {})
    out = os.path.join(str(tmp), outname)
    lines = []
    for line in open(SETUP).read().splitlines():
        key = line.split(":")[0].strip()
        if line.startswith("OutputDir"):
            line = "OutputDir: " + out
        elif key in changes and not line.startswith("#"):
            line = f"{key}: {changes[key]}"
        lines.append(line)
    cfg = os.path.join(str(tmp), outname + ".yml")
    with open(cfg, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([BIN, "-q", *args, cfg], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return out + "/"


def grid(path, rows=NR):
    return np.fromfile(path).reshape(rows, NPHI)


def n_iter(path):
    raw = open(path, "rb").read()
    assert len(raw) == 48
    return struct.unpack("<IIddddQ", raw)[6]


def test_reference_setup_end_to_end(tmp_path):
    import yaml
    out = run_driver(tmp_path, "sg")
    off = run_driver(tmp_path, "nosg", {"SelfGravity": "no"})
    snap = out + "snapshots/0/"
    info = yaml.safe_load(open(out + "info2D.yml"))
    for name in ("a_sg_rad", "a_sg_azi"):
        assert info[name]["filename"] == name + ".dat" and (info[name]["Nrad"], info[name]["Nazi"]) == (NR, NPHI)
        assert not info[name]["on_radial_interface"]
        assert abs(info[name]["code_to_cgs_factor"] / ACCEL_CGS - 1) < 1e-12
    assert not os.path.exists(off + "snapshots/0/a_sg_rad.dat")
    radii = np.loadtxt(out + "used_rad.dat")
    _, rmed = R.geometry(radii, NR)
    # the reference's criterion (check_results.py, testconfig.yml: 0.0014 for r > 2) on the written file
    g_r = grid(snap + "a_sg_rad.dat")
    dev = known_answer_deviation(rmed, g_r)
    print(f"a_sg_rad.dat against the reference's direct sum, r > 2: {dev:.4e} (threshold 0.0014)")
    assert dev < 0.0014
    assert np.abs(grid(snap + "a_sg_azi.dat")).max() < 1e-10 * np.abs(g_r).max()   # an axisymmetric disk pulls along r only
    # init_azimuthal_velocity (selfgravity.cpp:749-781; OmegaFrame = 0): Rmed sqrt(omega_cell^2 - <g_r> / Rmed) with
    # omega_cell from the speed the disk has without self-gravity, in the active rings 1 .. Nr-2.  Not checked here: the
    # two ghost rings -- the driver's value in row Nr-1 (minus the frame's speed, as the reference leaves it) and the
    # formula's in row 0 are overwritten by the boundary call of fcpt_init_physics before anything is written
    v_sg, v_off = grid(snap + "vazi.dat"), grid(off + "snapshots/0/vazi.dat")
    want = R.init_azimuthal_velocity(g_r, radii, v_off[:, 0] / rmed)
    err = np.abs(v_sg[1:-1] / want[1:-1, None] - 1).max()
    change = np.abs(v_sg[1:-1] / v_off[1:-1] - 1).max()
    print(f"vazi.dat against the numpy restatement {err:.3e}; against the run without self-gravity {change:.3e}")
    assert err <= 1e-12
    assert change > 1e-6


def test_restart_writes_the_same_bits(tmp_path):
    """Two snapshots of about ten steps each; the run restarted from the first writes the bits of the uninterrupted one
    (nothing of the self-gravity is stored: the kernel is rebuilt, the accelerations are recomputed by the first kick).
    The driver writes snapshots at monitor times only, and the CFL condition decides how many steps reach one: the
    "20-step run restarted at step 10" is therefore two monitor intervals of 1.4 time units (about ten steps each at the
    setup's CFL step of about 0.14), with the step counts read from misc.bin and held to a window rather than pinned: what
    is asserted exactly is that the restarted run reaches the second snapshot in the same number of steps with the same
    bits."""
    changes = {"Nsnapshots": "2", "Nmonitor": "1", "MonitorTimestep": "1.4"}
    full = run_driver(tmp_path, "full", changes)
    steps = [n_iter(full + f"snapshots/{k}/misc.bin") for k in (1, 2)]
    print("hydro steps at the two snapshots:", steps)
    assert 4 <= steps[0] <= 40 and steps[0] + 4 <= steps[1] <= 80
    again = os.path.join(str(tmp_path), "again")
    shutil.copytree(full, again)
    shutil.rmtree(os.path.join(again, "snapshots", "2"))
    with open(os.path.join(again, "snapshots", "list.txt"), "w") as f:
        f.write("0\n1\n")
    run_driver(tmp_path, "again", changes, args=("restart", "1"))
    assert n_iter(again + "/snapshots/2/misc.bin") == steps[1]
    for name in ("Sigma.dat", "vrad.dat", "vazi.dat", "a_sg_rad.dat", "a_sg_azi.dat"):
        a, b = np.fromfile(full + "snapshots/2/" + name), np.fromfile(again + "/snapshots/2/" + name)
        assert a.size > 0 and np.array_equal(a, b), name
    first, last = grid(full + "snapshots/0/Sigma.dat"), grid(full + "snapshots/2/Sigma.dat")
    assert not np.array_equal(first, last)
