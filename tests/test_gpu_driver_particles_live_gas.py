"""`fargocpt_hip` on tests/golden/setups/dust_drift_live_small.yml -- dust_drift_small.yml with Disk: yes: the star alone,
64 x 128 cells, ten snapshots.  Nothing moves but the gas and the particles, so the driver switches
fcpt_particles_follow_run_steps on and takes its fcpt_run_steps stretches between the monitor times, particles included.

Every snapshot's particles and gas equal a Python host-stepped loop over the ABI (cfl, calculate_timestep, snap_to_monitor,
particles_step, step, post) started from the files of snapshot 0.  Bars: the particles 1e-12, the bar of
tests/test_gpu_driver_particles.py; the gas bit for bit, as tests/test_gpu_parity.py::test_device_resident_dt_loop holds the
two loops.  Measured: the gas equal in every bit, the particles to 5.6e-13 (the frozen-gas run of that test stands at
9.2e-14 against its loop); 30 of the 60 hydro steps inside fcpt_run_steps.  The closing line of the driver reports the steps taken inside fcpt_run_steps, and a run restarted from snapshot
5 writes the same bytes."""
import os
import re
import shutil

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver

import tests.particles_cases as cases
import tests.particles_ref as R
from tests.test_driver_particles_refusals import driver as run_driver
from tests.test_gpu_driver_particles import read_particles
from tests.test_particles_run_steps_host import LIVE_SETUP, live_config

pytestmark = pytest.mark.gpu

GRIDS = (("Sigma.dat", B.F_SIGMA), ("vrad.dat", B.F_VRAD), ("vazi.dat", B.F_VAZI))


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dust_live")
    r = run_driver("start", live_config(tmp))
    assert r.returncode == 0, r.stderr
    return tmp, r.stdout


def read_grid(out, n, name, shape):
    return np.fromfile(os.path.join(out, "snapshots", str(n), name)).reshape(shape)


def test_the_closing_line_counts_the_steps_inside_run_steps(full_run):
    _, stdout = full_run
    m = re.search(r"-- Particles: (\d+) of this run's (\d+) hydro steps ran inside fcpt_run_steps", stdout)
    assert m, stdout
    inside, total = int(m.group(1)), int(m.group(2))
    print("%d of %d hydro steps inside fcpt_run_steps" % (inside, total))
    assert 0 < inside <= total


def test_snapshots_match_a_host_stepped_loop_over_the_abi(product, full_run):
    out = str(full_run[0] / "out")
    p0 = read_particles(out, 0)
    assert p0.size == 12 and np.all(p0["stokes"] > 0.0)
    d = cases.drift_desc(product)
    d.nr_global, d.nphi = 64, 128
    d.bc_vrad[1] = B.BC_OUTFLOW                       # OuterBoundary: outflow
    d.artificial_viscosity = B.ARTVISC_SN             # the driver's default
    d.nsnapshots, d.nmonitor, d.monitor_timestep = 10, 1, 0.628318531
    radii = product.radii(d)
    shapes = {B.F_SIGMA: (64, 128), B.F_VRAD: (65, 128), B.F_VAZI: (64, 128)}
    fields = [read_grid(out, 0, name, shapes[f]) for name, f in GRIDS] + [np.zeros((64, 128))]
    ctx = driver.make_context(product, d, fields=fields, radii=radii, bodies=([0.0], [0.0], [d.hydro_center_mass]))
    prm = product.particle_params_default(d)
    prm.gravity_cartesian = 1
    prm.escape_radius_min, prm.escape_radius_max = 0.5, 3.0
    ctx.particles_set(prm, p0["id"], *(np.ascontiguousarray(p0[k]) for k in R.FIELDS))
    ctx.calculate_timestep(ctx.cfl())        # main(): CalculateTimeStep; sim::init: once more
    ctx.apply_boundary(0.0, False)
    ctx.calculate_timestep(ctx.cfl())
    worst, steps = 0.0, 0
    for n in range(1, 11):
        t_next = n * d.monitor_timestep
        while True:
            cfl_dt = ctx.calculate_timestep(ctx.cfl())
            dt = ctx.snap_to_monitor(cfl_dt)
            ctx.particles_step(dt)                   # OmegaFrame = 0, the star alone: no frame angle, no indirect term
            ctx.step(dt)
            ctx.post(dt)
            steps += 1
            c = ctx.clock
            if abs(t_next - c.time) < 1e-6 * cfl_dt:
                c.n_monitor, c.n_snapshot = n, n
                ctx.clock = c
                break
        got, want = read_particles(out, n), ctx.particles_get()
        assert np.array_equal(got["id"], want["id"])
        diff = R.worst_difference({k: got[k] for k in ("id",) + R.FIELDS}, want)
        worst = max(worst, max(diff.values()))
        assert max(diff.values()) <= 1e-12, (n, diff)
        for name, f in GRIDS:
            assert np.array_equal(read_grid(out, n, name, shapes[f]), ctx.download(f)), (n, name)
    print("worst particle difference to the host-stepped loop: %.3e over %d steps" % (worst, steps))
    ctx.close()


def test_restart_from_snapshot_5_is_bitwise_identical(full_run, tmp_path):
    shutil.copytree(full_run[0] / "out", tmp_path / "out")
    for n in range(6, 11):
        shutil.rmtree(tmp_path / "out" / "snapshots" / str(n))
    r = run_driver("-q", "restart", "5", live_config(tmp_path))
    assert r.returncode == 0, r.stderr
    for n in range(6, 11):
        for name in ("particles.dat",) + tuple(g for g, _ in GRIDS):
            a = open(full_run[0] / "out" / "snapshots" / str(n) / name, "rb").read()
            b = open(tmp_path / "out" / "snapshots" / str(n) / name, "rb").read()
            assert len(a) > 0 and a == b, (n, name)
