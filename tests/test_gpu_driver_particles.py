"""`fargocpt_hip` on tests/golden/setups/dust_drift_small.yml (the reference's dust_drift setup on 64 x 128 cells with
boundary conditions the driver has, Disk: No, 10 snapshots): the particles.dat of every snapshot equals, to 1e-12, a
Python loop over the ABI started from snapshot 0's particles.dat, and a run restarted from snapshot 5 writes the same
bits as the uninterrupted one."""
import os

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver

import tests.particles_cases as cases
import tests.particles_ref as R
from tests.test_driver_particles_refusals import config, driver as run_driver

pytestmark = pytest.mark.gpu

RECORD = np.dtype([("id", "<u8")] + [(k, "<f8") for k in ("r", "phi", "r_dot", "phi_dot", "r_ddot", "phi_ddot", "mass", "radius",
                                                       "timestep", "facold", "stokes")])
assert RECORD.itemsize == 96


def read_particles(out, n):
    return np.fromfile(os.path.join(out, "snapshots", str(n), "particles.dat"), dtype=RECORD)


@pytest.fixture(scope="module")
def full_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dust")
    r = run_driver("-q", "start", config(tmp, {}))
    assert r.returncode == 0, r.stderr
    return tmp


def test_snapshots_match_a_loop_over_the_abi(product, full_run):
    out = str(full_run / "out")
    p0 = read_particles(out, 0)
    assert p0.size == 12 and np.all(p0["stokes"] > 0.0) and np.allclose(p0["r"], 1.0)
    assert np.allclose(p0["radius"], 1e-6 * cases.CM * 10.0 ** np.arange(12), rtol=1e-12)   # the species ladder, 1e-8 m up
    assert np.allclose(p0["phi_dot"], 1.0, rtol=1e-10) and np.all(p0["r_ddot"] == p0["phi_dot"])  # Kepler speed at 1 au, e = 0
    d = cases.drift_desc(product)
    d.nr_global, d.nphi = 64, 128
    d.bc_vrad[1] = B.BC_OUTFLOW                       # OuterBoundary: outflow
    d.artificial_viscosity = B.ARTVISC_SN             # the driver's default; it enters the CFL step
    d.nsnapshots, d.nmonitor, d.monitor_timestep = 10, 1, 0.628318531
    radii = product.radii(d)
    ctx = driver.make_context(product, d, radii=radii, bodies=([0.0], [0.0], [d.hydro_center_mass]))
    prm = product.particle_params_default(d)
    prm.gravity_cartesian = 1
    prm.escape_radius_min, prm.escape_radius_max = 0.5, 3.0
    ctx.particles_set(prm, p0["id"], *(np.ascontiguousarray(p0[k]) for k in R.FIELDS))
    ctx.calculate_timestep(ctx.cfl())        # main(): CalculateTimeStep; sim::init: once more
    ctx.apply_boundary(0.0, False)
    ctx.calculate_timestep(ctx.cfl())
    time, worst = 0.0, 0.0
    for n in range(1, 11):
        t_next = n * d.monitor_timestep
        while True:        # the driver's loop with Disk: No: CFL dt, policy, snapping; the gas stays as it is
            cfl_dt = ctx.calculate_timestep(ctx.cfl())
            c = ctx.clock
            c.time, c.n_monitor, c.n_snapshot = time, n - 1, n - 1
            ctx.clock = c
            dt = ctx.snap_to_monitor(cfl_dt)
            ctx.particles_step(dt)
            time += dt
            if abs(t_next - time) < 1e-6 * cfl_dt:
                break
        got, want = read_particles(out, n), ctx.particles_get()
        assert np.array_equal(got["id"], want["id"])
        diff = R.worst_difference({k: got[k] for k in ("id",) + R.FIELDS}, want)
        worst = max(worst, max(diff.values()))
        assert max(diff.values()) <= 1e-12, (n, diff)
        for k in ("mass", "r_ddot", "phi_ddot", "timestep", "facold"):     # kept on the host by id
            assert np.array_equal(got[k], p0[k][np.searchsorted(p0["id"], got["id"])]), k
    print("worst difference to the ABI loop: %.3e" % worst)
    ctx.close()


def test_restart_from_snapshot_5_is_bitwise_identical(full_run, tmp_path):
    import shutil
    shutil.copytree(full_run / "out", tmp_path / "out")
    for n in range(6, 11):
        shutil.rmtree(tmp_path / "out" / "snapshots" / str(n))
    r = run_driver("-q", "restart", "5", config(tmp_path, {}))
    assert r.returncode == 0, r.stderr
    for n in range(6, 11):
        a = open(full_run / "out" / "snapshots" / str(n) / "particles.dat", "rb").read()
        b = open(tmp_path / "out" / "snapshots" / str(n) / "particles.dat", "rb").read()
        assert len(a) > 0 and a == b, n
