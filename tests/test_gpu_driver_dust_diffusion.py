"""`fargocpt_hip --dust-seed N` on dust diffusion.
The reference's test/dust_diffusion (tests/golden/setups/dust_diffusion.yml, verbatim; 11 000 host-stepped launches on a
frozen 728 x 1237 grid, a few seconds): snapshot 1 passes the reference's own check (check_results.py, threshold 0.1)
and has the spread sqrt(2 D t); it is also compared with what the numpy restatement recorded for the same seed
(tests/golden/dust_diffusion_restatement.json).
tests/golden/setups/dust_diffusion_small.yml (64 x 128, ten snapshots, drag and diffusion on, 257 particles): every
snapshot equals a Python loop over the ABI from snapshot 0 within 1e-12, and a run restarted from snapshot 5 with the
same seed writes the same bits."""
import os
import shutil

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver

import tests.particles_cases as cases
import tests.particles_diffusion_cases as dcases
import tests.particles_ref as R
from tests.test_driver_particles_refusals import ROOT, driver as run_driver
from tests.test_gpu_driver_particles import read_particles
from tests.test_particles_diffusion_known_answer import golden, reference_rows

pytestmark = pytest.mark.gpu

SMALL_SEED = 7


def config(tmp_path, setup):
    text = open(os.path.join(ROOT, "tests", "golden", "setups", setup)).read().splitlines()
    text = [("OutputDir: " + str(tmp_path / "out")) if l.startswith("OutputDir") else l for l in text]
    cfg = tmp_path / "config.yml"
    cfg.write_text("\n".join(text) + "\n")
    return str(cfg)


def test_the_references_known_answer(tmp_path):
    r = run_driver("-q", "--dust-seed", str(dcases.KA_SEED), "start", config(tmp_path, "dust_diffusion.yml"))
    assert r.returncode == 0, r.stderr
    p = read_particles(str(tmp_path / "out"), 1)
    value, fullest = dcases.known_answer_criterion(p["r"], reference_rows())
    gold = golden()
    log = np.loadtxt(tmp_path / "out" / "monitor" / "timestepLogging.dat")
    print("device: criterion %.4f, mean r %.4f, std %.4f, %d live, fullest bin %d, %d hydro steps | restatement: criterion "
          "%.4f, mean %.4f, std %.4f, %d live | threshold %.1f; difference of the criteria %.4f against 3 / fullest bin = %.4f"
          % (value, p["r"].mean(), p["r"].std(), p.size, fullest, int(log[-1, 2]), gold["criterion"], gold["mean"], gold["std"],
             gold["live"], dcases.KA_THRESHOLD, abs(value - gold["criterion"]), 3.0 / fullest))
    assert int(log[-1, 2]) == dcases.KA_INTERVALS * dcases.KA_SUBSTEPS      # the step count the restatement takes
    assert value < dcases.KA_THRESHOLD
    assert abs(p["r"].std() / dcases.KA_STD - 1.0) <= 0.02
    assert p.size == gold["live"]
    assert abs(value - gold["criterion"]) <= 3.0 / fullest


@pytest.fixture(scope="module")
def small_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dust_diffusion")
    r = run_driver("-q", "--dust-seed", str(SMALL_SEED), "start", config(tmp, "dust_diffusion_small.yml"))
    assert r.returncode == 0, r.stderr
    return tmp


def test_snapshots_match_a_loop_over_the_abi(product, small_run):
    out = str(small_run / "out")
    p0 = read_particles(out, 0)
    assert p0.size == 257 and np.unique(p0["id"]).size == 257 and np.all(p0["stokes"] > 0.0)
    d = cases.drift_desc(product)
    d.nr_global, d.nphi = 64, 128
    d.viscous_alpha = 0.01
    d.bc_vrad[1] = B.BC_OUTFLOW                       # OuterBoundary: outflow
    d.artificial_viscosity = B.ARTVISC_SN             # the driver's default; it enters the CFL step
    d.nsnapshots, d.nmonitor, d.monitor_timestep = 10, 1, 0.628318531
    radii = product.radii(d)
    ctx = driver.make_context(product, d, radii=radii, bodies=([0.0], [0.0], [d.hydro_center_mass]))
    prm = product.particle_params_default(d)
    prm.gravity_cartesian = 1
    prm.escape_radius_min, prm.escape_radius_max = 0.5, 3.0
    ctx.particles_set(prm, p0["id"], *(np.ascontiguousarray(p0[k]) for k in R.FIELDS))
    ctx.particles_diffusion(True, True, SMALL_SEED, 0)
    ctx.calculate_timestep(ctx.cfl())        # main(): CalculateTimeStep; sim::init: once more
    ctx.apply_boundary(0.0, False)
    ctx.calculate_timestep(ctx.cfl())
    time, worst, moved = 0.0, 0.0, 0.0
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
    print("worst difference to the ABI loop: %.3e after %d particle steps" % (worst, ctx.particles_diffusion_get().step))
    # the kicks were there: without them a grain on a circular orbit keeps its radius to the drift of ten intervals
    last = read_particles(out, 10)
    start = p0[np.isin(p0["id"], last["id"])]
    assert np.abs(last["r"] - start["r"]).max() > 1e-3
    ctx.close()


def test_restart_from_snapshot_5_is_bitwise_identical(small_run, tmp_path):
    shutil.copytree(small_run / "out", tmp_path / "out")
    for n in range(6, 11):
        shutil.rmtree(tmp_path / "out" / "snapshots" / str(n))
    r = run_driver("-q", "--dust-seed", str(SMALL_SEED), "restart", "5", config(tmp_path, "dust_diffusion_small.yml"))
    assert r.returncode == 0, r.stderr
    for n in range(6, 11):
        a = open(small_run / "out" / "snapshots" / str(n) / "particles.dat", "rb").read()
        b = open(tmp_path / "out" / "snapshots" / str(n) / "particles.dat", "rb").read()
        assert len(a) > 0 and a == b, n

