"""test/dust_drift of the reference through the ABI on the device: twelve grains in the frozen 400 x 1403 disk, stepped
by k_particles_step with the fixed dt of test_particles_ref_drift.py.  The reference's criterion (1 % of Nakagawa's
drift speed) holds, and the deviations agree with the numpy restatement's (tests/golden/dust_drift_restatement.json,
which the CPU test pins to the restatement) within 1e-6."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver

import tests.particles_cases as cases
import tests.particles_ref as R
from tests.test_particles_ref_drift import drift_golden, sample_drift

pytestmark = pytest.mark.gpu


def test_device_drift_matches_nakagawa_and_the_restatement(product):
    d, radii, fields, prm, bodies, s = cases.drift_case(product)
    g = R.Grid(radii, d.nr_global, d.nphi)
    gas = cases.isothermal_gas(d, g, fields[0], fields[1], fields[2])
    s["stokes"] = R.initial_stokes(g, gas, R.physics(d, prm), s)    # check_tstop, as the driver sets it
    ctx = driver.make_context(product, d, fields=fields, radii=radii, bodies=bodies)   # frozen gas: no gas step
    # the gas of the CPU test is what fcpt_initial_fields gives; fcpt_init_physics has applied the boundary conditions to
    # the ghost rings, which the two grains that reach the inner edge would feel: put the initial values back
    for f, a in zip((B.F_SIGMA, B.F_VRAD, B.F_VAZI), fields):
        ctx.upload(f, a)
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))

    def advance(nsteps):
        for _ in range(nsteps):
            ctx.particles_step(cases.DRIFT_DT)
        return ctx.particles_get()

    stokes, dev = cases.drift_deviations(*sample_drift(advance, s["id"].copy(), ctx.particles_get()))
    ctx.close()
    gold = drift_golden()
    print("Stokes number, deviation on the device, deviation of the restatement")
    for row in zip(stokes, dev, gold["deviation"]):
        print("%.6e %+.6e %+.6e" % row)
    print("largest difference to the restatement: %.3e" % np.abs(dev - gold["deviation"]).max())
    assert np.all(np.abs(dev) < cases.DRIFT_TOLERANCE), dev
    assert np.abs(dev - np.array(gold["deviation"])).max() < 1e-6
