"""The known answers of the explicit adaptive integrator on the device: the Kepler orbit of
tests/test_particles_explicit_kepler.py (polar and Cartesian state) and the drifting grains of
tests/test_particles_explicit_drift.py, with the comparison and the bar of tests/test_gpu_particles_drift.py: the
criterion of the known answer itself, and agreement with the restatement's recorded deviations within 1e-6."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X
from tests.test_particles_explicit_drift import explicit_drift_case, explicit_golden, polar_view
from tests.test_particles_ref_drift import sample_drift

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cartesian", [False, True])
def test_device_kepler_orbit(product, cartesian):
    d, radii, g, fields, phys, prm, bodies, s = xc.kepler_case(product, cartesian)
    ctx = driver.make_context(product, d, radii=radii, bodies=bodies)
    ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, cartesian=cartesian)
    ctx.particles_diffusion(gas_drag=False)
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    ctx.particles_timestep_init()
    most = [0]

    def advance(dt):
        ctx.particles_step(dt)
        ad = ctx.particles_adaptive_get()
        sub = int(ad["accepted"][0] + ad["rejected"][0])
        most[0] = max(most[0], sub)
        return ctx.particles_get(), sub

    pos, en, mom, (x, y), substeps = xc.kepler_run(advance, cartesian)
    ctx.close()
    rpos, ren, rmom, (rx, ry), rsub = xc.restatement_kepler(product, cartesian)
    print("cartesian=%d: position %.3e (restatement %.3e), energy %.3e, angular momentum %.3e, %d substeps (%d), at most %d per call"
          % (cartesian, pos, rpos, en, mom, substeps, rsub, most[0]))
    assert pos < xc.KEPLER_POSITION_LIMIT and substeps < xc.KEPLER_SUBSTEPS_LIMIT and most[0] * 100 <= X.MAX_ATTEMPTS
    assert pos <= xc.KEPLER_BAR_FACTOR * xc.KEPLER_POSITION_MEASURED[cartesian]
    assert en <= xc.KEPLER_BAR_FACTOR * xc.KEPLER_ENERGY_MEASURED[cartesian]
    assert mom <= xc.KEPLER_BAR_FACTOR * xc.KEPLER_MOMENTUM_MEASURED[cartesian]
    assert max(abs(pos - rpos), abs(en - ren), abs(mom - rmom), float(np.hypot(x - rx, y - ry))) < 1e-6


def test_device_explicit_drift_matches_nakagawa_and_the_restatement(product):
    d, radii, fields, prm, bodies, g, gas, phys, s, keep = explicit_drift_case(product)
    gold = explicit_golden()
    sel = np.isin(keep, gold["grains"])         # the grains that keep t_stop >= 10 dt for the 100 orbits
    s = {k: v[sel] for k, v in s.items()}
    ctx = driver.make_context(product, d, fields=fields, radii=radii, bodies=bodies)   # frozen gas: no gas step
    for f, a in zip((B.F_SIGMA, B.F_VRAD, B.F_VAZI), fields):          # as in test_gpu_particles_drift.py
        ctx.upload(f, a)
    ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, cartesian=True)
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    ctx.particles_timestep_init()

    def advance(nsteps):
        for _ in range(nsteps):
            ctx.particles_step(cases.DRIFT_DT)
        return polar_view(ctx.particles_get())

    stokes, dev = cases.drift_deviations(*sample_drift(advance, s["id"].copy(), polar_view(ctx.particles_get())))
    ctx.close()
    print("Stokes number, deviation on the device, deviation of the restatement")
    for row in zip(stokes, dev, gold["deviation"]):
        print("%.6e %+.6e %+.6e" % row)
    print("largest difference to the restatement: %.3e" % np.abs(dev - gold["deviation"]).max())
    assert np.all(np.abs(dev) < cases.DRIFT_TOLERANCE), dev
    assert np.abs(dev - np.array(gold["deviation"])).max() < 1e-6
