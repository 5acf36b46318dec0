"""Known answer for the restatement of the explicit adaptive integrator (tests/particles_explicit_ref.py): a Kepler orbit
with e = 0.3, a = 1 around the star alone, polar and Cartesian state, Stokes number 1e30 (the softening vanishes), ten
orbits in 100 calls.  The position is compared with the solution of Kepler's equation, energy and angular momentum with
their initial values.  The bars are ten times what was measured (tests/particles_explicit_cases.py);
independently the position deviation stays below rtol x 1e4 = 1e-8 and the substep count below 1e4."""
import numpy as np
import pytest

import fargocpt_amd

import tests.particles_explicit_cases as xc

_runs = {}


def _run(cartesian):
    if cartesian not in _runs:
        _runs[cartesian] = xc.restatement_kepler(fargocpt_amd.load(), cartesian)
    return _runs[cartesian]


@pytest.mark.parametrize("cartesian", [False, True])
def test_kepler_orbit_of_the_restatement(cartesian):
    pos, en, mom, _, substeps = _run(cartesian)
    print("cartesian=%d: position %.3e, energy %.3e, angular momentum %.3e, %d substeps" % (cartesian, pos, en, mom, substeps))
    assert pos < xc.KEPLER_POSITION_LIMIT
    assert substeps < xc.KEPLER_SUBSTEPS_LIMIT
    assert pos <= xc.KEPLER_BAR_FACTOR * xc.KEPLER_POSITION_MEASURED[cartesian]
    assert en <= xc.KEPLER_BAR_FACTOR * xc.KEPLER_ENERGY_MEASURED[cartesian]
    assert mom <= xc.KEPLER_BAR_FACTOR * xc.KEPLER_MOMENTUM_MEASURED[cartesian]


def test_polar_and_cartesian_runs_agree():
    (xa, ya), (xb, yb) = _run(False)[3], _run(True)[3]
    gap = float(np.hypot(xa - xb, ya - yb))
    print("polar against Cartesian: %.3e" % gap)
    assert gap <= xc.KEPLER_BAR_FACTOR * max(xc.KEPLER_POSITION_MEASURED.values())
