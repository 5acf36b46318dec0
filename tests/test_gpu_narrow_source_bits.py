"""The source step of rings the marching kernels do not take (k_src_fused, k_av_fused, k_visc_fused; k_visc_factors) computes
the bits it computed before k_src_fused and k_visc_fused became templates over the body-force and StabilizeViscosity options
(k_visc_factors is the parent's text: restated as a caller of visc_factors_row it missed every factor hash here): SHA-256 of Sigma, v_r, v_phi, e, Q+, Q-, MASSFLOW (those the case has) and
of the dt history, after 5 steps of the host loop and after 6 steps of fcpt_run_steps, from rough states, and the two
correction-factor grids where k_visc_factors fills them in both builds from the same nu and Sigma: as fcpt_init_physics
leaves them in an ideal-EOS context (alpha viscosity: nu from the grid; an isothermal context does not run the kernel
there), and after ONE step of a narrow isothermal context with a constant nu (the parent queued the same kernel in its
per-loop kick; from the second step on the two builds' Sigma differ in the last bits).  Both sides assert that the grids
are not zero.  Recorded from a build of the parent commit
(tests/golden/make_narrow_source_parent_bits.py).  The three-slab case has its slabs in one process, so it takes the host
loop only (fcpt_run_steps on several slabs needs a communicator)."""
import hashlib
import json
import os

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups
from tests import rough_states as R
from tests.parity_runs import run_state

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "narrow_source_parent_bits.json")
HOST_STEPS, DEVICE_STEPS = 5, 6


def _rough(nr, nphi, physics, kind, slabs=1, **kw):
    def state(lib):
        return R.make_state(lib, R.case_desc(lib, nr, nphi, physics, kind, **kw), kind, nslabs=slabs) + (slabs,)
    return state


def _shocktube(lib):
    d = setups.shocktube(lib, 256, 4, "SN")   # Nphi <= 16: the artificial viscosity's length is the smaller cell side
    d.rank, d.nranks = 0, 1
    radii = lib.radii(d)
    fields = [np.ascontiguousarray(f) for f in lib.initial_fields(d, radii)]
    return d, radii, fields, 1


CASES = {
    "noisy_iso_32x96": _rough(32, 96, "iso", "noisy"),
    "shocked_visc_32x96_sn": _rough(32, 96, "visc", "shocked", av="SN"),   # ideal EOS, dissipation, viscous heating
    "floored_cool_lin_32x96": _rough(32, 96, "cool_lin", "floored"),
    "shocked_visc_32x96_lf": _rough(32, 96, "visc", "shocked", leapfrog=True),
    "noisy_iso_32x48": _rough(32, 48, "iso", "noisy"),
    "shocked_iso_48x96_3slabs": _rough(48, 96, "iso", "shocked", slabs=3),
    "shocktube_256x4_sn": _shocktube,
    "noisy_iso_40x3_lf_massflow": _rough(40, 3, "iso", "noisy", leapfrog=True, massflow=True),
}
FACTOR_GRIDS = (("init_ideal", 32, 96), ("init_ideal", 32, 130), ("step_iso", 32, 96), ("step_iso", 32, 48))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_hashes(lib, name):
    d0, radii, fields, slabs = CASES[name](lib)
    out = {}
    for loop, steps in (("host", HOST_STEPS), ("device", DEVICE_STEPS)):
        if loop == "device" and slabs > 1:
            continue
        grids, dts, _, _ = run_state(lib, d0, radii, fields, slabs, steps, loop)
        assert all(np.isfinite(g).all() for g in grids.values()), name
        out[loop] = {k: _sha(g) for k, g in sorted(grids.items())}
        out[loop]["dt"] = _sha(np.asarray(dts, dtype=np.float64))   # (device loop: the clock's time)
    return out


def factor_hashes(lib, kind, nr, nphi):
    d = setups.planet_disk(lib, nr, nphi, adiabatic=kind == "init_ideal")
    d.stabilize_viscosity = 1
    if kind == "step_iso":
        d.viscous_alpha, d.constant_viscosity = 0.0, 1.0e-2
    _, radii, fields = R.noisy(lib, d)
    ctx = driver.make_context(lib, d, fields=tuple(np.ascontiguousarray(f) for f in fields), radii=radii)   # + init_physics
    try:
        if kind == "step_iso":
            s = driver.SlabSet([ctx])
            s.prepare()
            s.run(1)
        out = {}
        for name, f in (("cfac_phi", B.F_VISC_CFAC_PHI), ("cfac_r", B.F_VISC_CFAC_R)):
            g = ctx.download(f)
            assert np.isfinite(g).all() and (g[1:] < 0).all(), "%s %dx%d: %s was not filled by k_visc_factors" % (kind, nr, nphi, name)
            out[name] = _sha(g)
        assert out["cfac_phi"] != out["cfac_r"]
        return out
    finally:
        ctx.close()


def factor_key(kind, nr, nphi):
    return "%s_%dx%d" % (kind, nr, nphi)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_record_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    assert sorted(golden["factors"]) == sorted(factor_key(*g) for g in FACTOR_GRIDS)


@pytest.mark.parametrize("name", sorted(CASES))
def test_narrow_source_step_gives_the_parent_bits(product, golden, name):
    assert case_hashes(product, name) == golden["cases"][name]


@pytest.mark.parametrize("grid", FACTOR_GRIDS, ids=[factor_key(*g) for g in FACTOR_GRIDS])
def test_correction_factors_give_the_parent_bits(product, golden, grid):
    assert factor_hashes(product, *grid) == golden["factors"][factor_key(*grid)]
