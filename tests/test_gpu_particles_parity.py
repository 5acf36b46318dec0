"""k_particles_step against the numpy restatement (tests/particles_ref.py), step by step on the same gas: after 8 gas
steps of planet_disk with Jupiter, 20 times {download Sigma, H, T, v_r, v_phi; fcpt_particles_step; gas step}, the
restatement stepping the same downloads with the same dt.  The particles are the draw that
test_particles_ref_census.py holds to its purpose.  Bar: the project's parity bar, max|a-b| / max|b| <= 1e-10 per
quantity over the live particles for r, r_dot, r phi_dot and stokes, the angle difference mod 2 pi <= 1e-10 for phi,
the same live ids -- checked after every one of the 20 steps, so that particles which leave during the run are compared
while they live."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups

import tests.particles_cases as cases
import tests.particles_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-10
GRIDS = (B.F_SIGMA, B.F_SCALE_HEIGHT, B.F_TEMPERATURE, B.F_VRAD, B.F_VAZI)


def _run(product, d, n, cartesian, compare=True):
    """-> (final live particles of the device, worst ratio to the bar, restatement diagnostics of compared particles)"""
    radii = product.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    bodies = setups.jupiter_bodies(d)
    ctx = driver.make_context(product, d, radii=radii, bodies=bodies)
    S = driver.SlabSet([ctx])
    S.prepare()
    S.run(8)
    prm = cases.parity_params(product, d, cartesian)
    phys = R.physics(d, prm)
    gas = R.gas_fields(*(ctx.download(f) for f in GRIDS), d.density_factor)
    s = cases.census_draw(d, radii, n=n)
    s["stokes"] = R.initial_stokes(g, gas, phys, s)
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    assert ctx.particles_count() == n
    dt, worst, r_in = cases.PARITY_DT, 0.0, []
    for _ in range(cases.PARITY_STEPS):
        if compare:
            gas = R.gas_fields(*(ctx.download(f) for f in GRIDS), d.density_factor)
        ctx.particles_step(dt, cases.PARITY_INDIRECT, d.omega_frame * dt)
        ctx.step(dt)
        ctx.post(dt)
        if compare:
            slots = np.flatnonzero(s["alive"])
            guards, diag = R.step(g, gas, phys, bodies, s, dt, cases.PARITY_INDIRECT, d.omega_frame * dt)
            assert not guards.any()
            r_in.append(diag["r_in"][s["alive"][slots]])
            got, want = ctx.particles_get(), R.live(s)
            assert np.array_equal(got["id"], want["id"]), "the sets of live particles differ"
            assert np.array_equal(got["radius"], want["radius"])
            diff = R.worst_difference(got, want)
            worst = max(worst, max(diff.values()) / BAR)
            assert max(diff.values()) <= BAR, diff
    out = ctx.particles_get()
    assert ctx.particles_count() == out["id"].size
    ctx.close()
    return out, worst, (g, np.concatenate(r_in) if r_in else None)


@pytest.mark.parametrize("adiabatic,cartesian,smoothing,omega_frame,n", [
    (False, False, 0.6, 1.0, 1000),     # 1000 is no multiple of 64 or 256
    (True, True, 0.6, 1.0, 1000),
    (False, True, 0.0, 0.0, 257),
    (True, False, 0.0, 0.0, 1),
])
def test_particle_step_matches_the_restatement(product, adiabatic, cartesian, smoothing, omega_frame, n):
    d = cases.parity_desc(product, 48, 256, adiabatic=adiabatic, smoothing=smoothing, omega_frame=omega_frame)
    out, worst, (g, r_in) = _run(product, d, n, cartesian)
    print("worst ratio to the bar: %.3e, %d of %d particles live" % (worst, out["id"].size, n))
    if n == 1000:   # the census' purpose, on the device's own gas: compared particles met both extrapolation zones
        assert (r_in < g.rmed[0]).any() and (r_in > g.rmed[-1]).any()
        assert out["id"].size < n, "nobody left the domain"


@pytest.mark.parametrize("spacing,adiabatic", [(B.SPACING_LOGARITHMIC, True), (B.SPACING_ARITHMETIC, False),
                                               (B.SPACING_EXPONENTIAL, False)])
def test_cell_search_on_the_three_radial_spacings(product, spacing, adiabatic):
    d = cases.parity_desc(product, 32, 64, adiabatic=adiabatic, spacing=spacing)
    # (with 32 rings on [0.4, 2.5] the Newton iteration of the exponential spacing, init.cpp:113-131, has no root for the
    #  default first-cell factor 1.41; 2.0 gives cells growing from 0.050 to 0.094)
    d.exponential_cell_size_factor = 2.0
    assert np.all(np.isfinite(product.radii(d)))
    out, worst, _ = _run(product, d, 257, cartesian=False)
    print("worst ratio to the bar: %.3e, %d of 257 particles live" % (worst, out["id"].size))


def test_two_identical_runs_give_identical_bits(product):
    d = cases.parity_desc(product, 48, 256)
    a, _, _ = _run(product, d, 1000, cartesian=False, compare=False)
    b, _, _ = _run(product, d, 1000, cartesian=False, compare=False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_guard_leaves_the_particle_alone_and_is_reported(product):
    """Gas at rest in a frame at rest and a particle at rest: v_rel = 0 exactly, so Ma = 0 trips the first guard of
    calc_tstop (the reference dies there).  The particle stays as it was, the next blocking call names it once, the
    other particles are stepped, and the context goes on and can be destroyed."""
    d = cases.parity_desc(product, 48, 256, omega_frame=0.0)
    radii = product.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    bodies = setups.jupiter_bodies(d)
    ctx = driver.make_context(product, d, radii=radii, bodies=bodies)
    ctx.upload(B.F_VRAD, np.zeros(ctx.shape(B.F_VRAD)))
    ctx.upload(B.F_VAZI, np.zeros(ctx.shape(B.F_VAZI)))
    prm = cases.parity_params(product, d, cartesian=False)
    phys = R.physics(d, prm)
    gas = R.gas_fields(*(ctx.download(f) for f in GRIDS), d.density_factor)
    s = cases.census_draw(d, radii, n=65)
    s["stokes"] = R.initial_stokes(g, gas, phys, s)
    at_rest = 40
    s["r_dot"][at_rest] = s["phi_dot"][at_rest] = 0.0
    before = {k: v.copy() for k, v in R.live(s).items()}
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    ctx.particles_step(cases.PARITY_DT)
    with pytest.raises(B.FcptError, match=r"particle id %d .*guard 1" % int(s["id"][at_rest])):
        ctx.particles_count()
    assert ctx.particles_count() == 65          # reported once; the particle lives on
    guards, _ = R.step(g, gas, phys, bodies, s, cases.PARITY_DT)
    assert guards[at_rest] == 1 and np.count_nonzero(guards) == 1
    got, want = ctx.particles_get(), R.live(s)
    for k in ("r", "phi", "r_dot", "phi_dot", "stokes"):
        assert got[k][at_rest] == before[k][at_rest], k        # untouched, bit for bit
    assert max(R.worst_difference(got, want).values()) <= BAR
    ctx.particles_step(cases.PARITY_DT)          # the context steps on ...
    with pytest.raises(B.FcptError, match="guard 1"):
        ctx.particles_get()
    assert ctx.particles_get()["id"].size == 65
    ctx.close()                                  # ... and is destroyable


def test_set_refuses_what_the_step_cannot_serve(product):
    d = cases.parity_desc(product, 48, 256)
    ctx = driver.make_context(product, d)
    prm = cases.parity_params(product, d, cartesian=False)
    one = np.ones(1)
    prm.escape_radius_min = 0.5 * d.rmin
    with pytest.raises(B.FcptError, match="escape radii"):
        ctx.particles_set(prm, np.zeros(1, dtype=np.uint64), one, one, one, one, one, one)
    prm.escape_radius_min = d.rmin
    ctx.particles_set(prm, np.zeros(1, dtype=np.uint64), one, one, one, one, one, one)
    assert ctx.particles_count() == 1
    ctx.particles_set(prm, np.zeros(0, dtype=np.uint64), *(np.zeros(0),) * 6)    # n = 0 removes them
    assert ctx.particles_count() == 0
    ctx.particles_step(1e-3)     # nothing to launch
    ctx.close()
    d.nranks, d.rank = 2, 0
    ctx = driver.make_context(product, d)
    with pytest.raises(B.FcptError, match="slab"):
        ctx.particles_set(prm, np.zeros(1, dtype=np.uint64), one, one, one, one, one, one)
    ctx.close()
