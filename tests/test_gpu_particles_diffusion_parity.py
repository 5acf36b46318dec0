"""k_particles_step with the drag off and with the diffusion kick, against the numpy restatement
(tests/particles_diffusion_ref.py), step by step beside the gas: the loop of test_gpu_particles_parity._run -- after 8
gas steps of planet_disk with Jupiter and a ring of gas at r = 1.4 (so that the kick's drift term takes both signs), 20
times {download the gas; fcpt_particles_step; gas step}, the restatement stepping the same downloads with the same dt,
seed and counter.  Bar: as there, max|a-b| / max|b| <= 1e-10 per quantity over the live particles, the angle difference
mod 2 pi <= 1e-10, the same live ids, after every step.  The draw is the one test_particles_diffusion_census.py holds
to its purpose; the counter starts below 2^32 and ends above it."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups

import tests.particles_cases as cases
import tests.particles_diffusion_cases as dcases
import tests.particles_diffusion_ref as D
import tests.particles_ref as R

pytestmark = pytest.mark.gpu

BAR = 1e-10
GRIDS = (B.F_SIGMA, B.F_SCALE_HEIGHT, B.F_TEMPERATURE, B.F_VRAD, B.F_VAZI)


def _gas(ctx, d):
    gas = R.gas_fields(*(ctx.download(f) for f in GRIDS), d.density_factor)
    gas["cs"] = ctx.download(B.F_SOUNDSPEED)
    return gas


def _run(product, d, n, cartesian, drag, diffusion, compare=True, seed=dcases.PARITY_SEED, split_at=None, ids=None):
    """-> (final live particles of the device, worst ratio to the bar)"""
    radii = product.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    bodies = setups.jupiter_bodies(d)
    dd = d.copy()
    sigma, vrad, vazi, energy = product.initial_fields(dd, radii)
    bump = dcases.ring_bump(g)[:, None]
    ctx = driver.make_context(product, dd, fields=(sigma * bump, vrad, vazi, energy * bump), radii=radii, bodies=bodies)
    S = driver.SlabSet([ctx])
    S.prepare()
    S.run(8)
    prm = cases.parity_params(product, d, cartesian)
    phys = R.physics(d, prm)
    s = dcases.diffusion_draw(d, radii, n=n)
    if ids is not None:
        s["id"] = np.asarray(ids, dtype=np.uint64)
    s["stokes"] = R.initial_stokes(g, _gas(ctx, d), phys, s)
    first = dcases.PARITY_FIRST_STEP
    ctx.particles_diffusion(drag, diffusion, seed, first)
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    assert ctx.particles_count() == n
    dt, worst = cases.PARITY_DT, 0.0
    for k in range(cases.PARITY_STEPS):
        if k == split_at:       # what a restart does: the live particles into a new set, the counter handed over
            p = ctx.particles_get()
            assert ctx.particles_diffusion_get().step == first + k
            ctx.particles_set(prm, p["id"], *(p[q] for q in R.FIELDS))
            ctx.particles_diffusion(drag, diffusion, seed, first + k)
        if compare:
            gas = _gas(ctx, d)
        ctx.particles_step(dt, cases.PARITY_INDIRECT, d.omega_frame * dt)
        ctx.step(dt)
        ctx.post(dt)
        if compare:
            guards, _ = D.step(g, gas, phys, bodies, s, dt, cases.PARITY_INDIRECT, d.omega_frame * dt, gas_drag=drag,
                               diffusion=diffusion, seed=seed, step_no=first + k)
            assert not guards.any()
            got, want = ctx.particles_get(), R.live(s)
            assert np.array_equal(got["id"], want["id"]), "the sets of live particles differ"
            assert np.array_equal(got["radius"], want["radius"])
            diff = R.worst_difference(got, want)
            worst = max(worst, max(diff.values()) / BAR)
            assert max(diff.values()) <= BAR, (k, diff)
    assert ctx.particles_diffusion_get().step == first + cases.PARITY_STEPS
    out = ctx.particles_get()
    ctx.close()
    return out, worst


@pytest.mark.parametrize("drag,diffusion", dcases.SWITCHES)
@pytest.mark.parametrize("adiabatic,cartesian,smoothing,omega_frame,n", [
    (False, False, 0.6, 1.0, 1000),
    (True, True, 0.6, 1.0, 1000),
    (False, True, 0.0, 0.0, 257),
    (True, False, 0.0, 0.0, 1),
])
def test_step_matches_the_restatement(product, adiabatic, cartesian, smoothing, omega_frame, n, drag, diffusion):
    d = cases.parity_desc(product, 48, 256, adiabatic=adiabatic, smoothing=smoothing, omega_frame=omega_frame)
    d.viscous_alpha = dcases.PARITY_ALPHA
    out, worst = _run(product, d, n, cartesian, drag, diffusion)
    print("worst ratio to the bar: %.3e, %d of %d particles live" % (worst, out["id"].size, n))
    if n == 1000:
        assert out["id"].size < n, "nobody left the domain"


@pytest.mark.parametrize("drag,diffusion", dcases.SWITCHES)
@pytest.mark.parametrize("spacing,adiabatic", [(B.SPACING_LOGARITHMIC, True), (B.SPACING_ARITHMETIC, False),
                                               (B.SPACING_EXPONENTIAL, False)])
def test_kick_cell_on_the_three_radial_spacings(product, spacing, adiabatic, drag, diffusion):
    d = cases.parity_desc(product, 32, 64, adiabatic=adiabatic, spacing=spacing)
    d.viscous_alpha = dcases.PARITY_ALPHA
    d.exponential_cell_size_factor = 2.0      # (as in test_gpu_particles_parity: the default has no root on this grid)
    out, worst = _run(product, d, 257, False, drag, diffusion)
    print("worst ratio to the bar: %.3e, %d of 257 particles live" % (worst, out["id"].size))


@pytest.mark.parametrize("drag", [True, False])
def test_without_alpha_there_is_no_kick_but_the_counter_runs(product, drag):
    d = cases.parity_desc(product, 48, 256)
    d.viscous_alpha = 0.0
    out, worst = _run(product, d, 257, False, drag, True)
    print("worst ratio to the bar: %.3e" % worst)
    if drag:    # D_g = 0: bit for bit the step without diffusion (pow(1, 1.5) = 1)
        ref, _ = _run(product, d, 257, False, True, False, compare=False)
        for k in ref:
            assert np.array_equal(out[k], ref[k]), k


def test_identical_runs_split_runs_and_seeds(product):
    d = cases.parity_desc(product, 48, 256)
    d.viscous_alpha = dcases.PARITY_ALPHA
    a, _ = _run(product, d, 1000, False, True, True, compare=False)
    b, _ = _run(product, d, 1000, False, True, True, compare=False)
    c, _ = _run(product, d, 1000, False, True, True, compare=False, split_at=9)
    e, _ = _run(product, d, 1000, False, True, True, compare=False, seed=dcases.PARITY_SEED + 1)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], c[k]), k
    both = np.intersect1d(a["id"], e["id"])
    assert both.size > 900
    ra, re = a["r"][np.isin(a["id"], both)], e["r"][np.isin(e["id"], both)]
    assert (ra != re).mean() > 0.9


def test_duplicate_ids_are_refused_while_diffusion_is_on(product):
    d = cases.parity_desc(product, 48, 256)
    ctx = driver.make_context(product, d)
    prm = cases.parity_params(product, d, cartesian=False)
    ones = np.ones(3)
    dup, distinct = np.array([5, 6, 5], dtype=np.uint64), np.array([5, 6, 7], dtype=np.uint64)
    ctx.particles_set(prm, dup, ones, ones, ones, ones, ones, ones)               # fine without diffusion
    with pytest.raises(B.FcptError, match="EINVAL.*distinct"):
        ctx.particles_diffusion(True, True, 1, 0)
    assert ctx.particles_diffusion_get().diffusion == 0                            # the refused call changed nothing
    ctx.particles_set(prm, distinct, ones, ones, ones, ones, ones, ones)
    ctx.particles_diffusion(True, True, 1, 0)
    with pytest.raises(B.FcptError, match="EINVAL.*distinct"):
        ctx.particles_set(prm, dup, ones, ones, ones, ones, ones, ones)
    assert ctx.particles_count() == 3                                              # ... and the particles stayed
    ctx.close()
