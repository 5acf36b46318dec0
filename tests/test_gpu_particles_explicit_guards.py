"""Guards 9 and 10 of k_particles_step_explicit.  Each case returns at once by construction: the attempt cap is an integer
comparison at the head of the loop, so a particle that would need more substeps, or whose step size is NaN, gives up after
max_attempts passes, is reported once with its id, and is left bit-identical to its upload, timestep and facold included;
its neighbours are stepped as the restatement steps them."""
import numpy as np
import pytest

from fargocpt_amd import binding as B

import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X
from tests.test_gpu_particles_explicit_parity import BAR, Bench, compare

pytestmark = pytest.mark.gpu

VICTIM = 40


@pytest.fixture(scope="module")
def bench(product):
    b = Bench(product)
    yield b
    b.ctx.close()


def _check(bench, s, drag, cartesian, guard, dt, max_attempts=0):
    ctx = bench.ctx
    before = ctx.particles_get()
    before.update(ctx.particles_adaptive_get())
    want = bench.step(s, dt, drag, cartesian, frame=False, indirect=(0.0, 0.0), max_attempts=max_attempts or X.MAX_ATTEMPTS)
    assert want[VICTIM] == guard and np.count_nonzero(want) == 1
    with pytest.raises(B.FcptError, match=r"particle id %d .*guard %d " % (int(s["id"][VICTIM]), guard)):
        ctx.particles_count()
    assert ctx.particles_count() == s["id"].size            # reported once; the particle lives on
    got, ad, _ = compare(ctx, s, cartesian, BAR)
    got.update(ad)
    for k in ("r", "phi", "r_dot", "phi_dot", "stokes", "timestep", "facold", "r_ddot", "phi_ddot", "accepted", "rejected"):
        assert np.array_equal(got[k][VICTIM:VICTIM + 1], before[k][VICTIM:VICTIM + 1], equal_nan=True), k     # bit for bit
    others = np.arange(s["id"].size) != VICTIM
    assert np.all(got["accepted"][others] >= 1)              # the neighbours were stepped


def _draw(bench, cartesian):
    s = xc.explicit_draw(bench.d, bench.radii, n=65, seed=7)
    s["stokes"] = R.initial_stokes(bench.g, bench.gas, bench.phys, s)
    return X.add_adaptive(xc.to_cartesian(s) if cartesian else s)


@pytest.mark.parametrize("cartesian", [False, True])
def test_attempt_cap_on_a_particle_that_needs_more(bench, cartesian):
    s = _draw(bench, cartesian)
    bench.upload(s, False, cartesian, max_attempts=3)
    h = bench.ctx.particles_adaptive_get()["timestep"]
    f = np.full(65, 1.0e-4)
    h[VICTIM] = 1.0e-9              # an accepted step grows tenfold at most: 1e-9 .. 1e-5 are five attempts, and 1e-3 is not reached
    s["timestep"], s["facold"] = h.copy(), f.copy()
    bench.ctx.particles_adaptive_set(h, f)
    _check(bench, s, False, cartesian, X.GUARD_ATTEMPTS, 1.0e-3, max_attempts=3)


def test_nan_step_size_ends_at_the_attempt_cap(bench):
    s = _draw(bench, False)
    bench.upload(s, True, False)
    ad = bench.ctx.particles_adaptive_get()
    h, f = ad["timestep"], ad["facold"]
    h[VICTIM] = np.nan
    s["timestep"], s["facold"] = h.copy(), f.copy()
    bench.ctx.particles_adaptive_set(h, f)
    _check(bench, s, True, False, X.GUARD_ATTEMPTS, xc.EXPLICIT_DT)


@pytest.mark.parametrize("cartesian", [False, True])
def test_stiff_grain_trips_guard_10(bench, cartesian):
    s = xc.explicit_draw(bench.d, bench.radii, n=65, seed=7)
    s["radius"][VICTIM] = xc.STIFF_GRAIN
    s["stokes"] = R.initial_stokes(bench.g, bench.gas, bench.phys, s)
    s = X.add_adaptive(xc.to_cartesian(s) if cartesian else s)
    bench.upload(s, True, cartesian)
    _check(bench, s, True, cartesian, X.GUARD_STIFF, xc.EXPLICIT_DT)
