"""The contract of the entry points of the explicit adaptive integrator: what is refused and by name, what invalidates the
adaptive state, round trips, permutation of the upload, and that a context which selected the explicit integrator and
went back computes the midpoint bits of tests/golden/particles_parent_bits.json."""
import json

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X
import tests.test_gpu_particles_default_bits as bits
from tests.test_gpu_particles_explicit_parity import Bench

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bench(product):
    b = Bench(product)
    yield b
    b.ctx.close()


def _draw(bench, n=65):
    s = xc.explicit_draw(bench.d, bench.radii, n=n, seed=9)
    s["stokes"] = R.initial_stokes(bench.g, bench.gas, bench.phys, s)
    return X.add_adaptive(s)


def test_no_step_from_an_unset_step_size(bench):
    ctx, s = bench.ctx, _draw(bench)
    ctx.particles_diffusion(gas_drag=True)
    ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT)
    ctx.particles_set(bench.prm, s["id"], *(s[k] for k in R.FIELDS))
    counter = ctx.particles_diffusion_get().step
    with pytest.raises(B.FcptError, match="EINVAL.*fcpt_particles_timestep_init or fcpt_particles_adaptive_set"):
        ctx.particles_step(xc.EXPLICIT_DT)
    assert ctx.particles_diffusion_get().step == counter + 1         # the Philox counter advances on every call
    ctx.particles_timestep_init()
    ctx.particles_step(xc.EXPLICIT_DT)
    assert np.all(ctx.particles_adaptive_get()["accepted"] >= 1)
    ctx.particles_set(bench.prm, s["id"], *(s[k] for k in R.FIELDS))     # set invalidates the adaptive state
    with pytest.raises(B.FcptError, match="fcpt_particles_timestep_init"):
        ctx.particles_step(xc.EXPLICIT_DT)
    with pytest.raises(B.FcptError, match="no adaptive state"):
        ctx.particles_adaptive_get()
    ctx.particles_adaptive_set(np.full(65, 1e-3), np.full(65, 1e-4))
    ctx.particles_step(xc.EXPLICIT_DT)
    assert ctx.particles_count() == 65


def test_adaptive_set_and_get_round_trip_bit_for_bit(bench):
    ctx, s = bench.ctx, _draw(bench)
    ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT)
    ctx.particles_set(bench.prm, s["id"], *(s[k] for k in R.FIELDS))
    rng = np.random.default_rng(1)
    h, f = rng.uniform(1e-6, 1e-1, 65), rng.uniform(1e-4, 1.0, 65)
    h[3], f[5] = np.nextafter(0.0, 1.0), np.nextafter(1.0, 0.0)
    ctx.particles_adaptive_set(h, f)
    got = ctx.particles_adaptive_get()
    assert np.array_equal(got["timestep"], h) and np.array_equal(got["facold"], f)
    assert not got["accepted"].any() and not got["rejected"].any() and not got["r_ddot"].any()
    with pytest.raises(B.FcptError, match="particle slots"):
        ctx.particles_adaptive_set(h[:64], f[:64])


def test_settings_that_are_refused_change_nothing(bench, product):
    ctx = driver.make_context(product, bench.d, radii=bench.radii)
    same = lambda p, q: (p.kind, p.cartesian, p.max_attempts) == q
    assert same(ctx.particles_integrator_get(), (0, 0, 0))
    # explicit, then diffusion: the second call is refused
    ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, cartesian=True, max_attempts=77)
    with pytest.raises(B.FcptError, match="EINVAL.*diffusion.*explicit adaptive integrator"):
        ctx.particles_diffusion(gas_drag=False, diffusion=True, seed=5, step=9)
    p = ctx.particles_diffusion_get()
    assert (p.gas_drag, p.diffusion, p.seed, p.step) == (1, 0, 0, 0)
    assert same(ctx.particles_integrator_get(), (1, 1, 77))
    # diffusion, then explicit
    ctx.particles_integrator(kind=B.INTEGRATOR_MIDPOINT)
    ctx.particles_diffusion(gas_drag=True, diffusion=True, seed=5, step=9)
    with pytest.raises(B.FcptError, match="EINVAL.*explicit adaptive integrator.*diffusion"):
        ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, max_attempts=5)
    assert same(ctx.particles_integrator_get(), (0, 0, 0))
    ctx.particles_diffusion(gas_drag=True, diffusion=False)
    with pytest.raises(B.FcptError, match="EINVAL.*cartesian = 1 needs the explicit"):
        ctx.particles_integrator(kind=B.INTEGRATOR_MIDPOINT, cartesian=True)
    with pytest.raises(B.FcptError, match="EINVAL.*max_attempts"):
        ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, max_attempts=-1)
    with pytest.raises(B.FcptError, match="EINVAL.*kind"):
        ctx.particles_integrator(kind=2)
    assert same(ctx.particles_integrator_get(), (0, 0, 0))
    with pytest.raises(B.FcptError, match="select the explicit adaptive integrator first"):
        ctx.particles_timestep_init()
    # the settings outlive particles_set
    ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, max_attempts=123)
    one = np.ones(1)
    ctx.particles_set(bench.prm, np.zeros(1, dtype=np.uint64), one, one, one, one, one, one)
    assert same(ctx.particles_integrator_get(), (1, 0, 123))
    ctx.close()


@pytest.mark.parametrize("cartesian", [False, True])
def test_permuting_the_upload_permutes_the_results_bit_for_bit(bench, cartesian):
    s = _draw(bench, 257)
    if cartesian:
        s = X.add_adaptive(xc.to_cartesian(s))
    perm = np.random.default_rng(4).permutation(257)
    results = []
    for order in (np.arange(257), perm):
        t = {k: v[order] for k, v in s.items()}
        bench.upload(t, True, cartesian)
        for _ in range(3):
            bench.ctx.particles_step(xc.EXPLICIT_DT, cases.PARITY_INDIRECT, bench.d.omega_frame * xc.EXPLICIT_DT)
        out = bench.ctx.particles_get()
        out.update(bench.ctx.particles_adaptive_get())
        results.append(out)
    a, b = results
    ia, ib = np.argsort(a["id"]), np.argsort(b["id"])
    assert a["id"].size >= 250 and not np.array_equal(a["id"], b["id"])
    for k in a:
        assert np.array_equal(a[k][ia], b[k][ib]), k


class _ExplicitAndBack:
    """The library, with contexts that select the explicit integrator with its Cartesian state and an attempt cap, and
    go back to the midpoint integrator before anything is uploaded."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def create(self, d, radii):
        ctx = self._lib.create(d, radii)
        ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, cartesian=True, max_attempts=50)
        ctx.particles_integrator(kind=B.INTEGRATOR_MIDPOINT)
        return ctx


@pytest.mark.parametrize("case", bits.CASES, ids=[bits.case_key(*c) for c in bits.CASES])
def test_back_to_the_midpoint_integrator_gives_the_parent_bits(product, case):
    want = json.load(open(bits.GOLDEN))["cases"][bits.case_key(*case)]
    assert bits.hashes(_ExplicitAndBack(product), case) == want


def test_midpoint_bits_after_explicit_steps_in_the_same_context(bench):
    """Explicit steps, then the same upload stepped by the midpoint integrator: the bits of a context that never left it."""
    s = _draw(bench, 257)
    outs = []
    for detour in (False, True):
        ctx = bench.ctx
        if detour:
            bench.upload(s, True, False)
            ctx.particles_step(xc.EXPLICIT_DT)
            ctx.particles_count()
        ctx.particles_integrator(kind=B.INTEGRATOR_MIDPOINT)
        ctx.particles_set(bench.prm, s["id"], *(s[k] for k in R.FIELDS))
        for _ in range(3):
            ctx.particles_step(cases.PARITY_DT, cases.PARITY_INDIRECT, bench.d.omega_frame * cases.PARITY_DT)
        outs.append(ctx.particles_get())
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
