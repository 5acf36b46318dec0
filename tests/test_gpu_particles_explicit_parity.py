"""k_particles_step_explicit and k_particles_timestep_init against the numpy restatement
(tests/particles_explicit_ref.py) on the device's own gas: 8 gas steps of planet_disk with Jupiter on the 48 x 256 grid,
one download of Sigma, H, T, v_r, v_phi, then particles_timestep_init and calls of particles_step with the gas frozen, the
restatement stepping the same download.  Frame rotating with Omega = 1, non-zero indirect term.

Bars: the project's parity bar, 1e-10, over all live particles after every call, no exclusions, for the state (r, phi mod
2 pi, r_dot, r phi_dot, stokes, or position pair, velocity pair and stokes of the Cartesian form) and for r_ddot and
phi_ddot.  timestep and facold are ill-conditioned: ten times the yardstick that tests/test_particles_explicit_census.py
measures from the restatement alone, over the particles whose substep counts agree with the restatement's in every call
(at most 1 % may disagree).

r_ddot and phi_ddot are the mean acceleration over the last accepted substep.  Where a call is covered in one substep, or
split by the step size of init_particle_timestep, they are as well conditioned as the state.  Where a step size that has
been through the controller splits a call, the last substep begins where rounding puts it, and the restatement differs
from itself in longdouble by 1e-7 and more (tests/particles_explicit_cases.py has the figures).  The parity case steps at
dt = 1e-3, where they are well conditioned, and holds every particle to the bar.  The tests of many substeps below (the
encounter, the step-size sequence) hold all particles to the bar in the state; in r_ddot and phi_ddot they hold those that
covered the call in one substep to the bar and all of them, the many-substep lanes included, to ten times the yardstick
measured from the restatement in float64 against longdouble on the same sequence, as is done for timestep."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X

pytestmark = pytest.mark.gpu

BAR = 1e-10
GRIDS = (B.F_SIGMA, B.F_SCALE_HEIGHT, B.F_TEMPERATURE, B.F_VRAD, B.F_VAZI)


class Bench:
    """A context after 8 gas steps, its gas on the host, and what the restatement needs."""

    def __init__(self, product, adiabatic=False, gas_steps=8):
        self.d = d = cases.parity_desc(product, 48, 256, adiabatic=adiabatic)
        self.radii = product.radii(d)
        self.g = R.Grid(self.radii, d.nr_global, d.nphi)
        self.bodies = setups.jupiter_bodies(d)
        self.ctx = driver.make_context(product, d, radii=self.radii, bodies=self.bodies)
        if gas_steps:
            S = driver.SlabSet([self.ctx])
            S.prepare()
            S.run(gas_steps)
        self.prm = cases.parity_params(product, d, False)
        self.phys = X.physics(d, self.prm)
        self.gas = R.gas_fields(*(self.ctx.download(f) for f in GRIDS), d.density_factor)

    def upload(self, s, drag, cartesian, max_attempts=0, init=True):
        ctx = self.ctx
        ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, cartesian=cartesian, max_attempts=max_attempts)
        ctx.particles_diffusion(gas_drag=drag)
        ctx.particles_set(self.prm, s["id"], *(s[k] for k in R.FIELDS))
        if init:
            ctx.particles_timestep_init()
            X.init_timestep(self.phys, self.bodies, s, cartesian)
        else:
            ctx.particles_adaptive_set(s["timestep"], s["facold"])

    def step(self, s, dt, drag, cartesian, indirect=cases.PARITY_INDIRECT, frame=True, **kw):
        angle = self.d.omega_frame * dt if frame else 0.0
        self.ctx.particles_step(dt, indirect, angle)
        return X.step(self.g, self.gas, self.phys, self.bodies, s, dt, indirect, angle, drag=drag, cartesian=cartesian, **kw)


def ratio(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max()) if a.size else 0.0


def compare(ctx, s, cartesian, bar=BAR, acceleration_bar=None):
    """The state and the accelerations of all live particles against the bar.  With an acceleration_bar: the accelerations
    of all live particles against that one, and those of the particles that covered the call in one substep against the
    bar.  -> (device state, device adaptive state, worst difference)"""
    got, want = ctx.particles_get(), X.live(s)
    assert np.array_equal(got["id"], want["id"]), "the sets of live particles differ"
    assert np.array_equal(got["radius"], want["radius"])
    diff = X.worst_difference_cartesian(got, want) if cartesian else R.worst_difference(got, want)
    ad = ctx.particles_adaptive_get()
    one = (ad["accepted"] + ad["rejected"] == 1) & (want["accepted"] + want["rejected"] == 1)
    held = np.ones_like(one) if acceleration_bar is None else one
    for k in ("r_ddot", "phi_ddot"):
        scale = np.abs(want[k]).max() if want[k].size else 1.0
        diff[k] = float(np.abs(ad[k] - want[k])[held].max() / scale) if held.any() else 0.0
        if acceleration_bar is not None:
            every = float(np.abs(ad[k] - want[k]).max() / scale) if want[k].size else 0.0
            assert every <= acceleration_bar, (k, every, acceleration_bar)
    assert max(diff.values()) <= bar, diff
    return got, ad, max(diff.values())


def counts_differ(ad, s):
    m = s["alive"]
    return (ad["accepted"] != s["accepted"][m]) | (ad["rejected"] != s["rejected"][m])


@pytest.mark.parametrize("cartesian", [False, True])
@pytest.mark.parametrize("drag", [False, True])
@pytest.mark.parametrize("adiabatic", [False, True])
def test_explicit_step_matches_the_restatement(product, adiabatic, drag, cartesian):
    b = Bench(product, adiabatic)
    n = 1000
    s = xc.parity_state(product, b.d, b.radii, b.g, b.gas, b.phys, cartesian, n)
    b.upload(s, drag, cartesian)
    ad = b.ctx.particles_adaptive_get()
    assert ratio(ad["timestep"], s["timestep"]) <= BAR and np.array_equal(ad["facold"], s["facold"])   # init_particle_timestep
    marginal = np.zeros(n, dtype=bool)          # by slot
    worst, census, most = 0.0, {}, 0
    for call in range(xc.EXPLICIT_CALLS):
        slots = np.flatnonzero(s["alive"])
        assert not b.step(s, xc.EXPLICIT_DT, drag, cartesian, census=census).any()
        if drag and call == 0:     # after the first call: the particles that started on RMIN and RMAX
            assert s["alive"][15] and s["alive"][115]
        got, ad, w = compare(b.ctx, s, cartesian)
        worst = max(worst, w)
        still = s["alive"][slots]
        marginal[slots[still]] |= counts_differ(ad, s)
        most = max(most, int((ad["accepted"] + ad["rejected"]).max()))
    live = np.flatnonzero(s["alive"])
    keep = ~marginal[live]
    ts = xc.relative_difference(ad["timestep"][keep], s["timestep"][live][keep])
    fo = xc.relative_difference(ad["facold"][keep], s["facold"][live][keep])
    print("worst state difference %.3e; timestep %.3e, facold %.3e over %d of %d live particles (%d marginal); at most %d "
          "substeps per call; %s" % (worst, ts, fo, keep.sum(), live.size, marginal.sum(), most, census))
    b.ctx.close()
    assert census["escape_inward"] >= 5 and census["escape_outward"] >= 5      # mid-run escapes in both directions
    assert marginal.sum() <= xc.COUNT_MISMATCH_DEVICE * n
    assert ts <= xc.YARDSTICK_FACTOR * xc.YARDSTICK_TIMESTEP and fo <= xc.YARDSTICK_FACTOR * xc.YARDSTICK_FACOLD
    assert most * 100 <= X.MAX_ATTEMPTS


@pytest.fixture(scope="module")
def bench(product):
    b = Bench(product)
    yield b
    b.ctx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_the_wavefront_and_the_block(bench, product, n):
    s = X.add_adaptive(xc.explicit_draw(bench.d, bench.radii, n=n, seed=n))
    s["stokes"] = R.initial_stokes(bench.g, bench.gas, bench.phys, s)
    bench.upload(s, True, False)
    for _ in range(2):
        assert not bench.step(s, xc.EXPLICIT_DT, True, False).any()
        compare(bench.ctx, s, False)
    assert bench.ctx.particles_count() == int(s["alive"].sum()) >= n - 6


@pytest.mark.parametrize("cartesian", [False, True])
def test_dead_particles_between_live_ones(bench, product, cartesian):
    n = 130
    s = xc.explicit_draw(bench.d, bench.radii, n=n, seed=11)
    gone = np.arange(n) % 3 == 0             # these cross the outer escape radius in the first call
    s["r"][gone] = bench.d.rmax - 1e-4
    s["r_dot"][gone] = 0.2
    s["stokes"] = R.initial_stokes(bench.g, bench.gas, bench.phys, s)
    s = X.add_adaptive(xc.to_cartesian(s) if cartesian else s)
    bench.upload(s, True, cartesian)
    for call in range(3):
        assert not bench.step(s, xc.EXPLICIT_DT, True, cartesian).any()
        got, _, _ = compare(bench.ctx, s, cartesian)
        assert got["id"].size == n - gone.sum()
    assert not s["alive"][gone].any() and s["alive"][~gone].all()


def test_one_lane_in_a_close_encounter_among_63_neighbours(bench, product):
    s = xc.encounter_wavefront(bench.d, bench.radii)
    bench.upload(s, False, False)
    for _ in range(xc.ENCOUNTER_CALLS):
        assert not bench.step(s, xc.ENCOUNTER_DT, False, False).any()
        got, ad, worst = compare(bench.ctx, s, False, acceleration_bar=xc.YARDSTICK_FACTOR * xc.ENCOUNTER_ACCELERATION_YARDSTICK)
        sub = (ad["accepted"] + ad["rejected"]).astype(int)
        assert got["id"].size == 64 and sub[xc.ENCOUNTER_LANE] >= 4 * np.delete(sub, xc.ENCOUNTER_LANE).mean()
        assert sub.max() * 100 <= X.MAX_ATTEMPTS          # in every call
    print("substeps: lane %d, others mean %.1f; worst difference %.3e" % (sub[xc.ENCOUNTER_LANE], np.delete(sub, xc.ENCOUNTER_LANE).mean(), worst))
    assert got["id"].size == 64 and sub[xc.ENCOUNTER_LANE] >= 4 * np.delete(sub, xc.ENCOUNTER_LANE).mean()


@pytest.mark.parametrize("cartesian", [False, True])
def test_the_step_size_persists_between_calls_of_different_dt(bench, product, cartesian):
    ctx, last, most = bench.ctx, {}, [0]

    def init(s):
        bench.upload(s, False, cartesian)

    def after(s):
        last["got"], last["ad"], _ = compare(ctx, s, cartesian, acceleration_bar=xc.YARDSTICK_FACTOR * xc.STEP_SIZE_ACCELERATION_YARDSTICK)
        most[0] = max(most[0], int((last["ad"]["accepted"] + last["ad"]["rejected"]).max()))

    s, census = xc.step_size_sequence(bench.d, bench.radii, cartesian, init,
                                      lambda s, dt, census: bench.step(s, dt, False, cartesian, census=census),
                                      plant=ctx.particles_adaptive_set, after=after)
    got, ad = last["got"], last["ad"]
    print(census)
    assert census["rejection"] >= 200 and census["accepted_after_rejection"] >= 200
    assert most[0] * 100 <= X.MAX_ATTEMPTS
    agree = ~counts_differ(ad, s)
    assert 1.0 - agree.mean() <= xc.STEP_SIZE_COUNT_MISMATCH      # twice the share on which the two restatements disagree
    live = s["alive"]
    ts = xc.relative_difference(ad["timestep"][agree], s["timestep"][live][agree])
    print("timestep %.3e over %d of %d" % (ts, agree.sum(), agree.size))
    assert ts <= xc.YARDSTICK_FACTOR * xc.STEP_SIZE_YARDSTICK
    # dt = 0 terminates, moves nothing and keeps every step size, bit for bit (frame at rest, no indirect term)
    ctx.particles_step(0.0)
    after0, ad0 = ctx.particles_get(), ctx.particles_adaptive_get()
    for k in ("r", "phi", "r_dot", "phi_dot"):
        assert np.array_equal(after0[k], got[k]), k
    assert np.array_equal(ad0["timestep"], ad["timestep"])
    assert np.all(ad0["accepted"] == 1) and np.all(ad0["rejected"] == 0)
