"""fcpt_particles_follow_run_steps: the particle step inside fcpt_run_steps -- step length, frame angle and Philox counter
from device memory, plain launches and the replayed hipGraph -- against the host-stepped loop over the ABI the feature does
not touch: per step fcpt_cfl, fcpt_calculate_timestep, fcpt_particles_step(dt, indirect, OmegaFrame * dt), fcpt_step,
fcpt_post.

Both loops launch the same kernels with the same operands, so the bar is bit equality (np.array_equal): ids, the six state
arrays and the live count, clock.time, Sigma, v_r, v_phi (and e), and for the explicit integrator everything
particles_adaptive_get returns.

planet_disk with Jupiter on 48 x 256 (48 x 96 for the ideal EOS), OmegaFrame = 0.9, a non-zero indirect term, 300 particles
(a block of 256 and a tail of 44 lanes).  The particles are the bulk of the parity draws (tests/particles_cases.py,
particles_explicit_cases.py) between r = 0.6 and 2.0, away from both escape radii; every test asserts that the host-stepped
loop alone trips no guard and keeps every particle alive."""
import ctypes as C

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups

import tests.particles_cases as cases
import tests.particles_diffusion_cases as dc
import tests.particles_explicit_cases as xc
import tests.particles_ref as R

pytestmark = pytest.mark.gpu

N = 300
INDIRECT = cases.PARITY_INDIRECT
SEED = dc.PARITY_SEED
ADAPTIVE = B.ADAPTIVE_FIELDS + ("accepted", "rejected")


def bulk(draw, d, radii, n=N):
    """The first n particles of three small draws (below 200 the draws are their bulk alone) that start inside [0.6, 2.0]."""
    parts = [draw(d, radii, n=199, seed=seed) for seed in (20240611, 20250307, 20260101)]
    s = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    keep = np.flatnonzero((s["r"] > 0.6) & (s["r"] < 2.0))[:n]
    assert keep.size == n
    s = {k: v[keep] for k, v in s.items()}
    s["id"] = dc.distinct_ids(n)
    return s


class Pair:
    """Two contexts from the same fields: `host` is stepped by the host-stepped loop, `dev` by run_steps with follow on."""

    def __init__(self, product, adiabatic=False, graph=0, explicit=False, monitor=None):
        # (OmegaFrame = 0.9, not 1: with 1 the product OmegaFrame * dt is dt, and a fused phi - OmegaFrame * dt would round
        #  like the separate product and subtraction of the host-stepped loop)
        self.d = d = cases.parity_desc(product, 48, 96 if adiabatic else 256, adiabatic=adiabatic, omega_frame=0.9)
        if monitor is not None:
            d.monitor_timestep, d.nmonitor, d.nsnapshots = monitor, 1, 1000
        assert d.omega_frame != 0.0
        self.radii = product.radii(d)
        fields = product.initial_fields(d.copy(), self.radii)
        self.prm = cases.parity_params(product, d, False)
        self.bodies = setups.jupiter_bodies(d)
        self.ctxs = []
        for _ in range(2):
            ctx = driver.make_context(product, d, fields=fields, radii=self.radii, bodies=self.bodies)
            ctx.set_bodies(*self.bodies, indirect=INDIRECT)
            ctx.set_option("graph_steps", graph)
            driver.SlabSet([ctx]).prepare()
            self.ctxs.append(ctx)
        self.host, self.dev = self.ctxs
        self.dev.particles_follow_run_steps(True)
        self.indirect = INDIRECT
        self.state = bulk(xc.explicit_draw if explicit else cases.census_draw, d, self.radii)

    def each(self, f):
        for ctx in self.ctxs:
            f(ctx)

    def upload(self, s=None):
        s = self.state if s is None else s
        self.each(lambda ctx: ctx.particles_set(self.prm, s["id"], *(s[k] for k in R.FIELDS)))

    def host_steps(self, nsteps, snap=False, particles=True):
        ctx, d = self.host, self.d
        for _ in range(nsteps):
            clk = ctx.clock
            dt = ctx.calculate_timestep(ctx.cfl())
            step_dt = ctx.snap_to_monitor(dt) if snap else dt
            if particles:
                ctx.particles_step(step_dt, self.indirect, d.omega_frame * step_dt)
            ctx.step(step_dt)
            ctx.post(step_dt)
            if snap and abs((clk.n_monitor + 1) * d.monitor_timestep - ctx.clock.time) < 1e-6 * dt:   # fcpt_run_steps, snap != 0
                now = ctx.clock
                now.n_monitor = clk.n_monitor + 1
                now.n_snapshot = now.n_monitor // max(d.nmonitor, 1)
                ctx.clock = now

    def assert_equal(self, adaptive=False, expect_alive=None, skip_id=None):
        """-> the host loop's particles; the host loop tripped no guard (particles_count would raise) and lost nobody"""
        want_n, got_n = self.host.particles_count(), self.dev.particles_count()
        assert want_n == (N if expect_alive is None else expect_alive)
        assert got_n == want_n
        want, got = self.host.particles_get(), self.dev.particles_get()
        for k in ("id",) + R.FIELDS:
            assert np.array_equal(got[k], want[k]), k
        if adaptive:
            wa, ga = self.host.particles_adaptive_get(), self.dev.particles_adaptive_get()
            m = np.ones(want_n, dtype=bool) if skip_id is None else want["id"] != skip_id
            for k in ADAPTIVE:
                assert np.array_equal(ga[k], wa[k]), k
            assert int((wa["accepted"] + wa["rejected"])[m].max()) <= 100
        ch, cd = self.host.clock, self.dev.clock
        assert (cd.time, cd.last_dt, cd.n_hydro_iter, cd.n_monitor, cd.n_snapshot) == \
               (ch.time, ch.last_dt, ch.n_hydro_iter, ch.n_monitor, ch.n_snapshot)
        sh, sd = self.host.state(), self.dev.state()
        assert set(sh) == set(sd) and ("energy" in sh) == (self.d.eos == B.EOS_IDEAL)
        for k in sh:
            assert np.array_equal(sd[k], sh[k]), k
        return want

    def close(self):
        self.each(lambda ctx: ctx.close())


def test_plain_launches_midpoint(product):
    p = Pair(product)
    p.upload()
    assert p.dev.particles_follow_run_steps_get() and not p.host.particles_follow_run_steps_get()
    p.host_steps(12)
    assert p.dev.run_steps(12) == 12
    assert p.dev.get_option("graph_replays") == 0
    after = p.assert_equal()
    assert not np.array_equal(after["r"], p.state["r"]) and not np.array_equal(after["phi"], p.state["phi"])
    # follow off: the particles stay the upload, bit for bit, and the gas is the same gas
    off = driver.make_context(product, p.d, fields=product.initial_fields(p.d.copy(), p.radii), radii=p.radii, bodies=p.bodies)
    off.set_bodies(*p.bodies, indirect=INDIRECT)
    off.set_option("graph_steps", 0)
    driver.SlabSet([off]).prepare()
    s = p.state
    off.particles_set(p.prm, s["id"], *(s[k] for k in R.FIELDS))
    assert off.run_steps(12) == 12
    got = off.particles_get()
    for k in ("id",) + R.FIELDS:
        assert np.array_equal(got[k], s[k]), k
    assert off.clock.time == p.dev.clock.time
    gas, gas_on = off.state(), p.dev.state()
    for k in gas:
        assert np.array_equal(gas[k], gas_on[k]), k
    off.close()
    p.close()


def test_ideal_eos(product):
    p = Pair(product, adiabatic=True)
    p.upload()
    p.host_steps(12)
    assert p.dev.run_steps(12) == 12
    p.assert_equal()
    p.close()


def test_graph_replay(product):
    p = Pair(product, graph=1)
    p.upload()
    p.host_steps(36)
    before = p.dev.get_option("graph_replays")
    for k in (21, 12, 3):
        assert p.dev.run_steps(k) == k
    assert p.dev.get_option("graph_replays") > before
    p.assert_equal()
    p.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("drag", [True, False])
def test_diffusion_across_the_word_boundary_of_the_counter(product, drag, graph):
    p = Pair(product, graph=graph)
    start, steps = 2 ** 32 - 3, 12
    p.each(lambda ctx: ctx.particles_diffusion(gas_drag=drag, diffusion=True, seed=SEED, step=start))
    p.upload()
    p.host_steps(steps)
    assert p.dev.run_steps(steps) == steps
    assert p.dev.particles_diffusion_get().step == start + steps == p.host.particles_diffusion_get().step
    p.assert_equal()
    # the counter the device loop left is the one the next host-stepped step draws with
    host = p.host
    p.host_steps(1)
    p.host = p.dev
    p.host_steps(1)
    p.host = host
    assert p.dev.particles_diffusion_get().step == start + steps + 1
    p.assert_equal()
    p.close()


@pytest.mark.parametrize("graph", [0, 1])
@pytest.mark.parametrize("cartesian", [False, True])
def test_explicit_integrator(product, cartesian, graph):
    p = Pair(product, graph=graph, explicit=True)
    p.each(lambda ctx: ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, cartesian=cartesian))
    p.upload(xc.to_cartesian(p.state) if cartesian else p.state)
    p.each(lambda ctx: ctx.particles_timestep_init())
    p.host_steps(12)
    assert p.dev.run_steps(12) == 12
    p.assert_equal(adaptive=True)
    p.close()


def test_a_captured_graph_is_dropped_when_the_particle_launch_changes(product):
    p = Pair(product, graph=1)
    p.upload()

    def round_trip(adaptive=False, expect_alive=None):
        replays = p.dev.get_option("graph_replays")
        p.host_steps(12)
        assert p.dev.run_steps(12) == 12
        assert p.dev.get_option("graph_replays") > replays
        p.assert_equal(adaptive=adaptive, expect_alive=expect_alive)

    round_trip()
    # another count
    few = {k: v[:130] for k, v in p.state.items()}
    p.upload(few)
    round_trip(expect_alive=130)
    # diffusion on, and off again
    p.each(lambda ctx: ctx.particles_diffusion(gas_drag=True, diffusion=True, seed=SEED, step=5))
    round_trip(expect_alive=130)
    p.each(lambda ctx: ctx.particles_diffusion(gas_drag=True, diffusion=False, seed=SEED, step=17))
    round_trip(expect_alive=130)
    # the explicit integrator, on weakly coupled bodies, with step sizes of its own
    heavy = bulk(xc.explicit_draw, p.d, p.radii)
    p.each(lambda ctx: ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT))
    p.upload(heavy)
    p.each(lambda ctx: ctx.particles_timestep_init())
    round_trip(adaptive=True)
    p.each(lambda ctx: ctx.particles_timestep_init())       # the same arrays, initialised anew
    round_trip(adaptive=True)
    p.each(lambda ctx: ctx.particles_integrator(kind=B.INTEGRATOR_MIDPOINT))
    round_trip()
    # the planet elsewhere, another indirect term
    x, y, m = p.bodies
    p.indirect = (-1.0e-4, 2.5e-4)
    p.each(lambda ctx: ctx.set_bodies([0.0, 0.0], [0.0, 1.0], m, indirect=p.indirect))
    round_trip()
    # follow off: a graph without the particle launch is captured and replayed, the particles stay where they are
    p.dev.particles_follow_run_steps(False)
    before = p.dev.particles_get()
    replays = p.dev.get_option("graph_replays")
    p.host_steps(12, particles=False)
    assert p.dev.run_steps(12) == 12
    assert p.dev.get_option("graph_replays") > replays
    p.assert_equal()
    after = p.dev.particles_get()
    for k in ("id",) + R.FIELDS:
        assert np.array_equal(after[k], before[k]), k
    # ... and on again
    p.dev.particles_follow_run_steps(True)
    round_trip()
    p.close()


def test_a_guard_tripped_inside_run_steps_is_reported_once(product):
    p = Pair(product, explicit=True)
    p.each(lambda ctx: ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT))
    s = p.state
    stiff_id = np.uint64(77)
    one = R.make_state([stiff_id], [1.5], [np.pi], [0.0], [1.5 ** -1.5], [xc.STIFF_GRAIN], [0.0])   # t_stop < 10 dt: guard 10
    s = {k: np.concatenate([s[k], one[k]]) for k in s}
    p.upload(s)
    p.each(lambda ctx: ctx.particles_timestep_init())
    p.host_steps(12)
    assert p.dev.run_steps(12) == 12
    for ctx in p.ctxs:
        with pytest.raises(B.FcptError, match=r"particle id 77 tripped guard 10"):
            ctx.particles_count()
    got = p.assert_equal(adaptive=True, expect_alive=N + 1, skip_id=stiff_id)      # the call after the report works
    k = int(np.flatnonzero(got["id"] == stiff_id)[0])
    for f in R.FIELDS:                                                               # left exactly as it was
        assert got[f][k] == one[f][0], f
    p.close()


def _run_steps_raw(ctx, nsteps, snap=0):
    done = C.c_int64(99)
    rc = ctx.lib.fn("run_steps")(ctx._h, C.c_int64(nsteps), C.c_int32(snap), C.byref(done))
    return rc, done.value


def test_refusals(product):
    # the explicit integrator without step sizes since the last particles_set
    p = Pair(product, explicit=True)
    p.dev.particles_integrator(kind=B.INTEGRATOR_EXPLICIT)
    s = p.state
    p.dev.particles_set(p.prm, s["id"], *(s[k] for k in R.FIELDS))
    c0 = p.dev.clock
    for snap in (0, 1):
        rc, done = _run_steps_raw(p.dev, 12, snap)
        assert rc != 0 and done == 0
        with pytest.raises(B.FcptError, match="no step sizes since the last fcpt_particles_set"):
            p.dev.run_steps(12, snap=bool(snap))
    c1 = p.dev.clock
    assert (c1.time, c1.n_hydro_iter, c1.last_dt) == (c0.time, c0.n_hydro_iter, c0.last_dt)
    p.dev.particles_timestep_init()
    assert p.dev.run_steps(12) == 12
    p.close()
    # Integrator: Leapfrog
    d = cases.parity_desc(product, 48, 256)
    d.integrator = B.INTEGRATOR_LEAPFROG
    ctx = driver.make_context(product, d, bodies=setups.jupiter_bodies(d))
    driver.SlabSet([ctx]).prepare()
    assert ctx.run_steps(8) == 8
    ctx.particles_follow_run_steps(True)
    c0 = ctx.clock
    rc, done = _run_steps_raw(ctx, 12)
    assert rc != 0 and done == 0
    with pytest.raises(B.FcptError, match="Leapfrog"):
        ctx.run_steps(12)
    c1 = ctx.clock
    assert (c1.time, c1.n_hydro_iter) == (c0.time, c0.n_hydro_iter)
    ctx.particles_follow_run_steps(False)
    assert ctx.run_steps(8) == 8
    ctx.close()


@pytest.mark.parametrize("graph", [0, 1])
def test_follow_without_particles_counts_the_steps(product, graph):
    p = Pair(product, graph=graph)
    p.dev.particles_diffusion(gas_drag=True, diffusion=True, seed=SEED, step=40)
    p.host.particles_diffusion(gas_drag=True, diffusion=True, seed=SEED, step=40)
    p.host_steps(20)
    assert p.dev.run_steps(20) == 20
    assert p.dev.particles_diffusion_get().step == 60 == p.host.particles_diffusion_get().step
    p.assert_equal(expect_alive=0)
    p.close()


def test_snap_to_monitor(product):
    p = Pair(product, monitor=0.02)
    p.upload()
    steps = 0
    while p.host.clock.n_monitor < 2:
        p.host_steps(1, snap=True)
        steps += 1
        assert steps < 60
    assert p.dev.run_steps(steps, snap=True) == steps
    assert p.dev.clock.n_monitor == 2
    assert p.dev.particles_diffusion_get().step == steps
    p.assert_equal()
    p.close()
