"""fcpt_particles_follow_run_steps on several slabs: the particle step and the migration inside fcpt_run_steps.

Two identical sets of slabs from the same fields, every context on a host-link communicator, one thread per slab.  Set A
calls run_steps(K) with follow on.  Set B is stepped from the host over the ABI the feature does not touch, per step
cfl_allreduce -> calculate_timestep -> [snap_to_monitor] -> particles_step(dt, indirect, OmegaFrame * dt) ->
particles_migrate -> step -> exchange -> post.

Both loops launch the same kernels on the same operands (the clock forms and the slab forms of the particle kernels are each
bit-equal to the host-argument one-slab kernel, and the in-loop message is a prefix of the full one), so the bar is bit
equality, np.array_equal: derived, not measured.  Compared: merged ids and the six state arrays (the adaptive fields for the
explicit integrator), the summed live count, every slab's Sigma, v_r, v_phi (and e) and clock, the particle counter and the
sums over the slabs of the migration counters.

planet_disk with Jupiter on 48 x 256 (48 x 96 for the ideal EOS), OmegaFrame = 0.9, a non-zero indirect term.  The step is
the CFL policy's: FirstDT = 1e-3 growing by CFLmaxVar = 1.1 per call, 1.2e-3 after sim::init and 3.8e-3 after K = 12 steps;
a crosser planted at a tenth of the Kepler speed covers about 1 % of a ring width per step.  Conditions that keep a pass
from hiding an empty test are asserted on set B alone."""
import functools
import threading

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X
import tests.particles_slab_cases as sc

pytestmark = pytest.mark.gpu

K = 12
N = 1000
INDIRECT = cases.PARITY_INDIRECT
OMEGA_FRAME = 0.9
SEED = 20250921
MONITOR = 0.01          # the 6th step passes it (the steps sum to 1.0e-2 after 6, to 2.8e-2 after 12)
GRIDS = (B.F_SIGMA, B.F_SCALE_HEIGHT, B.F_TEMPERATURE, B.F_VRAD, B.F_VAZI)
COMPARED = ("id",) + R.FIELDS
COUNTERS = ("sent_inner", "sent_outer", "received", "deferred")
LINK_TIMEOUT = "30"     # seconds: a failing slab does not hold the others for the built-in two minutes


def _in_threads(fns):
    out, err = [None] * len(fns), []

    def run(k):
        try:
            out[k] = fns[k]()
        except Exception as e:  # noqa: BLE001 -- reported below
            err.append((k, e))

    ts = [threading.Thread(target=run, args=(k,)) for k in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(180)
    assert not err, err
    assert not any(t.is_alive() for t in ts)
    return out


def _desc(product, adiabatic, monitor=None, leapfrog=False):
    d = cases.parity_desc(product, 48, 96 if adiabatic else 256, adiabatic=adiabatic, omega_frame=OMEGA_FRAME)
    if monitor is not None:
        d.monitor_timestep, d.nmonitor, d.nsnapshots = monitor, 1, 1000
    if leapfrog:
        d.integrator = B.INTEGRATOR_LEAPFROG
    return d


@functools.lru_cache(maxsize=None)
def _start(product, adiabatic):
    """Computed once per EOS and left unchanged: -> (radii, bodies, global initial fields, the restatement's gas of the
    prepared one-slab state, the step length sim::init leaves in the clock)."""
    d = _desc(product, adiabatic)
    radii = product.radii(d)
    bodies = setups.jupiter_bodies(d)
    fields = product.initial_fields(d.copy(), radii)
    ctx = driver.make_context(product, d, fields=fields, radii=radii, bodies=bodies)
    driver.SlabSet([ctx]).prepare()
    gas = R.gas_fields(*(ctx.download(f) for f in GRIDS), d.density_factor)
    dt0 = ctx.clock.last_dt
    ctx.close()
    return radii, bodies, fields, gas, dt0


def _harden(g, gas, phys, s, dt_last):
    """Stokes numbers of the state; for the explicit kick grains are enlarged until t_stop >= 20 dt at the longest step of
    the run (guard 10 is t_stop < 10 dt, and the draws of particles_explicit_cases.py were sized for dt = 1e-3)."""
    for _ in range(4):
        stokes = R.initial_stokes(g, gas, phys, s)
        if dt_last is None:
            return stokes
        stiff = stokes / R.omega_kepler(phys, s["r"]) < 20.0 * dt_last
        if not stiff.any():
            return stokes
        s["radius"][stiff] *= 10.0
    raise AssertionError("the explicit draw stays stiff")


def _draw(product, d, case, adiabatic, calm=False):
    """-> (params, state, plants, slots of the draw's escapers)"""
    radii, bodies, fields, gas, dt0 = _start(product, adiabatic)
    g = R.Grid(radii, d.nr_global, d.nphi)
    prm = cases.parity_params(product, d, False)
    edges = sc.interior_edges(product, d, radii)
    # a planted crosser moves at a tenth of the Kepler speed: far less than one ring width per step, at the last step too
    dt_last = dt0 * d.cfl_max_var ** K
    for edge in edges:
        row = int(np.flatnonzero(g.rinf == edge)[0])
        assert 0.1 * np.sqrt(d.G * d.hydro_center_mass / edge) * dt_last < g.rinf[row + 1] - g.rinf[row]
    if case.startswith("explicit"):
        phys = X.physics(d, prm)
        s = xc.explicit_draw(d, radii, n=N, dt=dt0, calls=K)
        plants = sc.plant_crossers(s, d, radii, edges, dt0, K)
        s["stokes"] = _harden(g, gas, phys, s, dt_last)
        if case == "explicit-cartesian":
            s = xc.to_cartesian(s)
        s = X.add_adaptive(s)
    else:
        # the draw of slab_draw.  The census' enterers cover 1.1 to 1.5 edge cells per `dt`: sized for the longest step, so
        # that their half drift stays inside the overlap wherever they get to.  The first step is a third of that one: it
        # leaves them outside the escape radius, where move() removes them -- here they count among the escapers
        s = cases.census_draw(d, radii, n=N, dt=dt_last)
        if calm:            # (slab_draw: without the enterers, for migrate_capacity = 1)
            k = np.arange(N)
            for sel, edge, sign in ((k % 100 == 13, d.rmin, 1.0), (k % 100 == 14, d.rmax, -1.0)):
                v = 0.1 * np.sqrt(d.G * d.hydro_center_mass / edge)
                s["r"][sel] = edge + sign * v * dt_last
                s["r_dot"][sel] = sign * v
                s["phi_dot"][sel] = np.sqrt(d.G * d.hydro_center_mass / s["r"][sel] ** 3)
        plants = sc.plant_crossers(s, d, radii, edges, dt0, K)
        s["stokes"] = _harden(g, gas, R.physics(d, prm), s, None)
    gone = (11, 12) if calm or case.startswith("explicit") else (11, 12, 13, 14)
    escapers = {k for k in range(N) if k % 100 in gone}           # the leavers next to the escape radii
    return prm, s, plants, escapers


class Sets:
    """Two sets of `nslabs` slabs from the same fields, each set on a host link of its own, after sim::init's sequence."""

    def __init__(self, product, tmp_path, monkeypatch, nslabs=3, adiabatic=False, monitor=None, overlap=0, leapfrog=False,
                 prepare=True, tag=""):
        monkeypatch.setenv("FCPT_HOSTLINK_TIMEOUT", LINK_TIMEOUT)       # ahead of the first comm_init_host
        self.d = d = _desc(product, adiabatic, monitor, leapfrog)
        self.radii, self.bodies, fields, _, _ = _start(product, adiabatic)
        self.nslabs, self.adiabatic = nslabs, adiabatic
        self.sets = []
        for name in ("a", "b"):
            ctxs = []
            for dk in sc.slab_descs(d, nslabs):
                ctx = driver.make_context(product, dk, fields=sc.cut_fields(product, dk, fields), radii=self.radii, bodies=self.bodies)
                ctx.set_bodies(*self.bodies, indirect=INDIRECT)
                ctx.set_option("comm_overlap", overlap)
                ctxs.append(ctx)
            link = str(tmp_path / ("hostlink_" + tag + name))
            _in_threads([lambda c=c: c.comm_init_host(link) for c in ctxs])
            if prepare:
                _in_threads([lambda c=c: self._init(c) for c in ctxs])
            self.sets.append(ctxs)
        self.a, self.b = self.sets

    @staticmethod
    def _init(c):           # main() and sim::init (driver.SlabSet.prepare) over the communicator
        c.calculate_timestep(c.cfl_allreduce())
        c.exchange()
        c.apply_boundary(0.0, False)
        c.calculate_timestep(c.cfl_allreduce())
        c.exchange()

    def each(self, f, which=None):
        for ctxs in (self.sets if which is None else [which]):
            for c in ctxs:
                f(c)

    def upload(self, case, prm, s, capacity=0, which=None):
        explicit = case.startswith("explicit")

        def setup(c):
            c.particles_slabs(True, capacity)
            if explicit:
                c.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, cartesian=case == "explicit-cartesian")
            if case == "diffusion":
                c.particles_diffusion(gas_drag=True, diffusion=True, seed=SEED)
            c.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
            if explicit:
                c.particles_timestep_init()

        self.each(setup, which)

    def host_loop(self, c, nsteps, snap, particles=True):
        d = self.d
        for _ in range(nsteps):
            clk = c.clock
            dt = c.calculate_timestep(c.cfl_allreduce())
            step_dt = c.snap_to_monitor(dt) if snap else dt
            if particles:
                c.particles_step(step_dt, INDIRECT, d.omega_frame * step_dt)
                c.particles_migrate()
            c.step(step_dt)
            c.exchange()
            c.post(step_dt)
            if snap and abs((clk.n_monitor + 1) * d.monitor_timestep - c.clock.time) < 1e-6 * dt:   # fcpt_run_steps, snap != 0
                now = c.clock
                now.n_monitor = clk.n_monitor + 1
                now.n_snapshot = now.n_monitor // max(d.nmonitor, 1)
                c.clock = now

    def run(self, snap=False):
        """K steps of both loops"""
        _in_threads([lambda c=c: self.host_loop(c, K, snap) for c in self.b])
        self.each(lambda c: c.particles_follow_run_steps(True), self.a)
        done = driver.SlabSet(self.a).run_steps_linked(K, snap=snap, timeout=180.0)
        assert done == [K] * self.nslabs

    def counters(self, ctxs):
        tot = [c.particles_slabs_get() for c in ctxs]
        return {k: sum(getattr(t, k) for t in tot) for k in COUNTERS}, tot

    def assert_gas_and_clock_equal(self):
        for ca, cb in zip(self.a, self.b):
            ka, kb = ca.clock, cb.clock
            assert (ka.time, ka.last_dt, ka.n_hydro_iter, ka.n_monitor, ka.n_snapshot) == \
                   (kb.time, kb.last_dt, kb.n_hydro_iter, kb.n_monitor, kb.n_snapshot)
            sa, sb = ca.state(), cb.state()
            assert set(sa) == set(sb) and ("energy" in sa) == self.adiabatic
            for k in sa:
                assert np.array_equal(sa[k], sb[k]), (ca.desc.rank, k)

    def assert_equal(self, explicit=False):
        """-> (set B's merged particles, its summed counters, its per-slab counters)"""
        count_b = sum(c.particles_count() for c in self.b)        # set B alone: a tripped guard would raise here
        want = driver.SlabSet(self.b).merged_particles(adaptive=explicit)
        assert count_b == want["id"].size
        assert sum(c.particles_count() for c in self.a) == count_b
        got = driver.SlabSet(self.a).merged_particles(adaptive=explicit)
        for k in COMPARED + (B.ADAPTIVE_FIELDS if explicit else ()):
            assert np.array_equal(got[k], want[k]), (k, int(np.count_nonzero(got[k] != want[k])) if got[k].shape == want[k].shape
                                                     else (got[k].shape, want[k].shape))
        self.assert_gas_and_clock_equal()
        for ca, cb in zip(self.a, self.b):
            assert ca.particles_diffusion_get().step == cb.particles_diffusion_get().step
        (tot_a, _), (tot_b, per_b) = self.counters(self.a), self.counters(self.b)
        assert tot_a == tot_b, (tot_a, tot_b)
        return want, tot_b, per_b

    def close(self):
        for ctxs in self.sets:
            _in_threads([lambda c=c: c.comm_barrier() for c in ctxs])
            for c in reversed(ctxs):
                c.comm_destroy()
                c.close()


def _conditions(p, product, s, plants, escapers, want, tot, per, cartesian=False, deferred=False):
    """What set B must have done for the comparison to mean something."""
    d, nslabs = p.d, p.nslabs
    win = sc.slab_windows(product, d, p.radii, nslabs)
    edges = {w[1] for w in win[:-1]}
    # at each interior edge at least one record went outward and one inward
    for k in range(nslabs - 1):
        assert per[k].sent_outer > 0 and per[k + 1].sent_inner > 0, (k, per[k].sent_outer, per[k + 1].sent_inner)
    assert per[0].sent_inner == 0 and per[-1].sent_outer == 0
    assert tot["sent_inner"] + tot["sent_outer"] == tot["received"]
    # apart from the draw's escapers the live count is the drawn one
    slot = {int(i): k for k, i in enumerate(s["id"])}
    live = {slot[int(i)] for i in want["id"]}
    assert set(range(N)) - live <= escapers, sorted(set(range(N)) - live - escapers)
    radius = {slot[int(i)]: (np.hypot(r, phi) if cartesian else r) for i, r, phi in zip(want["id"], want["r"], want["phi"])}
    # every planted crosser of this split is on the far side of its edge (the ones that turn back only have an owner)
    need = 0
    for k, (edge, sign, kind) in plants.items():
        if edge in edges and kind in ("bulk", "twin", "first", "last"):
            need += 1
            assert k in live and sign * (radius[k] - edge) > 0.0, (k, edge, sign, kind, radius.get(k))
    assert need >= 8 * (nslabs - 1) and tot["received"] >= need
    if not deferred:        # every live particle is held by the slab whose window holds it
        assert tot["deferred"] == 0
        for c, (lo, hi) in zip(p.b, win):
            own = c.particles_get()
            dist = np.hypot(own["r"], own["phi"]) if cartesian else own["r"]
            inside = ((dist >= lo) | c.split.is_first) & ((dist < hi) | c.split.is_last)
            assert inside.all(), (c.desc.rank, own["id"][~inside])


CASES = [("polar", False, 3), ("diffusion", False, 3), ("explicit", False, 3), ("explicit-cartesian", False, 3),
         ("polar", True, 3), ("polar", False, 2)]


@pytest.mark.parametrize("case,adiabatic,nslabs", CASES)
def test_loop_gives_the_bits_of_the_host_stepped_slabs(product, tmp_path, monkeypatch, case, adiabatic, nslabs):
    p = Sets(product, tmp_path, monkeypatch, nslabs=nslabs, adiabatic=adiabatic)
    prm, s, plants, escapers = _draw(product, p.d, case, adiabatic)
    p.upload(case, prm, s)
    p.run()
    explicit = case.startswith("explicit")
    want, tot, per = p.assert_equal(explicit)
    print("%s, %d slabs: %d live, %s" % (case, nslabs, want["id"].size, tot))
    assert p.b[0].particles_diffusion_get().step == K
    _conditions(p, product, s, plants, escapers, want, tot, per, cartesian=case == "explicit-cartesian")
    p.close()


def test_snap_to_monitor(product, tmp_path, monkeypatch):
    p = Sets(product, tmp_path, monkeypatch, monitor=MONITOR)
    prm, s, plants, escapers = _draw(product, p.d, "polar", False)
    p.upload("polar", prm, s)
    p.run(snap=True)
    want, tot, per = p.assert_equal()
    clk = p.b[0].clock
    print("snap: n_monitor %d after %d steps, time %.6e" % (clk.n_monitor, K, clk.time))
    assert clk.n_monitor >= 1 and clk.time >= MONITOR       # a step was snapped inside the K steps
    assert p.a[0].particles_diffusion_get().step == K
    _conditions(p, product, s, plants, escapers, want, tot, per)
    p.close()


def test_comm_overlap(product, tmp_path, monkeypatch):
    p = Sets(product, tmp_path, monkeypatch, overlap=1)
    assert all(c.get_option("comm_overlap") == 1 for ctxs in p.sets for c in ctxs)
    prm, s, plants, escapers = _draw(product, p.d, "polar", False)
    p.upload("polar", prm, s)
    p.run()
    want, tot, per = p.assert_equal()
    _conditions(p, product, s, plants, escapers, want, tot, per)
    p.close()


def test_capacity_one_defers_and_gives_the_same_bits(product, tmp_path, monkeypatch):
    """One record per side and step (a message of 1 + 6 doubles inside the loop): twins reach an edge in the same step and
    one of them waits.  The calm draw, see particles_slab_cases.slab_draw.  Who waits is decided by the slots (the lowest
    leaver of a side goes first, kernels/particles.h), not by the order in which wavefronts reach a counter, so the two sets
    queue the same particles and the counters, a turner that leaves its queue unserved included, are equal by derivation."""
    p = Sets(product, tmp_path, monkeypatch)
    prm, s, plants, escapers = _draw(product, p.d, "polar", False, calm=True)
    p.upload("polar", prm, s, capacity=1)
    p.run()
    want, tot, per = p.assert_equal()
    print("capacity 1: %s" % (tot,))
    assert tot["deferred"] > 0
    _conditions(p, product, s, plants, escapers, want, tot, per, deferred=True)
    p.close()


@pytest.mark.parametrize("snap", [False, True])
def test_no_particles_the_collective_is_issued_and_the_counter_counts(product, tmp_path, monkeypatch, snap):
    """Follow, slabs and communicator on, no particles: set B is run_steps without follow.  With snap the counter is
    advanced by fcpt_particles_step, which counts a call without particles too."""
    p = Sets(product, tmp_path, monkeypatch, monitor=MONITOR if snap else None)
    p.each(lambda c: c.particles_slabs(True))
    p.each(lambda c: c.particles_diffusion(gas_drag=True, diffusion=True, seed=SEED, step=40))
    p.each(lambda c: c.particles_follow_run_steps(True), p.a)
    assert driver.SlabSet(p.a).run_steps_linked(K, snap=snap, timeout=180.0) == [K] * 3
    assert driver.SlabSet(p.b).run_steps_linked(K, snap=snap, timeout=180.0) == [K] * 3
    p.assert_gas_and_clock_equal()
    assert (p.a[0].clock.n_monitor >= 1) == snap
    for ca, cb in zip(p.a, p.b):
        assert ca.particles_diffusion_get().step == 40 + K and cb.particles_diffusion_get().step == 40
        assert ca.particles_count() == 0
        t = ca.particles_slabs_get()
        assert (t.sent_inner, t.sent_outer, t.received, t.deferred) == (0, 0, 0, 0)
    p.close()


def _refused(ctxs, match):
    """run_steps on every slab at once (nobody enters a collective alone): each refuses, with the clock untouched"""
    def one(c):
        c0 = c.clock
        for snap in (False, True):
            with pytest.raises(B.FcptError, match=match):
                c.run_steps(K, snap=snap)
        c1 = c.clock
        assert (c1.time, c1.last_dt, c1.n_hydro_iter) == (c0.time, c0.last_dt, c0.n_hydro_iter)
    _in_threads([lambda c=c: one(c) for c in ctxs])


def test_run_steps_linked_wants_one_host_link(product, tmp_path, monkeypatch):
    """Contexts without a communicator, or on different links, are refused before a slab is started."""
    p = Sets(product, tmp_path, monkeypatch, nslabs=2, prepare=False)
    k0 = p.a[0].clock.n_hydro_iter
    with pytest.raises(ValueError, match="share one host-link"):
        driver.SlabSet([p.a[0], p.b[1]]).run_steps_linked(K)
    _in_threads([lambda c=c: c.comm_barrier() for c in p.a])
    for c in reversed(p.a):
        c.comm_destroy()
    with pytest.raises(ValueError, match="share one host-link"):
        driver.SlabSet(p.a).run_steps_linked(K)
    assert p.a[0].clock.n_hydro_iter == k0
    for c in p.a:
        c.close()
    p.sets = [p.b]
    p.close()


def test_refusals(product, tmp_path, monkeypatch):
    p = Sets(product, tmp_path, monkeypatch, nslabs=2, prepare=False)
    ctxs = p.a
    for c in ctxs:
        c.particles_follow_run_steps(True)
    # a communicator, but fcpt_particles_slabs off
    _refused(ctxs, r"multi-slab loop need fcpt_particles_slabs with on = 1 \(this context is slab \d of 2\)")
    # the explicit integrator without step sizes since the last particles_set
    prm, s, _, _ = _draw(product, p.d, "explicit", False)
    for c in ctxs:
        c.particles_slabs(True)
        c.particles_integrator(kind=B.INTEGRATOR_EXPLICIT)
        c.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    _refused(ctxs, "no step sizes since the last fcpt_particles_set")
    p.close()
    # Integrator: Leapfrog
    q = Sets(product, tmp_path, monkeypatch, nslabs=2, prepare=False, leapfrog=True, tag="frog_")
    for c in q.a:
        c.particles_slabs(True)
        c.particles_follow_run_steps(True)
    _refused(q.a, "Leapfrog")
    q.close()
