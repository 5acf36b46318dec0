"""Particles on 2 and 3 radial slabs against one slab (fcpt_particles_slabs): ownership, migration, guard 11.

Frozen gas: 8 gas steps on one slab, the global grids downloaded once per EOS and uploaded, whole or in row slices (as
tests/util.py cuts slabs), into fresh contexts -- the one-slab context and every slab hold the same gas bits.  Per step
particles_step on every slab, then SlabSet.migrate_particles().  The per-slot state is a function of the inputs alone and
the slab kernels rewrite no floating expression, so the slabs' states merged by slot EQUAL the one-slab arrays bit for
bit (np.array_equal): the derived expectation, not a measurement.  It is asserted after every step, with the set of live
ids, and with exactly one owner per live particle.

Live gas (3 slabs stepping gas and dust) is held to the project's parity bar, max|a-b| / max|b| <= 1e-10 per quantity and
the angle mod 2 pi, as test_gpu_particles_parity.py forms it: the slabs' gas differs from the one-slab gas by rounding."""
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

BAR = 1e-10
GRIDS = (B.F_SIGMA, B.F_SCALE_HEIGHT, B.F_TEMPERATURE, B.F_VRAD, B.F_VAZI)
STATE = (B.F_SIGMA, B.F_VRAD, B.F_VAZI, B.F_ENERGY)
SEED = 20250921
CASES = ("polar", "cartesian", "diffusion", "explicit", "explicit-cartesian")


@functools.lru_cache(maxsize=None)
def _frozen(product, adiabatic):
    """-> (desc, radii, bodies, global (sigma, vrad, vazi, energy) after 8 gas steps, restatement gas of that state)"""
    d = cases.parity_desc(product, 48, 256, adiabatic=adiabatic)
    radii = product.radii(d)
    bodies = setups.jupiter_bodies(d)
    ctx = driver.make_context(product, d, radii=radii, bodies=bodies)
    S = driver.SlabSet([ctx])
    S.prepare()
    S.run(8)
    fields = tuple(ctx.download(f) for f in STATE)
    gas = R.gas_fields(*(ctx.download(f) for f in GRIDS), d.density_factor)
    ctx.close()
    return d, radii, bodies, fields, gas


def _context(product, dk, radii, bodies, fields):
    """A fresh context of slab dk.rank holding the rows of the frozen gas, bit for bit."""
    sub = sc.cut_fields(product, dk, fields)
    ctx = driver.make_context(product, dk, fields=sub, radii=radii, bodies=bodies)
    for f, a in zip(STATE, sub):        # (whatever init_physics did to the grids: the downloaded bits again)
        ctx.upload(f, a)
    return ctx


def _setup(ctx, case, prm, s, slabs, capacity=0):
    explicit = case.startswith("explicit")
    if slabs:
        ctx.particles_slabs(True, capacity)
    if explicit:
        ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, cartesian=case == "explicit-cartesian")
    if case == "diffusion":
        ctx.particles_diffusion(gas_drag=True, diffusion=True, seed=SEED)
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    if explicit:
        ctx.particles_timestep_init()


def _draw(product, case, adiabatic, calm=False):
    """-> (desc, radii, bodies, fields, params, state, plants, dt, steps)"""
    d, radii, bodies, fields, gas = _frozen(product, adiabatic)
    g = R.Grid(radii, d.nr_global, d.nphi)
    prm = cases.parity_params(product, d, case == "cartesian")
    if case.startswith("explicit"):
        s, plants = sc.explicit_slab_state(product, d, radii, g, gas, X.physics(d, prm), case == "explicit-cartesian")
        return d, radii, bodies, fields, prm, s, plants, xc.EXPLICIT_DT, xc.EXPLICIT_CALLS
    s, plants = sc.slab_draw(product, d, radii, calm=calm)
    s["stokes"] = R.initial_stokes(g, gas, R.physics(d, prm), s)
    return d, radii, bodies, fields, prm, s, plants, cases.PARITY_DT, cases.PARITY_STEPS


def _state(ctx_or_set, explicit):
    if isinstance(ctx_or_set, driver.SlabSet):
        return ctx_or_set.merged_particles(adaptive=explicit)
    out = ctx_or_set.particles_get()
    if explicit:
        out.update(ctx_or_set.particles_adaptive_get())
    return out


COMPARED = ("id",) + R.FIELDS
ADAPTIVE = B.ADAPTIVE_FIELDS      # (the substep counters stay with the slab that took the step)


def _assert_equal_bits(got, want, explicit, where):
    for k in COMPARED + (ADAPTIVE if explicit else ()):
        assert np.array_equal(got[k], want[k]), (where, k, int(np.count_nonzero(got[k] != want[k])) if got[k].shape == want[k].shape
                                                 else (got[k].shape, want[k].shape))


def _run(product, case, adiabatic, nslabs, capacity=0, calm=False):
    """-> (final one-slab state, final merged state, summed counters, plants)"""
    d, radii, bodies, fields, prm, s, plants, dt, steps = _draw(product, case, adiabatic, calm)
    explicit = case.startswith("explicit")
    one = _context(product, d, radii, bodies, fields)
    _setup(one, case, prm, s, slabs=False)
    ctxs = [_context(product, dk, radii, bodies, fields) for dk in sc.slab_descs(d, nslabs)]
    for c in ctxs:
        _setup(c, case, prm, s, slabs=True, capacity=capacity)
    S = driver.SlabSet(ctxs)
    n = s["id"].size
    assert sum(c.particles_count() for c in ctxs) == n == one.particles_count()       # every particle has one owner
    # a particle exactly on an edge belongs to the outer slab and stays there: nothing moves before the first step
    _assert_equal_bits(_state(S, explicit), _state(one, explicit), explicit, "start")
    S.migrate_particles()
    assert sum(c.particles_slabs_get().sent_inner + c.particles_slabs_get().sent_outer for c in ctxs) == 0
    win = sc.slab_windows(product, d, radii, nslabs)
    for k, (edge, _, kind) in plants.items():
        if kind == "on":
            owners = [int(s["id"][k]) in c.particles_get()["id"] for c in ctxs]
            assert owners == [lo <= edge < hi for lo, hi in win], (k, edge, owners)
    angle = d.omega_frame * dt
    for step in range(steps):
        one.particles_step(dt, cases.PARITY_INDIRECT, angle)
        for c in ctxs:
            c.particles_step(dt, cases.PARITY_INDIRECT, angle)
        S.migrate_particles()
        want = _state(one, explicit)
        per_slab = [c.particles_get()["id"] for c in ctxs]
        ids = np.concatenate(per_slab)
        assert np.unique(ids).size == ids.size, "a live particle has two owners"
        assert sum(c.particles_count() for c in ctxs) == want["id"].size
        _assert_equal_bits(_state(S, explicit), want, explicit, "step %d" % step)
    tot = [c.particles_slabs_get() for c in ctxs]
    counters = {k: sum(getattr(t, k) for t in tot) for k in ("sent_inner", "sent_outer", "received", "deferred")}
    assert tot[0].sent_inner == 0 and tot[-1].sent_outer == 0
    out = _state(one, explicit), _state(S, explicit), counters, plants
    one.close()
    for c in ctxs:
        c.close()
    return out


def _crossers(plants, nslabs, product, adiabatic, back=True):
    """Changes of owner the planted particles of an nslabs run must make (those at an edge of that split; the ones that
    turn back cross twice, unless random kicks of their excursion's size are on)."""
    d, radii = _frozen(product, adiabatic)[:2]
    edges = {w[1] for w in sc.slab_windows(product, d, radii, nslabs)[:-1]}
    return sum((1 if kind != "back" else 2 * back) for edge, _, kind in plants.values() if edge in edges and kind != "on")


@pytest.mark.parametrize("nslabs", sc.SLAB_COUNTS)
@pytest.mark.parametrize("adiabatic", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_slabs_carry_the_bits_of_one_slab(product, case, adiabatic, nslabs):
    want, got, counters, plants = _run(product, case, adiabatic, nslabs)
    assert want["id"].size < 1000, "nobody left the domain"
    sent = counters["sent_inner"] + counters["sent_outer"]
    need = _crossers(plants, nslabs, product, adiabatic, back=case != "diffusion")
    print("%s, %d slabs: %d records sent (%d planted crossings), %d deferred, %d live" %
          (case, nslabs, sent, need, counters["deferred"], want["id"].size))
    assert sent == counters["received"] and counters["deferred"] == 0
    assert sent >= need > 0


@pytest.mark.parametrize("case", ["polar", "explicit"])
def test_capacity_one_defers_and_gives_the_same_bits(product, case):
    """One record per side and call: the twins of the planted crossers reach an edge in the same step, so one of them
    waits for the next call.  The merged bits are those of one slab after every step, and those of the built-in capacity at
    the end.  (The midpoint draw without the census' enterers, see slab_draw: deferred twice they trip guard 11, by design.)"""
    explicit = case == "explicit"
    want, got, counters, _ = _run(product, case, False, 3, capacity=1, calm=True)
    print("%s, capacity 1: %d deferred, %d records sent" % (case, counters["deferred"], counters["received"]))
    assert counters["deferred"] > 0
    assert counters["sent_inner"] + counters["sent_outer"] == counters["received"]
    free = _run(product, case, False, 3, calm=True)[1]
    _assert_equal_bits(got, free, explicit, "capacity 1 against the built-in capacity")


def test_guard_11_reports_the_particle_that_outruns_the_overlap(product):
    """One particle just inside the edge of a 2-slab split, aimed outward at 12 ring widths per step: its half drift ends
    six rings beyond the edge, past the last row whose gas the slab holds.  Slab 0 reports it and leaves it unchanged; on
    one slab the same particle trips nothing."""
    d, radii, bodies, fields, gas = _frozen(product, False)
    g = R.Grid(radii, d.nr_global, d.nphi)
    prm = cases.parity_params(product, d, False)
    dt = cases.PARITY_DT
    (_, edge), _ = sc.slab_windows(product, d, radii, 2)
    row = int(np.flatnonzero(g.rinf == edge)[0])
    s = cases.census_draw(d, radii, n=65)
    k = 40
    s["r"][k], s["phi"][k] = edge * (1.0 - 1e-6), np.pi
    s["r_dot"][k] = (g.rinf[row + B.OVERLAP - 1] - s["r"][k]) / (0.5 * dt)
    s["phi_dot"][k] = np.sqrt(d.G * d.hydro_center_mass / s["r"][k] ** 3)
    s["radius"][k] = sc.PLANT_RADIUS
    assert s["r_dot"][k] * dt > B.OVERLAP * (g.rinf[row + 1] - g.rinf[row])
    s["stokes"] = R.initial_stokes(g, gas, R.physics(d, prm), s)
    pid = int(s["id"][k])

    one = _context(product, d, radii, bodies, fields)
    _setup(one, "polar", prm, s, slabs=False)
    one.particles_step(dt, cases.PARITY_INDIRECT, d.omega_frame * dt)
    after = one.particles_get()         # no guard
    assert pid in after["id"] and after["r"][after["id"] == pid][0] > g.rinf[row + B.OVERLAP]
    one.close()

    ctxs = [_context(product, dk, radii, bodies, fields) for dk in sc.slab_descs(d, 2)]
    for c in ctxs:
        _setup(c, "polar", prm, s, slabs=True)
    before = ctxs[0].particles_get()
    assert pid in before["id"] and pid not in ctxs[1].particles_get()["id"]
    ctxs[0].particles_step(dt, cases.PARITY_INDIRECT, d.omega_frame * dt)
    with pytest.raises(B.FcptError, match=r"particle id %d tripped guard 11" % pid):
        ctxs[0].particles_count()
    got = ctxs[0].particles_get()       # reported once; the call works again
    m, m0 = got["id"] == pid, before["id"] == pid
    for q in R.FIELDS:
        assert got[q][m][0] == before[q][m0][0], q      # untouched, bit for bit
    assert not np.array_equal(got["r"][~m], before["r"][~m0])       # the rest was stepped
    ctxs[0].particles_step(dt, cases.PARITY_INDIRECT, d.omega_frame * dt)
    with pytest.raises(B.FcptError, match="guard 11"):
        ctxs[0].particles_get()
    assert ctxs[0].particles_count() >= 1
    for c in ctxs:
        c.close()


def _fixed_step(S, dt):
    for c in S.ctxs:
        c.step(dt)
    S.exchange_local()
    for c in S.ctxs:
        c.post(dt)


def test_live_gas_on_three_slabs_meets_the_parity_bar(product):
    d = cases.parity_desc(product, 48, 256)
    radii = product.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    bodies = setups.jupiter_bodies(d)
    prm = cases.parity_params(product, d, False)
    fields = product.initial_fields(d.copy(), radii)
    sets = []
    for ns in (1, 3):
        ctxs = [driver.make_context(product, dk, fields=sc.cut_fields(product, dk, fields), radii=radii, bodies=bodies)
                for dk in sc.slab_descs(d, ns)]
        S = driver.SlabSet(ctxs)
        S.prepare()
        S.run(8)
        sets.append(S)
    one = sets[0].ctxs[0]
    gas = R.gas_fields(*(one.download(f) for f in GRIDS), d.density_factor)
    s, _ = sc.slab_draw(product, d, radii)
    s["stokes"] = R.initial_stokes(g, gas, R.physics(d, prm), s)
    _setup(one, "polar", prm, s, slabs=False)
    for c in sets[1].ctxs:
        _setup(c, "polar", prm, s, slabs=True)
    dt, worst = cases.PARITY_DT, 0.0
    for _ in range(cases.PARITY_STEPS):
        for S in sets:
            for c in S.ctxs:
                c.particles_step(dt, cases.PARITY_INDIRECT, d.omega_frame * dt)
            S.migrate_particles()
            _fixed_step(S, dt)
        got, want = sets[1].merged_particles(), one.particles_get()
        assert np.array_equal(got["id"], want["id"]), "the sets of live particles differ"
        diff = R.worst_difference(got, want)
        worst = max(worst, max(diff.values()))
        assert max(diff.values()) <= BAR, diff
    sent = sum(c.particles_slabs_get().sent_inner + c.particles_slabs_get().sent_outer for c in sets[1].ctxs)
    print("live gas, 3 slabs against 1: worst ratio to the bar %.3e, %d records sent" % (worst / BAR, sent))
    assert sent > 0
    for S in sets:
        for c in S.ctxs:
            c.close()


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


def test_collective_gives_the_bits_of_pack_and_unpack(product, tmp_path):
    """Three contexts on the host link, one thread each: particles_migrate() in place of the hand-over by the caller."""
    d, radii, bodies, fields, prm, s, plants, dt, steps = _draw(product, "polar", False)
    ctxs = [_context(product, dk, radii, bodies, fields) for dk in sc.slab_descs(d, 3)]
    for c in ctxs:
        _setup(c, "polar", prm, s, slabs=True)
    with pytest.raises(B.FcptError, match="fcpt_comm_init"):
        ctxs[0].particles_migrate()                 # no communicator yet
    link = str(tmp_path / "hostlink")
    _in_threads([lambda c=c: c.comm_init_host(link) for c in ctxs])
    angle = d.omega_frame * dt

    def run(c):
        for _ in range(steps):
            c.particles_step(dt, cases.PARITY_INDIRECT, angle)
            c.particles_migrate()
        return c.particles_get()

    parts = _in_threads([lambda c=c: run(c) for c in ctxs])
    got = driver.merge_particles(parts)
    want = _run(product, "polar", False, 3)[1]
    _assert_equal_bits(got, want, False, "collective against pack / unpack")
    _in_threads([lambda c=c: c.comm_barrier() for c in ctxs])
    for c in reversed(ctxs):
        c.comm_destroy()
        c.close()


def test_refusals(product):
    d, radii, bodies, fields, prm, s, plants, dt, steps = _draw(product, "polar", False)
    dk = sc.slab_descs(d, 2)[0]
    ctx = _context(product, dk, radii, bodies, fields)
    with pytest.raises(B.FcptError, match=r"particles need the whole grid in one slab \(this context is slab 0 of 2\)"):
        ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))          # on = 0: today's refusal and its text
    with pytest.raises(B.FcptError, match="needs fcpt_particles_slabs"):
        ctx.particles_migrate_pack(None, None)
    fit = (ctx.particles_migrate_count() - 1) // 6
    assert ctx.particles_migrate_count() == ctx.exchange_count()
    with pytest.raises(B.FcptError, match="migrate_capacity"):
        ctx.particles_slabs(True, fit + 1)
    ctx.particles_slabs(True, fit)
    p = ctx.particles_slabs_get()
    assert (p.on, p.migrate_capacity, p.sent_inner, p.sent_outer, p.received, p.deferred) == (1, fit, 0, 0, 0, 0)
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    assert 0 < ctx.particles_count() < s["id"].size
    # a corrupt message writes nothing and is reported: a count beyond the capacity, a slot index beyond the slots
    cnt = ctx.particles_migrate_count()
    before = ctx.particles_get()
    for word0, slot in ((fit + 1.0, 0.0), (1.0, float(s["id"].size)), (1.0, -1.0), (1.0, 0.5), (np.nan, 0.0)):
        msg = np.zeros(cnt)
        msg[0], msg[1] = word0, slot
        ctx.particles_migrate_unpack(None, msg)
        with pytest.raises(B.FcptError, match="guard 12"):
            ctx.particles_count()
        after = ctx.particles_get()
        for q in before:
            assert np.array_equal(before[q], after[q]), q
    # particles inside fcpt_run_steps on a slab: refused with the clock untouched
    ctx.particles_follow_run_steps(True)
    clock = ctx.clock
    with pytest.raises(B.FcptError, match="multi-slab"):
        ctx.run_steps(4)
    now = ctx.clock
    assert (now.time, now.n_hydro_iter) == (clock.time, clock.n_hydro_iter)
    ctx.close()
