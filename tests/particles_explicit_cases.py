"""Inputs shared by the tests of the explicit adaptive particle integrator (tests/particles_explicit_ref.py), and the
bars that were measured from the restatement alone."""
from __future__ import annotations

import numpy as np

from fargocpt_amd import binding as B

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_ref as X

# The gas is frozen during the 8 calls.  The step is of the size of a hydro step (the CFL step of the 2048 x 4096 benchmark
# grid is 9.3e-4): the integrator is meant for t_stop >= 10 dt with dt the CFL step.  Every particle then covers a call in
# one clipped substep, or in two during the first calls, while its step size is still the well-conditioned one of
# init_particle_timestep.  That is what makes r_ddot and phi_ddot, the mean acceleration over the LAST accepted substep,
# as well conditioned as the state: where a call is split by a step size that has been through the controller (err^0.17
# of a cancellation), the last substep begins where rounding puts it.  Measured with the restatement alone, float64
# against longdouble, largest difference of r_ddot / phi_ddot over the four isothermal variants:
#   dt = 0.001: 1.9e-14 / 7.3e-16     dt = 0.002: 1.8e-8 / 1.2e-7     dt = 0.004: 7.4e-7 / 2.0e-7
# so only at 0.001 can the parity bar of 1e-10 tell an error from rounding (tests/test_particles_explicit_census.py holds
# the case to a tenth of the bar).  At dt = 0.01 .. 0.05 the two restatements also disagree on the substep counts of
# 0.4 .. 2.4 % of the particles, more than the 0.2 % a case may have; at 0.001 on none.  Rejections and calls of many
# substeps are the subject of the step-size, encounter and Kepler tests.
EXPLICIT_DT = 1.0e-3
EXPLICIT_CALLS = 8

# ---- measured from the restatement on the CPU ("Explicit adaptive integrator") -----------------
# Kepler orbit, e = 0.3, a = 1, 10 orbits in 100 calls: deviation of the position from the solution of Kepler's equation
# (relative to a), of the energy and of the angular momentum (relative to their initial values), polar / Cartesian state
KEPLER_POSITION_MEASURED = {False: 7.1e-10, True: 1.2e-9}
KEPLER_ENERGY_MEASURED = {False: 1.2e-11, True: 1.8e-11}
KEPLER_MOMENTUM_MEASURED = {False: 1.5e-12, True: 2.3e-11}
KEPLER_AGREEMENT_MEASURED = 4.1e-10          # |polar - Cartesian| of the final position
KEPLER_SUBSTEPS_MEASURED = {False: 4842, True: 5031}
KEPLER_BAR_FACTOR = 10.0                     # libm differences between hosts
KEPLER_POSITION_LIMIT = 1e-8                 # rtol x 1e4, whatever was measured
KEPLER_SUBSTEPS_LIMIT = 10000
# timestep and facold are ill-conditioned (err is a cancellation down to 1e-12 of the state): the largest relative
# difference between the restatement in float64 and in longdouble over the parity case, 8 calls, among the
# particles whose substep counts agree.  The device must stay within 10 times these.
# Measured: timestep 2.4e-4 / 2.2e-4 / 3.0e-4 / 1.8e-4 and facold 3.5e-3 / 4.4e-3 / 4.4e-3 / 6.2e-3 for drag off polar,
# drag off Cartesian, drag on polar, drag on Cartesian (isothermal initial gas).
YARDSTICK_TIMESTEP = 3.1e-4
YARDSTICK_FACOLD = 6.2e-3
ACCELERATION_CONDITIONING = 1e-11      # r_ddot, phi_ddot of the two restatements on the parity case: a tenth of the parity bar
YARDSTICK_FACTOR = 10.0
COUNT_MISMATCH_DEVICE = 0.01           # share of particles whose accepted / rejected counts may differ from the restatement's
COUNT_MISMATCH_RESTATEMENTS = 0.002    # ... between the float64 and the longdouble restatement


def kepler_case(lib: B.Library, cartesian: bool, e=0.3, a=1.0):
    """Star only, Stokes number 1e30 so that the softening vanishes, pericentre on the x axis.
    -> (desc, radii, grid, H grid as `fields`, physics, params, bodies, state with adaptive fields)."""
    d = cases.parity_desc(lib, 48, 256, omega_frame=0.0)
    radii = lib.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    prm = lib.particle_params_default(d)
    phys = X.physics(d, prm)
    gm = d.G * d.hydro_center_mass
    rp, vp = a * (1.0 - e), np.sqrt(gm / a * (1.0 + e) / (1.0 - e))
    if cartesian:
        s = R.make_state([7], [rp], [0.0], [0.0], [vp], [1.0], [1e30])
    else:
        s = R.make_state([7], [rp], [0.0], [0.0], [vp / rp], [1.0], [1e30])
    X.add_adaptive(s)
    H = d.aspect_ratio * g.rmed ** (1.0 + d.flaring_index)
    fields = {"H": H[:, None] * np.ones((g.nr, g.nphi))}
    bodies = ([0.0], [0.0], [d.hydro_center_mass])
    return d, radii, g, fields, phys, prm, bodies, s


KEPLER_ORBITS, KEPLER_CALLS = 10, 100


def kepler_truth(t, gm=1.0, e=0.3, a=1.0):
    """Position at time t after pericentre from Kepler's equation (Newton's iteration to rounding)."""
    M = np.sqrt(gm / a ** 3) * t
    E = M
    for _ in range(60):
        E = E - (E - e * np.sin(E) - M) / (1.0 - e * np.cos(E))
    return a * (np.cos(E) - e), a * np.sqrt(1.0 - e * e) * np.sin(E)


def cartesian_of(p, cartesian):
    """(x, y, v_x, v_y) of a state dict in either form."""
    if cartesian:
        return p["r"], p["phi"], p["r_dot"], p["phi_dot"]
    c, s = np.cos(p["phi"]), np.sin(p["phi"])
    return (p["r"] * c, p["r"] * s, p["r_dot"] * c - p["r"] * p["phi_dot"] * s, p["r_dot"] * s + p["r"] * p["phi_dot"] * c)


def kepler_deviations(p, cartesian, t, gm=1.0, e=0.3, a=1.0):
    """-> (position deviation / a, relative energy deviation, relative angular momentum deviation, (x, y))"""
    x, y, vx, vy = (float(v[0]) for v in cartesian_of(p, cartesian))
    xt, yt = kepler_truth(t, gm, e, a)
    en = 0.5 * (vx * vx + vy * vy) - gm / np.hypot(x, y)
    en0, l0 = -0.5 * gm / a, np.sqrt(gm * a * (1.0 - e * e))
    return np.hypot(x - xt, y - yt) / a, abs(en - en0) / abs(en0), abs(x * vy - y * vx - l0) / l0, (x, y)


def to_cartesian(s):
    """The same particles with x, y, v_x, v_y in r, phi, r_dot, phi_dot (CartesianParticles)."""
    out = R.copy_state(s)
    out["r"], out["phi"], out["r_dot"], out["phi_dot"] = cartesian_of(s, False)
    return out


def explicit_draw(d: B.Desc, radii, n=1000, seed=20250307, dt=EXPLICIT_DT, calls=EXPLICIT_CALLS):
    """n weakly coupled bodies (10 m to 1 km, a fifth of them 10 cm to 1 m, the Epstein regime: t_stop >= 10 dt everywhere in
    the planet_disk gas) in polar form: a bulk on
    eccentric orbits, particles in the first and last half column of the ring, leavers that cross either escape
    radius during the run, one particle exactly on RMIN and one on RMAX moving inward of them, and enterers that start
    outside [RMIN, RMAX] (their first drag kick is skipped).  Nobody starts next to the planet at (1, 0)."""
    rng = np.random.default_rng(seed)
    nr, nphi = d.nr_global, d.nphi
    g = R.Grid(radii, nr, nphi)
    vk = lambda r: np.sqrt(d.G * d.hydro_center_mass / r)
    r = np.exp(rng.uniform(np.log(d.rmin * 1.06), np.log(d.rmax * 0.95), n))
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    radius = cases.CM * 10.0 ** rng.uniform(3.0, 5.0, n)
    # (eccentric orbits throughout: where r_dot passes through zero its error scale, atol + rtol |r_dot|, collapses to
    #  atol and the controller's decisions of the polar form become a matter of rounding)
    r_dot = vk(r) * rng.uniform(0.05, 0.3, n) * rng.choice([-1.0, 1.0], n)
    v_phi = vk(r) * (1.0 + rng.normal(0.0, 0.02, n))
    k = np.arange(n)
    if n >= 200:
        # a fifth of the draw are boulders of 10 cm to 1 m: t_stop >= 10 dt still, and the Epstein regime (Kn > 1) with them
        m = (k % 10 == 5) | (k % 10 == 6)
        radius[m] = cases.CM * 10.0 ** rng.uniform(1.0, 2.0, m.sum())
        phi[k % 50 == 1] = rng.uniform(0.02, 0.45, (k % 50 == 1).sum()) * g.dphi
        phi[k % 50 == 2] = 2.0 * np.pi - rng.uniform(0.02, 0.45, (k % 50 == 2).sum()) * g.dphi
        near = (np.abs(r - 1.0) < 0.12) & (np.abs(np.mod(phi + np.pi, 2.0 * np.pi) - np.pi) < 0.15)
        r[near] *= 1.25
        v_phi[near] = vk(r[near])
        for sel, edge, sign in ((k % 100 == 11, d.rmin, -1.0), (k % 100 == 12, d.rmax, 1.0)):      # leavers
            c = sel.sum()
            v = 0.1 * vk(edge)
            r[sel] = edge - sign * v * dt * rng.uniform(0.5, calls - 1.0, c)
            r_dot[sel] = sign * v
            v_phi[sel] = vk(r[sel])
        for sel, edge, sign in ((k % 100 == 13, d.rmin, 1.0), (k % 100 == 14, d.rmax, -1.0)):      # enterers
            c = sel.sum()               # a fraction of one call's path outside: inside the escape radius when the call ends
            v = 0.1 * vk(edge)
            r[sel] = edge - sign * v * dt * rng.uniform(0.1, 0.8, c)
            r_dot[sel] = sign * v
            v_phi[sel] = vk(r[sel])
        for slot, edge, sign in ((15, d.rmin, 1.0), (115, d.rmax, -1.0)):                   # exactly on RMIN, RMAX
            r[slot], phi[slot] = edge, 0.0        # (phi = 0: x = r and y = 0 exactly in the Cartesian form as well)
            r_dot[slot] = sign * 0.05 * vk(edge)
            v_phi[slot] = vk(edge)
    return R.make_state(k + 1000, r, phi, r_dot, v_phi / r, radius, np.zeros(n))


def relative_difference(a, b):
    """max |a - b| / |b| elementwise (the yardstick's measure for timestep and facold)."""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


def kepler_run(advance, cartesian):
    """KEPLER_CALLS calls over KEPLER_ORBITS orbits; advance(dt) -> (live particles, accepted + rejected of the call).
    -> (position, energy, angular momentum deviations, (x, y), substeps in all)"""
    dt = KEPLER_ORBITS * 2.0 * np.pi / KEPLER_CALLS
    total, p = 0, None
    for _ in range(KEPLER_CALLS):
        p, substeps = advance(dt)
        total += int(substeps)
    return kepler_deviations(p, cartesian, KEPLER_CALLS * dt) + (total,)


def restatement_kepler(lib, cartesian, dtype=np.float64):
    d, radii, g, fields, phys, prm, bodies, s = kepler_case(lib, cartesian)
    X.init_timestep(phys, bodies, s, cartesian, dtype)

    def advance(dt):
        guards = X.step(g, fields, phys, bodies, s, dt, drag=False, cartesian=cartesian, dtype=dtype)
        assert not guards.any()
        return X.live(s), s["accepted"][0] + s["rejected"][0]

    return kepler_run(advance, cartesian)


COMOVING_OFFSET = 1.0e-12


def parity_state(lib, d, radii, g, gas, phys, cartesian, n=1000):
    """The draw with check_tstop's Stokes numbers, in the form asked for, with the adaptive fields."""
    s = explicit_draw(d, radii, n=n)
    if n >= 200:
        # ten particles that move with the gas to 1e-12 of its speed: Re <= 1e-3, the first branch of the Stokes
        # coefficient (in their first call; gravity then pulls them off the pressure-supported gas)
        m = np.arange(n) % 100 == 16
        _, _, vr, va = R.interpolate(g, gas, s["r"][m], s["phi"][m], phys["omega_frame"])
        s["r_dot"][m] = vr + COMOVING_OFFSET * np.abs(va)
        s["phi_dot"][m] = va * (1.0 + COMOVING_OFFSET) / s["r"][m]
    s["stokes"] = R.initial_stokes(g, gas, phys, s)
    if cartesian:
        s = to_cartesian(s)
    return X.add_adaptive(s)


STIFF_GRAIN = cases.CM * 0.01    # a grain of 0.1 mm: t_stop < 10 dt anywhere in the planet_disk gas (guard 10)
# dt and calls: the lane takes 73, 35, 24 and 17 substeps in its four calls (its neighbours 2.0 .. 1.0 on average) -- at
# most 100, two orders of magnitude below the attempt cap (at dt = 0.05 its first call took 205)
ENCOUNTER_DT, ENCOUNTER_CALLS, ENCOUNTER_LANE = 0.004, 4, 37
# r_ddot, phi_ddot of calls of many substeps are as ill-conditioned as timestep: the restatement in float64 against itself
# in longdouble, largest max|a-b| / max|b| over the calls of the encounter (2.6e-3, 7.9e-4, 2.2e-2, 6.5e-3) and of the
# step-size sequence (polar 9.8e-4, 3.8e-4, 4.4e-14; Cartesian 1.4e-5, 1.4e-5, 1.4e-15).  The device stays within ten times.
ENCOUNTER_ACCELERATION_YARDSTICK = 2.2e-2
STEP_SIZE_ACCELERATION_YARDSTICK = 1.0e-3


def encounter_wavefront(d: B.Desc, radii):
    """64 particles with the drag off, one wavefront: 63 of the bulk beyond r = 0.9 and, in lane 37, one with Stokes
    number 0.1 (the softening length is 0.6 H sqrt(alpha / (alpha + St)) = 0.003) that starts 0.002 from the planet at
    (1, 0), at rest relative to it, and needs many times the substeps of its neighbours."""
    s = explicit_draw(d, radii, n=64, seed=5)
    s["stokes"][:] = 1.0e3
    inner = s["r"] < 0.9
    s["phi_dot"][inner] *= (s["r"][inner] / (s["r"][inner] + 0.5)) ** 1.5
    s["r"][inner] += 0.5
    k = ENCOUNTER_LANE
    s["r"][k], s["phi"][k], s["r_dot"][k], s["phi_dot"][k], s["stokes"][k] = 1.002, 0.0, 0.0, d.omega_frame, 0.1
    return X.add_adaptive(s)


def restatement_runs(lib, drag, cartesian, census=None):
    """The parity case on the isothermal initial gas, 8 calls, in float64 and in longdouble.
    -> (states, per-call (accepted, rejected) of both runs, largest substep count of a call)"""
    from fargocpt_amd import setups
    d = cases.parity_desc(lib, 48, 256)
    radii = lib.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    sigma, vrad, vazi, _ = lib.initial_fields(d, radii)
    gas = cases.isothermal_gas(d, g, sigma, vrad, vazi)
    bodies = setups.jupiter_bodies(d)
    phys = X.physics(d, cases.parity_params(lib, d, False))
    s0 = parity_state(lib, d, radii, g, gas, phys, cartesian)
    states, counts, most = [], [], 0
    for dtype in (np.float64, np.longdouble):
        s = R.copy_state(s0)
        X.init_timestep(phys, bodies, s, cartesian, dtype)
        hist = []
        for _ in range(EXPLICIT_CALLS):
            live = s["alive"].copy()
            guards = X.step(g, gas, phys, bodies, s, EXPLICIT_DT, cases.PARITY_INDIRECT, d.omega_frame * EXPLICIT_DT, drag=drag,
                            cartesian=cartesian, dtype=dtype, census=census if dtype is np.float64 else None)
            assert not guards.any()
            hist.append((s["accepted"].copy(), s["rejected"].copy()))
            most = max(most, int((s["accepted"] + s["rejected"])[live].max()))
        states.append(s)
        counts.append(hist)
    return states, counts, most


def count_mismatch(hist_a, hist_b):
    """Slots whose accepted or rejected counts differ in any call."""
    m = np.zeros(hist_a[0][0].size, dtype=bool)
    for (aa, ar), (ba, br) in zip(hist_a, hist_b):
        m |= (aa != ba) | (ar != br)
    return m


# the restatement in float64 against itself in longdouble on this sequence: timestep 3.8e-3 (polar) and 6.5e-3 (Cartesian)
# among the particles whose substep counts agree; those of 4 (polar) and 0 (Cartesian) of the 257 do not
STEP_SIZE_YARDSTICK = 6.6e-3
STEP_SIZE_COUNT_MISMATCH = 2.0 * 4.0 / 257.0      # share of the device's particles that may differ in their counts: twice that
STEP_SIZE_CALLS = ((0.05, None), (0.2, 0.15), (EXPLICIT_DT, None))      # (dt, step size planted in every slot before the call)


def step_size_sequence(d, radii, cartesian, init, step, plant=None, after=None):
    """257 bodies with the drag off through three calls: several substeps per particle; a step size planted too large for
    every orbit, which is rejected until it fits; one clipped substep.  init(s), step(s, dt, census) -> guards,
    plant(h, facold) and after(s) are the caller's (restatement, or restatement and device).  -> (state, census)"""
    s = explicit_draw(d, radii, n=257, seed=3)
    s["stokes"][:] = 1.0e3            # (drag off: only the softening reads it)
    s = X.add_adaptive(to_cartesian(s) if cartesian else s)
    init(s)
    census = {}
    for dt, h in STEP_SIZE_CALLS:
        if h is not None:
            s["timestep"] = np.full(257, h)
            if plant:
                plant(s["timestep"].copy(), np.asarray(s["facold"], dtype=np.float64))
        assert not step(s, dt, census).any()
        if after:
            after(s)
    return s, census


def acceleration_gap(a, b):
    """max |a - b| / max |b| of r_ddot and of phi_ddot over the particles that live in both states; the larger of the two"""
    m = a["alive"] & b["alive"]
    out = 0.0
    for k in ("r_ddot", "phi_ddot"):
        x, y = np.asarray(a[k][m], dtype=np.float64), np.asarray(b[k][m], dtype=np.float64)
        out = max(out, float(np.abs(x - y).max() / np.abs(y).max()))
    return out
