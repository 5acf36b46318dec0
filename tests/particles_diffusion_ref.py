"""Dust diffusion in numpy: the statement the HIP kernel's drag-off path and Brownian kick are compared with.

Restated from the reference's lines (src/particles/), on top of tests/particles_ref.py:
  integrate_exponential_midpoint with particle_gas_drag_enabled false (particles.cpp:1616-1656): tstop = 1e100, the
    propagator formed from it as written, no drag terms;
  check_tstop (particles.cpp:1277-1311), which particles::integrate calls before the kick when the drag is off (:1548-1551);
  diffuse_dust and kick_length (dust_diffusion.cpp:29-97) with compute_gas_diffusion_coefficient (:102-119) and
    compute_gas_density_radial_derivative (:135-149), then move() on the kicked radius.
The reference's host generator is replaced by a counter-based one, so that a deviate depends on (seed, id, step) alone:
Philox4x32-10 (Salmon et al. 2011) in uint64 arithmetic, counter = (id low, id high, step low, step high),
key = (seed low, seed high), u = ((w_a << 20 | w_b >> 12) + 0.5) 2^-52, snv = sqrt(-2 log u1) cos(2 pi u2).

The gas fields are those of particles_ref.gas_fields plus "cs", the sound speed grid (SOUNDSPEED of the reference).
rho, d rho / dr and D_g are evaluated from the fields given to each step (the kernel's stated departure: the reference
keeps the values of init unless Disk: yes).
"""
from __future__ import annotations

import numpy as np

import tests.particles_ref as R

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32(counter, key):
    """counter: four arrays (or scalars) of 32-bit words, key: two -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(v, dtype=np.uint64) for v in counter))
    k0, k1 = (np.asarray(v, dtype=np.uint64) for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2          # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def uniforms(seed, ids, step):
    seed, ids, step = (np.asarray(v, dtype=np.uint64) for v in (seed, ids, step))
    w = philox4x32((ids & MASK, ids >> S32, step & MASK, step >> S32), (seed & MASK, seed >> S32))
    unit = lambda hi, lo: (((hi << np.uint64(20)) | (lo >> np.uint64(12))).astype(np.float64) + 0.5) * 2.0 ** -52
    return unit(w[0], w[1]), unit(w[2], w[3])


def std_normal(seed, ids, step):
    u1, u2 = uniforms(seed, ids, step)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def schmidt(st):
    """compute_Schmidt_number (Youdin & Lithwick 2007, eq. 37)"""
    return (1.0 + st * st) ** 2 / (1.0 + 4.0 * st * st)


def kick_cells(g: R.Grid, r, phi):
    """get_rinf_id (clamped as the release build does) and get_inf_azimuthal_id"""
    i = np.clip(np.searchsorted(g.rinf, r, side="right") - 1, 0, g.nr - 1)
    j = np.clip(np.floor(phi / g.dphi).astype(np.int64), 0, g.nphi - 1)
    return i, j


def kick(g: R.Grid, fields, prm, r, phi, stokes, dt, snv):
    """kick_length -> (delta r, {mean, sigma, row, column})"""
    i, j = kick_cells(g, r, phi)
    if "rho" not in fields:      # formed once per set of grids, as in particles_ref.interpolate
        fields["rho"] = fields["sigma"] / (fields["density_factor"] * fields["H"])
    rho_grid = fields["rho"]
    dg = prm["alpha"] * fields["cs"][i, j] * fields["H"][i, j]
    dd = dg / schmidt(stokes)
    rho = rho_grid[i, j]
    inner = (i >= 1) & (i <= g.nr - 2)          # the derivative's loop leaves rows 0 and Nr-1 at zero
    ip, im = np.where(inner, i + 1, i), np.where(inner, i - 1, i)
    with np.errstate(all="ignore"):
        drho = np.where(inner, (rho_grid[ip, j] - rho_grid[im, j]) / np.where(inner, g.rmed[ip] - g.rmed[im], 1.0), 0.0)
        mean = dd / rho * drho * dt * dt * R.omega_kepler(prm, r)
        sigma = np.sqrt(2.0 * dd * dt)
        corr_2d = r * (np.sqrt(1.0 + (sigma * snv / r) ** 2) - 1.0)
    return mean + snv * sigma + corr_2d, {"mean": mean, "sigma": sigma, "row": i, "column": j}


def _midpoint_without_drag(g, fields, prm, bodies, s, m, dt, indirect):
    """integrate_exponential_midpoint with the drag off, for the slots m -> r3, phi3, r_dot2, phi_dot3, tstop"""
    r0, phi0, stokes_old = (s[k][m] for k in ("r", "phi", "stokes"))
    c, sn = np.cos(phi0), np.sin(phi0)
    r_dot0 = s["r_dot"][m] + dt * (indirect[0] * c + indirect[1] * sn)
    phi_dot0 = s["phi_dot"][m] + dt * (-indirect[0] * sn + indirect[1] * c) / r0
    l0 = r0 * r0 * phi_dot0
    half = 0.5 * dt
    r1 = r0 + r_dot0 * half
    phi1 = R.wrap(phi0 + 0.5 * (l0 / (r0 * r0) + l0 / (r1 * r1)) * half)
    ts = 1e100
    r_in = np.minimum(np.maximum(r1, g.rinf[0]), g.rinf[g.nr])
    _, _, i_cell, ja, _ = R._cells(g, r_in, phi1)
    with np.errstate(all="ignore"):
        h_dust = fields["H"][i_cell, ja] * np.sqrt(prm["alpha"] / (prm["alpha"] + stokes_old))
        eps_sq = (h_dust * prm["thickness_smoothing"]) ** 2
        a_r, minus_l_dot = R._gravity(prm, bodies, r1, phi1, eps_sq)
        decay = np.exp(-dt / ts)
        h1 = ts * (-np.expm1(-dt / ts))
        l2 = decay * l0 + h1 * minus_l_dot
        r_dot2 = decay * r_dot0
        r_dot2 = r_dot2 + h1 * 0.5 * (l0 * l0 + l2 * l2) / (r1 * r1 * r1)
        r_dot2 = r_dot2 + h1 * a_r
        r3 = r1 + r_dot2 * half
        phi3 = R.wrap(phi1 + 0.5 * (l2 / (r1 * r1) + l2 / (r3 * r3)) * half)
    return r3, phi3, r_dot2, l2 / (r3 * r3), ts


def step(g: R.Grid, fields, prm, bodies, s, dt, indirect=(0.0, 0.0), frame_angle=0.0, *, gas_drag=True, diffusion=False,
         seed=0, step_no=0):
    """particles::integrate for one step, in place -> (guard numbers per slot, diagnostics of the kicked particles).
    With the defaults it is particles_ref.step."""
    if gas_drag and not diffusion:
        return R.step(g, fields, prm, bodies, s, dt, indirect, frame_angle)
    m = s["alive"].copy()
    slots_all = np.flatnonzero(m)
    if gas_drag:
        # the drag step without move() and rotate(): nobody escapes, the frame does not turn
        open_prm = dict(prm, escape_radius_min=0.0, escape_radius_max=np.inf)
        t = R.copy_state(s)
        guard, _ = R.step(g, fields, open_prm, bodies, t, dt, indirect, 0.0)
        guard = guard[slots_all]
        assert t["alive"][slots_all].all()
        r3, phi3, r_dot2, phi_dot3, stokes = (t[k][slots_all] for k in ("r", "phi", "r_dot", "phi_dot", "stokes"))
    else:
        r3, phi3, r_dot2, phi_dot3, ts = _midpoint_without_drag(g, fields, prm, bodies, s, m, dt, indirect)
        guard = np.zeros(slots_all.size, dtype=np.int64)
        if diffusion:   # check_tstop at the end position
            rho, temp, vr, va = R.interpolate(g, fields, np.clip(r3, g.rinf[0], g.rinf[g.nr]), phi3, prm["omega_frame"])
            vrel = np.sqrt((vr - r_dot2) ** 2 + (va - phi_dot3 * r3) ** 2)
            ts, guard, _ = R.tstop(prm, s["radius"][m], rho, vrel, temp)
        stokes = ts * R.omega_kepler(prm, r3)
    diag = {}
    r4, phi_dot4 = r3, phi_dot3
    if diffusion:
        snv = std_normal(seed, s["id"][m], step_no)
        delta, diag = kick(g, fields, prm, r3, phi3, stokes, dt, snv)
        diag.update(snv=snv, stokes=stokes, r_before=r3, delta=delta)
        with np.errstate(all="ignore"):
            r4 = r3 + delta
            phi_dot4 = phi_dot3 * (r3 / r4) ** 1.5
    with np.errstate(all="ignore"):
        gone = ((r4 * r4 > prm["escape_radius_max"] ** 2 - R.DBL_EPSILON) | (r4 * r4 < prm["escape_radius_min"] ** 2 + R.DBL_EPSILON)
                | ~(r4 > 0.0))
        gone_before = (r3 * r3 > prm["escape_radius_max"] ** 2 - R.DBL_EPSILON) | (r3 * r3 < prm["escape_radius_min"] ** 2 + R.DBL_EPSILON)
    diag["gone"], diag["gone_before_kick"] = gone, gone_before
    phi4 = R.wrap(phi3 - frame_angle)
    ok = guard == 0
    slots = slots_all[ok]
    for k, v in (("r", r4), ("phi", phi4), ("r_dot", r_dot2), ("phi_dot", phi_dot4), ("stokes", stokes)):
        s[k][slots] = v[ok]
    s["alive"][slots] = ~gone[ok]
    guards = np.zeros(m.size, dtype=np.int64)
    guards[slots_all] = guard
    return guards, diag


def sound_speed(d, fields):
    """SOUNDSPEED from T: c_s^2 = R T / mu (locally isothermal), gamma R T / mu (ideal)"""
    from fargocpt_amd import binding as B
    gamma = d.adiabatic_index if d.eos != B.EOS_ISOTHERMAL else 1.0
    return np.sqrt(gamma * d.Rgas / d.mu * fields["T"])
