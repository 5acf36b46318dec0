"""The dust-particle step in numpy, vectorised over particles: the statement the HIP kernel is compared with.

One call of `step` is, for every live particle, the reference's sequence (src/particles/particles.cpp)
  update_velocities_from_indirect_term (:1326-1341, polar form),
  integrate_exponential_midpoint (:1579-1672) with calculate_gas_drag_expmid (:1247-1273), find_nearest (:115-133),
  interpolate_bilinear (:1062-1127), calc_tstop (:1130-1214), calculate_dust_smoothing (:896-912) and the gravity of
  the bodies in polar (:981-1018) or Cartesian (:1020-1060) form,
  the escape test of move() (:2019-2031) and rotate (:2394-2395).
It takes the gas as arrays (Sigma, H, T, v_r, v_phi in the reference's Field layout), so it does not depend on how
anybody forms rho and T.  Cells are found by searching the radius arrays (the interpolant is continuous across cells).

Departure from the reference, shared with the kernel: the lower row of the cell-centred interpolation is clamped to
[0, Nr-2] (beyond Rmed[Nr-1] the reference reads row Nr of a scalar grid, out of bounds) and that of v_r to [0, Nr-1].
A particle whose calc_tstop would die() is left unchanged and its guard number (1 .. 8) is returned.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("r", "phi", "r_dot", "phi_dot", "radius", "stokes")
TWO_PI = 2.0 * np.pi
DBL_EPSILON = float(np.finfo(np.float64).eps)


class Grid:
    """Interface and centre radii of a whole grid (src/init.cpp:169-225) from the interface array of fcpt_radii."""

    def __init__(self, radii, nr: int, nphi: int):
        ri, rs = np.asarray(radii[:nr], dtype=np.float64), np.asarray(radii[1:nr + 1], dtype=np.float64)
        self.nr, self.nphi = nr, nphi
        self.rinf = np.asarray(radii[:nr + 1], dtype=np.float64)           # Rinf[0 .. nr] (Rinf[nr] = Rsup[nr-1])
        self.rmed = 2.0 / 3.0 * (rs * rs * rs - ri * ri * ri) / (rs * rs - ri * ri)
        self.dphi = TWO_PI / nphi


def make_state(ids, r, phi, r_dot, phi_dot, radius, stokes):
    s = {"id": np.array(ids, dtype=np.uint64)}
    for k, v in zip(FIELDS, (r, phi, r_dot, phi_dot, radius, stokes)):
        s[k] = np.array(v, dtype=np.float64)
    s["alive"] = np.ones(s["id"].size, dtype=bool)
    return s


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def live(s):
    """What fcpt_particles_get hands out: the live particles in slot order."""
    m = s["alive"]
    return {k: v[m].copy() for k, v in s.items() if k != "alive"}


def wrap(phi):
    """check_angle (:84-95): one turn at most."""
    return np.where(phi >= TWO_PI, phi - TWO_PI, np.where(phi < 0.0, phi + TWO_PI, phi))


def _cells(g: Grid, r, phi):
    ia = np.clip(np.searchsorted(g.rinf, r, side="right") - 1, 0, g.nr - 1)      # Rinf[ia] <= r
    ib_raw = np.searchsorted(g.rmed, r, side="right") - 1                        # Rmed[ib] <= r, -1 below Rmed[0]
    ib = np.clip(ib_raw, 0, g.nr - 2)
    i_cell = np.clip(ib_raw, 0, g.nr - 1)                                        # get_rmed_id, release build
    ja = np.clip(np.floor(phi / g.dphi).astype(np.int64), 0, g.nphi - 1)    # phi in [0, 2 pi]: 2 pi itself stays in the last column
    jb = np.mod(np.floor((phi - 0.5 * g.dphi) / g.dphi).astype(np.int64), g.nphi)
    return ia, ib, i_cell, ja, jb


def _bilinear(q, im, jm, jp, rm, rp, phim, phip, dphi, r, phi):
    qm = ((phip - phi) * q[im, jm] + (phi - phim) * q[im, jp]) / dphi
    qp = ((phip - phi) * q[im + 1, jm] + (phi - phim) * q[im + 1, jp]) / dphi
    return ((rp - r) * qm + (r - rm) * qp) / (rp - rm)


def interpolate(g: Grid, fields, r, phi, omega_frame):
    """interpolate_quantities (:1216-1244): rho, T, v_r and v_phi + r OmegaFrame at (r, phi); r inside the grid."""
    ia, ib, _, ja, jb = _cells(g, r, phi)
    jap, jbp = (ja + 1) % g.nphi, (jb + 1) % g.nphi
    seam = jb == g.nphi - 1
    low = seam & (phi < np.pi)         # inside column 0: the previous centre lies at -dphi/2
    phim_b = np.where(low, -0.5 * g.dphi, (jb + 0.5) * g.dphi)
    phip_b = np.where(low, 0.5 * g.dphi, np.where(seam, (jb + 1.5) * g.dphi, (jbp + 0.5) * g.dphi))
    phim_a, phip_a = ja * g.dphi, (ja + 1.0) * g.dphi
    if "rho" not in fields:      # formed once per set of grids
        fields["rho"] = fields["sigma"] / (fields["density_factor"] * fields["H"])
    rho_grid = fields["rho"]
    rbm, rbp = g.rmed[ib], g.rmed[ib + 1]
    rho = _bilinear(rho_grid, ib, jb, jbp, rbm, rbp, phim_b, phip_b, g.dphi, r, phi)
    temp = _bilinear(fields["T"], ib, jb, jbp, rbm, rbp, phim_b, phip_b, g.dphi, r, phi)
    vr = _bilinear(fields["vrad"], ia, jb, jbp, g.rinf[ia], g.rinf[ia + 1], phim_b, phip_b, g.dphi, r, phi)
    va = _bilinear(fields["vazi"], ib, ja, jap, rbm, rbp, phim_a, phip_a, g.dphi, r, phi)
    return rho, temp, vr, va + r * omega_frame


def tstop(prm, size, rho, vrel, temperature):
    """calc_tstop (:1130-1214) -> (tstop, guard number or 0, diagnostics {Kn, Ma, Re})."""
    m0, a0 = prm["molecule_mass"], prm["molecule_radius"]
    with np.errstate(all="ignore"):
        vthermal = np.sqrt(8.0 * prm["k_B"] * temperature / (np.pi * m0))
        nu = 1.0 / 3.0 * m0 * vthermal / (np.pi * a0 ** 2)
        mfp = m0 / np.pi / a0 ** 2 / rho
        c_s = vthermal * np.sqrt(np.pi / 8.0)
        kn = 0.5 * mfp / size
        ma = vrel / c_s
        re = 2.0 * size * rho * vrel / nu
        cde = 2.0 * np.sqrt(ma * ma + 128.0 / 9.0 / np.pi)
        cds = np.where(
            re <= 1.0e-3,
            24.0 * nu / (2.0 * size * rho * c_s) + 3.6 / c_s * vrel ** 0.687 * (2.0 * size * rho / nu) ** -0.313,
            np.where(re <= 500.0, 24.0 * ma / re + 3.6 * ma * re ** -0.313,
                     np.where(re <= 1500.0, ma * 9.5e-5 * re ** 1.397, ma * 2.61)))
        cd = (9.0 * kn * kn * cde + cds) / (3.0 * kn + 1.0) / (3.0 * kn + 1.0)
        t = 4.0 * mfp * prm["particle_density"] / (3.0 * rho * cd * c_s * kn)
    guard = np.zeros(np.shape(vrel), dtype=np.int64)
    for number, bad in ((8, cd > 1e20), (7, cd < 1e-20), (6, cds > 1e30), (5, cds < 1e-30), (4, cde > 1e20),
                        (3, cde < 1e-20), (2, ma > 1e20), (1, ma < 1e-20)):   # the first test in source order wins
        guard = np.where(bad, number, guard)
    return t, guard, {"Kn": kn, "Ma": ma, "Re": re}


def _gravity(prm, bodies, r, phi, eps_sq):
    """(d2r/dt2, minus dl/dt) from all bodies, star included."""
    G = prm["G"]
    ar, mdl = np.zeros_like(r), np.zeros_like(r)
    bx, by, bm = (np.asarray(v, dtype=np.float64) for v in bodies)
    if prm["gravity_cartesian"]:
        c, s = np.cos(phi), np.sin(phi)
        x, y = r * c, r * s
        ax, ay = np.zeros_like(r), np.zeros_like(r)
        for k in range(bm.size):
            dx, dy = x - bx[k], y - by[k]
            d2 = dx * dx + dy * dy + eps_sq
            d = np.sqrt(d2)
            ax += -G * bm[k] * dx / (d * d2)
            ay += -G * bm[k] * dy / (d * d2)
        return ax * c + ay * s, (-ax * s + ay * c) * r
    for k in range(bm.size):
        rp, pp = np.hypot(bx[k], by[k]), np.arctan2(by[k], bx[k])
        s, c = np.sin(phi - pp), np.cos(phi - pp)
        d = np.sqrt(r * r + rp * rp - 2.0 * r * rp * c)
        d2s = d * d + eps_sq
        ar -= G * bm[k] * (r - rp * c) / (d2s * d)
        mdl -= G * bm[k] * r * rp * s / (d2s * d)
    return ar, mdl


def omega_kepler(prm, r):
    return np.sqrt(prm["G"] * prm["Mc"] / (r * r * r))


def initial_stokes(g: Grid, fields, prm, s):
    """check_tstop (:1277-1311): the Stokes number of particles at rest in their slots, before the first step."""
    r, phi = s["r"], s["phi"]
    rho, temp, vr, va = interpolate(g, fields, np.clip(r, g.rinf[0], g.rinf[g.nr]), phi, prm["omega_frame"])
    vrel = np.sqrt((vr - s["r_dot"]) ** 2 + (va - s["phi_dot"] * r) ** 2)
    t, guard, _ = tstop(prm, s["radius"], rho, vrel, temp)
    assert not guard.any(), "check_tstop would die()"
    return t * omega_kepler(prm, r)


def step(g: Grid, fields, prm, bodies, s, dt, indirect=(0.0, 0.0), frame_angle=0.0):
    """Advance the state in place by dt; returns (guard numbers per slot, diagnostics of the live particles' drag law)."""
    m = s["alive"].copy()
    r0, phi0, size, stokes_old = (s[k][m] for k in ("r", "phi", "radius", "stokes"))
    # the indirect term's kick
    c, sn = np.cos(phi0), np.sin(phi0)
    r_dot0 = s["r_dot"][m] + dt * (indirect[0] * c + indirect[1] * sn)
    phi_dot0 = s["phi_dot"][m] + dt * (-indirect[0] * sn + indirect[1] * c) / r0
    l0 = r0 * r0 * phi_dot0
    half = 0.5 * dt
    # drift over half a step at constant angular momentum
    r1 = r0 + r_dot0 * half
    phi1 = wrap(phi0 + 0.5 * (l0 / (r0 * r0) + l0 / (r1 * r1)) * half)
    # the gas where the particle is (inside the grid for the interpolation only)
    r_in = np.minimum(np.maximum(r1, g.rinf[0]), g.rinf[g.nr])
    rho, temp, vg_r, vg_a = interpolate(g, fields, r_in, phi1, prm["omega_frame"])
    dv_r = vg_r - r_dot0
    dl = r1 * vg_a - l0
    vrel = np.sqrt(dv_r * dv_r + (vg_a - phi_dot0 * r0) ** 2)
    ts, guard, diag = tstop(prm, size, rho, vrel, temp)
    # smoothing length from the dust scale height of the particle's cell (Dubrulle et al. 1995)
    _, _, i_cell, ja, _ = _cells(g, r_in, phi1)
    with np.errstate(all="ignore"):
        h_dust = fields["H"][i_cell, ja] * np.sqrt(prm["alpha"] / (prm["alpha"] + stokes_old))
        eps_sq = (h_dust * prm["thickness_smoothing"]) ** 2
        a_r, minus_l_dot = _gravity(prm, bodies, r1, phi1, eps_sq)
        # the kick with the exponential propagator
        decay = np.exp(-dt / ts)
        h1 = ts * (-np.expm1(-dt / ts))
        l2 = decay * l0 + h1 * minus_l_dot
        l2 = l2 + h1 * (dl + l0) / ts
        r_dot2 = decay * r_dot0
        r_dot2 = r_dot2 + h1 * 0.5 * (l0 * l0 + l2 * l2) / (r1 * r1 * r1)
        r_dot2 = r_dot2 + h1 * a_r
        r_dot2 = r_dot2 + h1 * (dv_r + r_dot0) / ts
        # the second half of the drift
        r3 = r1 + r_dot2 * half
        phi3 = wrap(phi1 + 0.5 * (l2 / (r1 * r1) + l2 / (r3 * r3)) * half)
        stokes = ts * omega_kepler(prm, r3)
        phi_dot3 = l2 / (r3 * r3)
    gone = (r3 * r3 > prm["escape_radius_max"] ** 2 - DBL_EPSILON) | (r3 * r3 < prm["escape_radius_min"] ** 2 + DBL_EPSILON)
    phi3 = wrap(phi3 - frame_angle)
    ok = guard == 0
    slots = np.flatnonzero(m)[ok]
    for k, v in (("r", r3), ("phi", phi3), ("r_dot", r_dot2), ("phi_dot", phi_dot3), ("stokes", stokes)):
        s[k][slots] = v[ok]
    s["alive"][slots] = ~gone[ok]
    guards = np.zeros(m.size, dtype=np.int64)
    guards[np.flatnonzero(m)] = guard
    diag["r_in"], diag["phi"] = r_in, phi1
    return guards, diag


def gas_fields(sigma, H, T, vrad, vazi, density_factor):
    return {"sigma": sigma, "H": H, "T": T, "vrad": vrad, "vazi": vazi, "density_factor": density_factor}


def physics(desc, params):
    """The scalars `step` reads, from a descriptor and an fcpt_particle_params."""
    out = {k: getattr(params, k) for k in ("particle_density", "molecule_mass", "molecule_radius", "k_B",
                                           "escape_radius_min", "escape_radius_max", "gravity_cartesian")}
    out.update(G=desc.G, Mc=desc.hydro_center_mass, alpha=desc.viscous_alpha, thickness_smoothing=desc.thickness_smoothing,
               omega_frame=desc.omega_frame)
    return out


def worst_difference(a, b):
    """The parity measure over two sets of live particles with the same ids: max|a-b|/max|b| for r, r_dot, r phi_dot and
    stokes, and the largest angle difference mod 2 pi for phi.  -> {quantity: value}."""
    assert np.array_equal(a["id"], b["id"]), "the sets of live particles differ"
    out = {}
    if a["id"].size == 0:
        return {k: 0.0 for k in ("r", "r_dot", "r_phi_dot", "stokes", "phi")}
    for k in ("r", "r_dot", "stokes"):
        out[k] = float(np.abs(a[k] - b[k]).max() / np.abs(b[k]).max())
    va, vb = a["r"] * a["phi_dot"], b["r"] * b["phi_dot"]
    out["r_phi_dot"] = float(np.abs(va - vb).max() / np.abs(vb).max())
    d = np.mod(a["phi"] - b["phi"] + np.pi, TWO_PI) - np.pi
    out["phi"] = float(np.abs(d).max())
    return out
