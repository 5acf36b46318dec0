"""ParticleIntegrator: explicit in numpy: the statement k_particles_step_explicit is compared with.

One call of `step` is, for every live particle, the reference's sequence (src/particles/particles.cpp)
  update_velocities_from_indirect_term (:1314-1343; the Cartesian form :1322-1324 with cartesian=True),
  update_velocities_from_gas_drag (:1428-1504) or _cart (:1345-1418) when drag=True,
  the adaptive Cash-Karp loop of integrate_explicit_adaptive (:1693-2012) with calculate_dust_smoothing (:896-912) and
  calculate_accelerations_from_star_and_planets (:914-952) or _cart (:954-979),
  the escape test of move() (:2019-2031) and rotate (:2369-2397).
`init_timestep` is init_particle_timestep (:248-374).

The loop is a masked per-particle loop: every pass advances the particles that have not reached dt by one substep of
their own size.  All arithmetic runs in `dtype` (float64 or np.longdouble); the state arrays are kept in it.

As written in the reference, not "fixed": old_timestep (:1726) is a reference to particles[i].timestep.  After
`particles[i].timestep = old_timestep / fac` (:1981) it holds the new value already, so a rejection divides the stored
step a second time, by fmin(facc1, fac11 / safe), and fmin(|timestep|, |old_timestep|) after a rejection changes nothing.

Shared with the kernel, beyond the reference: guards 1..8 of calc_tstop leave the particle unchanged; guard 9 is the cap
on accepted + rejected substeps per particle and call; guard 10 is t_stop < 10 dt in the drag kick (check_tstop,
:1303-1309, which the reference tests once at start-up).
"""
from __future__ import annotations

import numpy as np

import tests.particles_ref as R

ADAPTIVE = ("timestep", "facold", "r_ddot", "phi_ddot")
STATE = ("r", "phi", "r_dot", "phi_dot", "stokes") + ADAPTIVE
GUARD_ATTEMPTS, GUARD_STIFF = 9, 10
MAX_ATTEMPTS = 10000

BETA, FAC1, FAC2, SAFE = 0.04, 0.2, 10.0, 0.9
EXPO1 = 0.2 - BETA * 0.75
FACC1, FACC2 = 1.0 / FAC1, 1.0 / FAC2
E1 = 37.0 / 378.0 - 2825.0 / 27648.0
E3 = 250.0 / 621.0 - 18575.0 / 48384.0
E4 = 125.0 / 594.0 - 13525 / 55296.0
E5 = -277.0 / 14336.0
E6 = 512.0 / 1771.0 - 1.0 / 4.0
ATOL, RTOL = 1e-14, 1e-12


def add_adaptive(s, timestep=None, facold=None):
    """The explicit integrator's fields beside those of particles_ref.make_state."""
    n = s["id"].size
    s["timestep"] = np.zeros(n) if timestep is None else np.array(timestep, dtype=np.float64)
    s["facold"] = np.zeros(n) if facold is None else np.array(facold, dtype=np.float64)
    s["r_ddot"], s["phi_ddot"] = np.zeros(n), np.zeros(n)
    s["accepted"], s["rejected"] = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    return s


def _polar_bodies(bodies):
    bx, by, bm = (np.asarray(v, dtype=np.float64) for v in bodies)
    return bx, by, bm, np.sqrt(bx * bx + by * by), np.arctan2(by, bx)


def angle_cart(x, y):
    """t_particle::get_angle with CartesianParticles."""
    phi = np.arctan2(y, x)
    return np.where(phi < 0.0, phi + R.TWO_PI, phi)


def accelerations(prm, bodies, cartesian, q1, q2, v1, v2, eps_sq):
    """d(velocity)/dt from all bodies, star included; the softening stands inside the square root."""
    G = prm["G"]
    bx, by, bm, br, bphi = _polar_bodies(bodies)
    if cartesian:
        a1, a2 = np.zeros_like(q1), np.zeros_like(q1)
        for k in range(bm.size):
            dx, dy = bx[k] - q1, by[k] - q2
            r2 = dx * dx + dy * dy
            r2 = r2 + eps_sq
            r = np.sqrt(r2)
            factor = G * bm[k] / (r * r2)
            a1 = a1 + factor * dx
            a2 = a2 + factor * dy
        return a1, a2
    a1 = q1 * v2 * v2
    a2 = -2.0 * v1 / q1 * v2
    for k in range(bm.size):
        s, c = np.sin(q2 - bphi[k]), np.cos(q2 - bphi[k])
        d = np.sqrt(q1 * q1 + br[k] * br[k] - 2.0 * q1 * br[k] * c + eps_sq)
        factor = G * bm[k] / (d * (d * d))
        a1 = a1 - factor * (q1 - br[k] * c)
        a2 = a2 - factor * br[k] * s / q1
    return a1, a2


def init_timestep(prm, bodies, s, cartesian=False, dtype=np.float64):
    """init_particle_timestep: Hairer's starting step with rsmooth = 0.05; facold = 1e-4.  -> branch per slot:
    'regular', 'dnf' (dnf or dny <= 1e-10) or 'dnf+der12' (der12 <= 1e-15 as well)."""
    m = s["alive"]
    atoli = 1e-12
    q1, q2, v1, v2 = (np.asarray(s[k][m], dtype=dtype) for k in ("r", "phi", "r_dot", "phi_dot"))
    eps_sq = dtype(0.05) * dtype(0.05)
    with np.errstate(all="ignore"):
        k1_v1, k1_v2 = accelerations(prm, bodies, cartesian, q1, q2, v1, v2, eps_sq)
        dnf, dny = np.zeros_like(q1), np.zeros_like(q1)
        for f, y in ((v1, q1), (v2, q2), (k1_v1, v1), (k1_v2, v2)):
            dnf = dnf + (f / atoli) * (f / atoli)
            dny = dny + (y / atoli) * (y / atoli)
        small = (dnf <= 1.0e-10) | (dny <= 1.0e-10)
        h = np.where(small, dtype(1.0e-6), np.sqrt(dny / dnf) * 0.01)
        t_q1, t_q2, t_v1, t_v2 = q1 + h * v1, q2 + h * v2, v1 + h * k1_v1, v2 + h * k1_v2
        k2_v1, k2_v2 = accelerations(prm, bodies, cartesian, t_q1, t_q2, t_v1, t_v2, eps_sq)
        der2 = np.zeros_like(q1)
        for d in (t_v1 - v1, t_v2 - v2, k2_v1 - k1_v1, k2_v2 - k1_v2):
            der2 = der2 + (d / atoli) * (d / atoli)
        der2 = np.sqrt(der2) / h
        der12 = np.fmax(np.abs(der2), np.sqrt(dnf))
        flat = der12 <= 1.0e-15
        h1 = np.where(flat, np.fmax(1.0e-6, np.abs(h) * 1.0e-3), np.power(0.01 / der12, 1.0 / 5.0))
        out = np.fmin(100.0 * h, h1)
    for k in ADAPTIVE:
        s[k] = np.asarray(s[k], dtype=dtype).copy()
    s["timestep"][m] = out
    s["facold"][m] = 1.0e-4
    branch = np.full(m.size, "", dtype=object)
    branch[np.flatnonzero(m)] = np.where(flat, "dnf+der12", np.where(small, "dnf", "regular"))
    return branch


def _count(census, key, n):
    if census is not None and n:
        census[key] = census.get(key, 0) + int(n)


def step(g: R.Grid, fields, prm, bodies, s, dt, indirect=(0.0, 0.0), frame_angle=0.0, *, drag=True, cartesian=False,
         max_attempts=MAX_ATTEMPTS, dtype=np.float64, census=None):
    """Advance the state in place by dt -> guard numbers per slot (0: none; a guarded particle is left as it was)."""
    for k in STATE:
        s[k] = np.array(s[k], dtype=dtype)
    m = s["alive"].copy()
    slots = np.flatnonzero(m)
    q1, q2, v1, v2, stokes, h, facold = (s[k][m].copy() for k in ("r", "phi", "r_dot", "phi_dot", "stokes", "timestep", "facold"))
    size = s["radius"][m]
    guard = np.zeros(slots.size, dtype=np.int64)
    dt = dtype(dt)
    with np.errstate(all="ignore"):
        # ---- update_velocities_from_indirect_term
        if cartesian:
            v1 = indirect[0] * dt + v1
            v2 = indirect[1] * dt + v2
        else:
            c, sn = np.cos(q2), np.sin(q2)
            v1, v2 = (v1 + dt * (indirect[0] * c + indirect[1] * sn),
                      v2 + dt * (-indirect[0] * sn + indirect[1] * c) / q1)
        # ---- update_velocities_from_gas_drag(_cart)
        if drag:
            r = np.sqrt(q1 * q1 + q2 * q2) if cartesian else q1
            phi = angle_cart(q1, q2) if cartesian else q2
            below, above = r < prm["rmin"], r > prm["rmax"]      # RMIN, RMAX (Rinf[0] < RMIN: the ghost ring)
            _count(census, "drag_skipped_below_rmin", below.sum())
            _count(census, "drag_skipped_above_rmax", above.sum())
            _count(census, "drag_on_rmin", (r == prm["rmin"]).sum())
            _count(census, "drag_on_rmax", (r == prm["rmax"]).sum())
            k = np.flatnonzero(~(below | above))
            if k.size:
                rk, pk = r[k], phi[k]
                rho, temp, vg_r, vg_a = R.interpolate(g, fields, rk, pk, prm["omega_frame"])
                if cartesian:
                    c, sn = np.cos(pk), np.sin(pk)
                    rel1 = v1[k] - (c * vg_r - sn * vg_a)
                    rel2 = v2[k] - (sn * vg_r + c * vg_a)
                else:
                    rel1 = v1[k] - vg_r
                    rel2 = rk * v2[k] - vg_a
                vrel = np.sqrt(rel1 * rel1 + rel2 * rel2)
                ts, gd, diag = R.tstop(prm, size[k], rho, vrel, temp)
                gd = np.where((gd == 0) & (ts < 10.0 * dt), GUARD_STIFF, gd)
                _count(census, "guard_stiff", (gd == GUARD_STIFF).sum())
                if census is not None:
                    ok = gd == 0
                    re, kn = np.asarray(diag["Re"], dtype=np.float64)[ok], np.asarray(diag["Kn"], dtype=np.float64)[ok]
                    for name, sel in (("Re<=1e-3", re <= 1e-3), ("Re<=500", (re > 1e-3) & (re <= 500.0)),
                                      ("Re<=1500", (re > 500.0) & (re <= 1500.0)), ("Re>1500", re > 1500.0),
                                      ("Kn>1", kn > 1.0), ("Kn<1", kn < 1.0)):
                        _count(census, name, sel.sum())
                v1[k] = v1[k] + dt * (-rel1 / ts)
                v2[k] = v2[k] + dt * ((-rel2 / ts) if cartesian else (-rel2 / rk / ts))
                stokes[k] = ts * R.omega_kepler(prm, rk)
                guard[k] = gd
        # ---- the adaptive loop
        n = slots.size
        elapsed = np.zeros(n, dtype=dtype)
        last, reject = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        acc, rej = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        a1_out, a2_out = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
        done = guard != 0
        smoothing_factor = np.sqrt(prm["alpha"] / (prm["alpha"] + stokes)) * prm["thickness_smoothing"]
        while not done.all():
            capped = ~done & (acc + rej >= max_attempts)
            guard[capped] = GUARD_ATTEMPTS
            done |= capped
            a = np.flatnonzero(~done)
            if a.size == 0:
                break
            y = [q1[a], q2[a], v1[a], v2[a]]
            ts = h[a].copy()
            clip = elapsed[a] + ts * 1.01 > dt
            ts[clip] = (dt - elapsed[a])[clip]
            is_last = clip.copy()
            update = ~clip
            _count(census, "clipped_last", clip.sum())
            rr = np.sqrt(y[0] * y[0] + y[1] * y[1]) if cartesian else y[0]
            pp = angle_cart(y[0], y[1]) if cartesian else y[1]
            _, _, i_cell, ja, _ = R._cells(g, rr, pp)
            rsmooth = fields["H"][i_cell, ja] * smoothing_factor[a]
            eps_sq = rsmooth * rsmooth

            def f(state):
                d1, d2 = accelerations(prm, bodies, cartesian, state[0], state[1], state[2], state[3], eps_sq)
                return [state[2], state[3], d1, d2]

            k1 = f(y)
            k2 = f([y[j] + ts * 0.2 * k1[j] for j in range(4)])
            k3 = f([y[j] + ts * (0.075 * k1[j] + 0.225 * k2[j]) for j in range(4)])
            k4 = f([y[j] + ts * (0.3 * k1[j] - 0.9 * k2[j] + 1.2 * k3[j]) for j in range(4)])
            k5 = f([y[j] + ts * (-11.0 / 54.0 * k1[j] + 2.5 * k2[j] - 70.0 / 27.0 * k3[j] + 35.0 / 27.0 * k4[j]) for j in range(4)])
            k6 = f([y[j] + ts * (1631.0 / 55296.0 * k1[j] + 175.0 / 512.0 * k2[j] + 575.0 / 13824.0 * k3[j] +
                                 44275.0 / 110592.0 * k4[j] + 253.0 / 4096.0 * k5[j]) for j in range(4)])
            slope = [37.0 / 378.0 * k1[j] + 250.0 / 621.0 * k3[j] + 125.0 / 594.0 * k4[j] + 512.0 / 1771.0 * k6[j] for j in range(4)]
            new = [y[0] + ts * slope[0], y[1] + ts * slope[1], y[2] + ts * slope[2], y[3] + ts * slope[3]]
            if not cartesian:
                new[1] = R.wrap(new[1])
            err = np.zeros_like(ts)
            for j in range(4):
                est = ts * (E1 * k1[j] + E3 * k3[j] + E4 * k4[j] + E5 * k5[j] + E6 * k6[j])
                sq = est / (ATOL + RTOL * np.fmax(np.abs(y[j]), np.abs(new[j])))
                err = err + sq * sq
            err = np.sqrt(err / 4.0)
            fac11 = np.power(err, EXPO1)
            fac = fac11 / np.power(facold[a], BETA)
            fac = np.fmax(FACC2, np.fmin(FACC1, fac / SAFE))
            _count(census, "fac_ge_1_rule", (~update & (fac < 1.0)).sum())
            fac = np.where(update, fac, np.fmax(fac, 1.0))
            hn = h[a] / fac                       # particles[i].timestep = old_timestep / fac; old_timestep IS this value now
            ok = err <= 1.0
            _count(census, "rejection", (~ok).sum())
            _count(census, "accepted_after_rejection", (ok & reject[a]).sum())
            # accepted: after a rejection, fmin(|timestep|, |old_timestep|) of one and the same value
            hn_acc = np.where(reject[a], np.fmin(np.abs(hn), np.abs(hn)), hn)
            # rejected: old_timestep / fmin(facc1, fac11 / safe) -- the second division
            hn_rej = hn / np.fmin(FACC1, fac11 / SAFE)
            h[a] = np.where(ok, hn_acc, hn_rej)
            facold[a] = np.where(ok, np.fmax(err, 1.0e-4), facold[a])
            elapsed[a] = np.where(ok, elapsed[a] + ts, elapsed[a])
            for arr, val in ((q1, new[0]), (q2, new[1]), (v1, new[2]), (v2, new[3]), (a1_out, slope[2]), (a2_out, slope[3])):
                arr[a] = np.where(ok, val, arr[a])
            reject[a] = ~ok
            acc[a] += ok
            rej[a] += ~ok
            done[a] = ok & is_last
        # ---- move(), rotate()
        rsq = q1 * q1 + q2 * q2 if cartesian else q1 * q1
        out_, in_ = rsq > prm["escape_radius_max"] ** 2 - R.DBL_EPSILON, rsq < prm["escape_radius_min"] ** 2 + R.DBL_EPSILON
        if cartesian:
            c, sn = np.cos(dtype(frame_angle)), np.sin(dtype(frame_angle))
            q1, q2 = q1 * c + q2 * sn, -q1 * sn + q2 * c
            v1, v2 = v1 * c + v2 * sn, -v1 * sn + v2 * c
        else:
            q2 = R.wrap(q2 - frame_angle)
    ok = guard == 0
    _count(census, "escape_outward", (ok & out_).sum())
    _count(census, "escape_inward", (ok & in_).sum())
    w = slots[ok]
    for k, v in (("r", q1), ("phi", q2), ("r_dot", v1), ("phi_dot", v2), ("stokes", stokes), ("timestep", h), ("facold", facold),
                 ("r_ddot", a1_out), ("phi_ddot", a2_out)):
        s[k][w] = v[ok]
    s["accepted"][w] = acc[ok]
    s["rejected"][w] = rej[ok]
    s["alive"][w] = ~(out_ | in_)[ok]
    guards = np.zeros(m.size, dtype=np.int64)
    guards[slots] = guard
    return guards


def live(s):
    m = s["alive"]
    return {k: np.asarray(v[m], dtype=np.float64 if v.dtype.kind == "f" else v.dtype).copy() for k, v in s.items() if k != "alive"}


def worst_difference_cartesian(a, b):
    """The parity measure for a Cartesian state: max|a-b| / max|b| over the position pair, the velocity pair and stokes."""
    assert np.array_equal(a["id"], b["id"]), "the sets of live particles differ"
    if a["id"].size == 0:
        return {"position": 0.0, "velocity": 0.0, "stokes": 0.0}
    out = {}
    for name, keys in (("position", ("r", "phi")), ("velocity", ("r_dot", "phi_dot"))):
        d = max(np.abs(a[k] - b[k]).max() for k in keys)
        out[name] = float(d / max(np.abs(b[k]).max() for k in keys))
    out["stokes"] = float(np.abs(a["stokes"] - b["stokes"]).max() / np.abs(b["stokes"]).max())
    return out


def physics(desc, params):
    """particles_ref.physics and RMIN, RMAX, outside which the drag kick is skipped."""
    out = R.physics(desc, params)
    out.update(rmin=desc.rmin, rmax=desc.rmax)
    return out
