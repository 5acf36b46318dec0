"""Inputs shared by the tests of particles on several slabs: the draws of the parity tests with particles planted at every
interior edge of the 2-slab and the 3-slab split of the grid, and the helpers that cut one global state into slabs."""
from __future__ import annotations

import numpy as np

from fargocpt_amd import binding as B

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X

SLAB_COUNTS = (2, 3)
PLANT_RADIUS = cases.CM * 10.0 ** 3.5      # 30 m: keeps its speed over the run, and t_stop >= 10 dt for the explicit kick
# slots of the draws that belong to none of their special classes (k % 10 in {3, 7}, k % 50 in {1, 2}, k % 100 in 11 .. 16)
PLANT_RESIDUES = (20, 24, 25, 26, 28, 29, 30, 34, 35, 36, 38, 39, 40, 44, 45, 46, 48, 49)


def slab_windows(lib: B.Library, d: B.Desc, radii, nslabs):
    """[(r_lo, r_hi)] of the slabs of an nslabs split of the grid of `d`."""
    out = []
    for rank in range(nslabs):
        dk = d.copy()
        dk.rank, dk.nranks = rank, nslabs
        out.append(lib.particles_slab_window(dk, radii))
    return out


def interior_edges(lib: B.Library, d: B.Desc, radii, counts=SLAB_COUNTS):
    """The shared edges of the splits into `counts` slabs, ascending, each once."""
    edges = set()
    for ns in counts:
        edges.update(w[1] for w in slab_windows(lib, d, radii, ns)[:-1])
    return sorted(edges)


def plant_crossers(s, d: B.Desc, radii, edges, dt, steps, seed=7):
    """Overwrites slots of the polar state `s` in place with particles at every edge of `edges`.  Per edge and direction:
    crossers a known number of step lengths inside the edge, moving toward it at a tenth of the Kepler speed (one in a
    column of the bulk, its twin at the same radius in another, one in the first and one in the last half column of the
    ring), and one that turns back: it
    crosses slowly on an orbit whose angular momentum is 10 % off the circular one, so the centrifugal imbalance,
    0.19 G M / r^2, reverses it after a third of the run and it crosses again.  Per edge one particle exactly on the edge
    radius, at phi = pi (opposite the planet: the 2-slab edge lies next to its orbit; in the Cartesian form x = -r and
    y^2 is 1e-32 of x^2, so x^2 + y^2 rounds to r^2).  The seam crossers of an edge within 0.2 of the planet's orbit are
    planted in the bulk instead.  A step covers about 1 % of a ring width, so nobody needs a row beyond the overlap.
    -> {slot: (edge, direction, kind)} with kind in "bulk", "twin", "first", "last", "back", "on"."""
    rng = np.random.default_rng(seed)
    n = s["id"].size
    g = R.Grid(radii, d.nr_global, d.nphi)
    gm = d.G * d.hydro_center_mass
    vk = lambda r: np.sqrt(gm / r)
    free = [k for k in range(n) if k % 100 in PLANT_RESIDUES]
    plants = {}

    def put(r, phi, r_dot, v_phi, what):
        k = free.pop(0)
        s["r"][k], s["phi"][k], s["r_dot"][k], s["phi_dot"][k] = r, phi, r_dot, v_phi / r
        s["radius"][k] = PLANT_RADIUS
        plants[k] = what

    span = steps * dt
    for edge in edges:
        for sign in (1.0, -1.0):        # outward, inward
            v = 0.1 * vk(edge)
            for kind in ("bulk", "first", "last"):
                if abs(edge - 1.0) < 0.2 and kind != "bulk":
                    kind = "bulk"       # the planet sits at (1, 0), on the seam: no fly-by (see census_draw)
                r = edge - sign * v * dt * rng.uniform(0.5, steps - 1.5)
                if kind == "bulk":      # and a twin in another column that crosses in the same step (migrate_capacity = 1)
                    put(r, rng.uniform(0.5, 5.5), sign * v, vk(r), (edge, sign, "twin"))
                phi = {"bulk": rng.uniform(0.5, 5.5), "first": rng.uniform(0.02, 0.45) * g.dphi,
                       "last": 2.0 * np.pi - rng.uniform(0.02, 0.45) * g.dphi}[kind]
                put(r, phi, sign * v, vk(r), (edge, sign, kind))
            # the turning point after span / 3, the edge a sixth of the way to it
            a = 0.19 * gm / (edge * edge)
            u = a * span / 3.0
            reach = u * u / (2.0 * a)
            r = edge - sign * reach / 6.0
            put(r, rng.uniform(0.5, 5.5), sign * u, vk(r) * (0.9 if sign > 0 else 1.1), (edge, sign, "back"))
        put(edge, np.pi, 0.0, vk(edge), (edge, 0.0, "on"))
    return plants


def slab_draw(lib: B.Library, d: B.Desc, radii, n=1000, dt=cases.PARITY_DT, steps=cases.PARITY_STEPS, calm=False):
    """census_draw plus the planted crossers of the 2-slab and 3-slab edges.  -> (state, plants)
    calm: without the census' enterers.  They cross the grid at 3 to 5 ring widths per step, so one of them whose hand-over
    is deferred twice has outrun the overlap (guard 11): with migrate_capacity = 1 that is what a run with them comes to.
    They start one step length inside the grid's edge instead, at a tenth of the Kepler speed."""
    s = cases.census_draw(d, radii, n=n, dt=dt)
    if calm:
        k = np.arange(n)
        for sel, edge, sign in ((k % 100 == 13, d.rmin, 1.0), (k % 100 == 14, d.rmax, -1.0)):
            v = 0.1 * np.sqrt(d.G * d.hydro_center_mass / edge)
            s["r"][sel] = edge + sign * v * dt
            s["r_dot"][sel] = sign * v
            s["phi_dot"][sel] = np.sqrt(d.G * d.hydro_center_mass / s["r"][sel] ** 3)
    plants = plant_crossers(s, d, radii, interior_edges(lib, d, radii), dt, steps)
    return s, plants


def explicit_slab_state(lib: B.Library, d: B.Desc, radii, g, gas, phys, cartesian, n=1000):
    """particles_explicit_cases.parity_state with the planted crossers, for EXPLICIT_CALLS calls of EXPLICIT_DT.
    -> (state with the adaptive fields, plants)"""
    s = xc.explicit_draw(d, radii, n=n)
    plants = plant_crossers(s, d, radii, interior_edges(lib, d, radii), xc.EXPLICIT_DT, xc.EXPLICIT_CALLS)
    m = np.arange(n) % 100 == 16
    _, _, vr, va = R.interpolate(g, gas, s["r"][m], s["phi"][m], phys["omega_frame"])
    s["r_dot"][m] = vr + xc.COMOVING_OFFSET * np.abs(va)
    s["phi_dot"][m] = va * (1.0 + xc.COMOVING_OFFSET) / s["r"][m]
    s["stokes"] = R.initial_stokes(g, gas, phys, s)
    if cartesian:
        s = xc.to_cartesian(s)
    return X.add_adaptive(s), plants


def subset(s, slots):
    """The state of the slots `slots` alone (a small state for the restatement)."""
    slots = np.asarray(sorted(slots))
    return {k: v[slots].copy() for k, v in s.items()}, slots


def crossings(history, edge):
    """How often a series of radii changes the side of `edge` (a radius exactly on it belongs to the outer side)."""
    side = np.asarray(history) >= edge
    return int(np.count_nonzero(side[1:] != side[:-1]))


def slab_descs(d: B.Desc, nslabs):
    out = []
    for rank in range(nslabs):
        dk = d.copy()
        dk.rank, dk.nranks = rank, nslabs
        out.append(dk)
    return out


def cut_fields(lib: B.Library, dk: B.Desc, fields):
    """The rows of slab dk.rank of the global (sigma, vrad, vazi, energy), as tests/util.py cuts them."""
    s = lib.split_domain(dk)
    sl = slice(s.imin, s.imin + s.nr)
    sub = (fields[0][sl], fields[1][s.imin:s.imin + s.nr + 1], fields[2][sl], fields[3][sl])
    return tuple(np.ascontiguousarray(x) for x in sub)
