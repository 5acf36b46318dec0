"""Planted maxima for the CFL reduction (plain numpy, no GPU).

`condition_cfl` restates cfl.cpp:185-376 in float64 from the reference's formulas: the per-ring <v_phi>, the FARGO
shear limit of ring pair (0, 1) and of the pairs (n, n+1) of the active rings, and for every active cell the six
inverse limits (sound, v_r, residual v_phi, artificial viscosity, viscosity, heating and cooling) and the
StabilizeViscosity: 2 clause.  dt is the minimum of all of it, and a minimum hides everything but the one cell and
term that bind: a state tests a term at a place only if that term binds there.

A *plant* is one small change of a base state (the planet disk with the 1e-3 perturbation of tests/util.perturb)
whose size is found from the base dt and the cell's own widths, so that the limit of the cell meant to bind is
PLANT_TIGHTEN times tighter than the base dt -- wherever the cell lies, also in the wide outer rings that never
bind on their own.  `dead` plants put the same changes where they must not count.

Which cell binds, and through which term (the artificial viscosity multiplies a velocity jump by 4 C^2 ~ 8, so
it outweighs the advection term of the same jump):

  vr+    v_r > 0 at face (i, j): cell i is compressed (v_r(i+1) - v_r(i) < 0): term 4 (and 2) of cell (i, j)
  vr-    v_r < 0 at face (i, j): cell i expands (term 2 alone), cell i-1 is compressed: term 4 of cell (i-1, j)
         binds; where ring i-1 is not active (i = first_active) cell (i, j) binds through term 2
  vphi+  v_phi spike > 0 at (i, j): the jump to column j+1 compresses cell (i, j): term 4 (and 3)
  vphi-  v_phi spike < 0 at (i, j): the jump from column j-1 compresses cell (i, j-1), which reads column j as its
         azimuthal neighbour: term 4 of cell (i, j-1)
  e      ideal EOS, e x factor at (i, j): c_s, term 1 (term 5 with it, smaller for alpha = 1e-3)
  q      ideal EOS, Q+ spike at (i, j): term 6
  cfac   StabilizeViscosity: 2, a negative correction factor at (i, j): -CFL / c
  shear  a uniform v_phi offset of one ring: the pair's shear limit (residuals and jumps do not change)
  nu     (a variant of the descriptor, not a plant of the state: `Case.const_nu`, `const_nu_for`) a constant
         viscosity so large that term 5 binds in the base state
  mean   a v_phi spike in ring 0 or ring active_size: their cells do not count, their means do (shear limit)
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from types import SimpleNamespace

import numpy as np

from fargocpt_amd import binding as B, setups
from tests.util import perturb

PLANT_TIGHTEN = 4.0
CFL_EDGE_LO, CFL_EDGE_HI = B.OVERLAP + 1, B.OVERLAP + 2   # the split launch of kernels/launch.h
TERMS = ("sound", "vr", "vres", "artvisc", "visc", "heat")   # invdt1 .. invdt6
FIELD_IDS = {"sigma": B.F_SIGMA, "vrad": B.F_VRAD, "vazi": B.F_VAZI, "energy": B.F_ENERGY, "qplus": B.F_QPLUS,
             "qminus": B.F_QMINUS, "cfac_phi": B.F_VISC_CFAC_PHI, "cfac_r": B.F_VISC_CFAC_R}

_NP = SimpleNamespace(maximum=np.maximum, minimum=np.minimum, sqrt=np.sqrt, abs=np.abs)
_PY = SimpleNamespace(maximum=max, minimum=min, sqrt=math.sqrt, abs=abs)


# ---------------------------------------------------------------------------------------------------------------
# descriptors, geometry, base states
def case_desc(lib, nr, nphi, ideal=False, leapfrog=False, av="TW", fast=True, stabilize=0, rank=0, nranks=1):
    d = setups.planet_disk(lib, nr * nranks, nphi, adiabatic=ideal)
    d.rank, d.nranks = rank, nranks
    d.integrator = B.INTEGRATOR_LEAPFROG if leapfrog else B.INTEGRATOR_EULER
    d.artificial_viscosity = {"TW": B.ARTVISC_TW, "SN": B.ARTVISC_SN, "None": B.ARTVISC_NONE}[av]
    d.fast_transport = 1 if fast else 0
    d.stabilize_viscosity = stabilize
    return d


def geometry(lib, d, radii, pad=0):
    """The slab's rings as init.cpp:169-225 forms them, and its active range (split.cpp:34-88).  `pad`: that many
    rings beyond the slab's nr in every array (the reference keeps GEOM_PAD of them)."""
    s = lib.split_domain(d)
    nr = s.nr
    ri = np.asarray(radii[s.imin:s.imin + nr + pad], dtype=np.float64)
    rs = np.asarray(radii[s.imin + 1:s.imin + nr + pad + 1], dtype=np.float64)
    rmed = (2.0 / 3.0 * (rs * rs * rs - ri * ri * ri)) / (rs * rs - ri * ri)
    g = SimpleNamespace(nr=nr, nphi=d.nphi, imin=s.imin, first_active=s.radial_first_active,
                        active_size=s.radial_active_size, Rinf=ri, Rsup=rs, Rmed=rmed, InvRmed=1.0 / rmed,
                        InvDiffRsup=1.0 / (rs - ri), dphi=2.0 * math.pi / float(d.nphi),
                        invdphi=float(d.nphi) / (2.0 * math.pi))
    g.is_first, g.is_last = bool(s.is_first), bool(s.is_last)
    g.Surf = math.pi * (rs * rs - ri * ri) / float(d.nphi)
    g.InvSurf = 1.0 / g.Surf
    g.InvRinf = 1.0 / ri
    g.InvDiffRsupRb = 1.0 / ((rs - ri) * rmed)
    g.InvDiffRmed = np.zeros_like(rmed)   # rows 1 .. nr (init.cpp:219-221), 0 elsewhere
    g.InvDiffRmed[1:nr + 1] = (1.0 / (rmed[1:] - rmed[:-1]))[:nr]
    g.dxr = rs - ri
    g.dxa = rmed * g.dphi
    g.cell = np.minimum(g.dxr, g.dxa)
    g.omega_k = np.sqrt(d.G * d.hydro_center_mass / (rmed * rmed * rmed))
    g.cs_iso = (d.aspect_ratio * np.power(rmed, d.flaring_index)) * np.sqrt(d.G * d.hydro_center_mass / rmed)
    return g


def base_state(lib, d):
    """(d0, radii, geometry, state of the slab): initial_fields of the global grid, perturbed, cut to the slab;
    Q+ = Q- = 0 for the ideal EOS; zero correction factors with StabilizeViscosity."""
    dfull = d.copy()
    dfull.rank, dfull.nranks = 0, 1
    radii = lib.radii(dfull)
    fields = perturb(lib.initial_fields(dfull, radii), dfull, 1e-3)   # (dfull.sigma0 possibly rescaled)
    d0 = dfull.copy()
    d0.rank, d0.nranks = d.rank, d.nranks
    g = geometry(lib, d0, radii)
    sl = slice(g.imin, g.imin + g.nr)
    st = {"sigma": fields[0][sl], "vrad": fields[1][g.imin:g.imin + g.nr + 1], "vazi": fields[2][sl],
          "energy": fields[3][sl]}
    if d0.eos == B.EOS_IDEAL:
        st["qplus"] = np.zeros((g.nr, g.nphi))
        st["qminus"] = np.zeros((g.nr, g.nphi))
    if d0.stabilize_viscosity:
        st["cfac_phi"] = np.zeros((g.nr, g.nphi))
        st["cfac_r"] = np.zeros((g.nr, g.nphi))
    return d0, radii, g, {k: np.ascontiguousarray(v, dtype=np.float64).copy() for k, v in st.items()}


# ---------------------------------------------------------------------------------------------------------------
# the restatement
def _lf(d):
    return 0.6 if d.integrator == B.INTEGRATOR_LEAPFROG else 1.0


def _terms(xp, d, g, i, vr0, vr1, va, van, vmean, sigma, energy, qp, qm):
    """The six inverse limits of the cells of ring i (cfl.cpp:243-321); arrays over the ring, or one cell's numbers."""
    lf = _lf(d)
    dxr, dxa, cell = float(g.dxr[i]), float(g.dxa[i]), float(g.cell[i])
    if d.eos == B.EOS_IDEAL:   # compute_sound_speed, compute_scale_height (SourceEuler.cpp:1054-1092, :1218-1251)
        gam = d.adiabatic_index
        cs = xp.sqrt(gam * (gam - 1.0) * energy / sigma)
        H = cs / math.sqrt(gam) * (1.0 / float(g.omega_k[i]))
    else:
        cs = float(g.cs_iso[i]) + 0.0 * va
        H = cs * (1.0 / float(g.omega_k[i]))
    nu = d.viscous_alpha * H * cs if d.viscous_alpha > 0 else d.constant_viscosity + 0.0 * va   # viscosity.cpp:98-137
    invdt1 = cs / cell
    invdt2 = vr0 / dxr
    invdt3 = ((va - vmean) if d.fast_transport else va) / dxa
    C = d.artificial_viscosity_factor
    if d.artificial_viscosity == B.ARTVISC_SN:
        dvr = xp.maximum(-(vr1 - vr0), 0.0 * va)
        dva = xp.maximum(-(van - va), 0.0 * va)
        invdt4 = 4.0 * (C * C) * xp.maximum(dvr / dxr, dva / dxa) * lf
    else:   # TW, and None (cfl.cpp:292)
        eps_rr = (vr1 - vr0) * float(g.InvDiffRsup[i])
        eps_pp = float(g.InvRmed[i]) * ((van - va) * g.invdphi + 0.5 * (vr1 + vr0))
        invdt4 = 4.0 * (C * C) * (-xp.minimum(eps_rr + eps_pp, 0.0 * va)) * lf
    invdt5 = 4.0 * nu / (cell * cell) * lf
    if d.eos == B.EOS_IDEAL:
        invdt6 = (1.0 / d.heating_cooling_cfl_limit) * xp.abs((qp - qm) / energy) * lf
    else:
        invdt6 = 0.0 * va
    return invdt1, invdt2, invdt3, invdt4, invdt5, invdt6


def _dt_of(xp, d, t):
    return d.cfl / xp.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + t[3] * t[3] + t[4] * t[4] + t[5] * t[5])


def ring_mean(vazi_ring):
    """<v_phi> summed in column order, as the reference's loop does (:196-205)."""
    return float(np.add.accumulate(vazi_ring)[-1] / float(vazi_ring.size))


def eval_ring(d, g, st, i, vmean_i):
    """(invdt[6, nphi], dt_cell before the StabilizeViscosity clause, its limit -CFL / c or inf) of ring i."""
    z = np.zeros(g.nphi)
    va = st["vazi"][i]
    t = _terms(_NP, d, g, i, st["vrad"][i], st["vrad"][i + 1], va, np.roll(va, -1), vmean_i, st["sigma"][i],
               st["energy"][i], st.get("qplus", [z] * g.nr)[i], st.get("qminus", [z] * g.nr)[i])
    dt6 = _dt_of(_NP, d, t)
    stab = np.full(g.nphi, np.inf)
    if d.stabilize_viscosity == 2:   # cfl.cpp:331-351
        c = np.minimum(st["cfac_phi"][i], st["cfac_r"][i])
        with np.errstate(divide="ignore"):
            stab = np.where(c != 0.0, -d.cfl / np.where(c != 0.0, c, 1.0), np.inf)
    return np.array(t), dt6, stab


def shear_pairs(g):
    """The ring pairs (n, n+1), by n, whose shear limit counts: (0, 1) (:207-208) and those of the active rings."""
    return [0] + [n for n in range(max(g.first_active, 1), g.active_size)]


def _shear_dt(d, g, vmean, n):
    return d.cfl * g.dphi / (abs(vmean[n] * g.InvRmed[n] - vmean[n + 1] * g.InvRmed[n + 1]) + 1.0e-100)


@dataclass
class Result:
    dt: float
    dt_cell: np.ndarray    # [nr, nphi], inf outside the active rings
    dt_six: np.ndarray     # the same before the StabilizeViscosity clause
    invdt: np.ndarray      # [6, nr, nphi], 0 outside the active rings
    shear: np.ndarray      # [nr], shear limit of pair (n, n+1), inf where the pair does not count
    vmean: np.ndarray

    def binding(self):
        """("cell", i, j, term) or ("shear", n, n+1, "shear"): where dt comes from, and through which term."""
        n = int(np.argmin(self.shear))
        i, j = (int(x) for x in np.unravel_index(int(np.argmin(self.dt_cell)), self.dt_cell.shape))
        if self.shear[n] < self.dt_cell[i, j]:
            return ("shear", n, n + 1, "shear")
        if self.dt_cell[i, j] < self.dt_six[i, j]:
            return ("cell", i, j, "cfac")
        return ("cell", i, j, TERMS[int(np.argmax(np.abs(self.invdt[:, i, j])))])


def condition_cfl(d, g, st, base: "Result | None" = None, rings=None) -> Result:
    """cfl.cpp:185-376 for the slab.  With `base` (the result for a state that differs from `st` only in `rings`: the
    rings whose cells or mean changed) only those rings are evaluated anew."""
    if base is None:
        rings = range(g.nr)
        r = Result(np.inf, np.full((g.nr, g.nphi), np.inf), np.full((g.nr, g.nphi), np.inf),
                   np.zeros((6, g.nr, g.nphi)), np.full(g.nr, np.inf), np.zeros(g.nr))
    else:
        r = Result(base.dt, base.dt_cell.copy(), base.dt_six.copy(), base.invdt.copy(), base.shear.copy(),
                   base.vmean.copy())
    rings = sorted(set(rings))
    for i in rings:
        r.vmean[i] = ring_mean(st["vazi"][i])
    counted = set(shear_pairs(g))
    for i in rings:
        for n in (i - 1, i):
            if n in counted:
                r.shear[n] = _shear_dt(d, g, r.vmean, n)
        if g.first_active <= i < g.active_size:
            t, dt6, stab = eval_ring(d, g, st, i, r.vmean[i])
            r.invdt[:, i], r.dt_six[i], r.dt_cell[i] = t, dt6, np.minimum(dt6, stab)
    r.dt = float(min(r.shear.min(), r.dt_cell.min()))
    return r


# ---------------------------------------------------------------------------------------------------------------
# plants
@dataclass
class Plant:
    name: str
    kind: str
    ring: int
    col: int
    changes: list                 # [(field, index, new value)]: the planted state is the base with these entries
    rings: tuple                  # rings whose cells or mean the changes reach
    bind: "tuple | None" = None   # ("cell", i, j) or ("shear", n, n+1); None: a dead plant, dt must not move
    term: "str | None" = None
    fields: tuple = field(default=())

    def apply(self, st):
        for f, idx, v in self.changes:
            st[f][idx] = v

    def restore(self, st, base):
        for f, idx, _ in self.changes:
            st[f][idx] = base[f][idx]


def _cell_dt(d, g, st, vmean, i, j):
    """dt_cell of one cell in plain Python floats (the same formulas: _terms)."""
    jn = 0 if j == g.nphi - 1 else j + 1
    q = lambda k: float(st[k][i, j]) if k in st else 0.0
    t = _terms(_PY, d, g, i, float(st["vrad"][i, j]), float(st["vrad"][i + 1, j]), float(st["vazi"][i, j]),
               float(st["vazi"][i, jn]), vmean, float(st["sigma"][i, j]), float(st["energy"][i, j]), q("qplus"),
               q("qminus"))
    return _dt_of(_PY, d, t)


def _solve(f, target, start):
    """The amplitude m > 0 with f(m) = target for a decreasing f (f(0) > target): doubling, then bisection."""
    lo, hi = 0.0, start
    for _ in range(200):
        if f(hi) < target:
            break
        lo, hi = hi, 2.0 * hi
    else:
        raise AssertionError("no amplitude reaches the target limit")
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if f(mid) < target:
            hi = mid
        else:
            lo = mid
    return hi


class Planter:
    """Sizes and builds the plants of one base state.  `st` is a scratch copy that every call leaves as it found it."""

    def __init__(self, d, g, base_st, base_res, tighten=PLANT_TIGHTEN):
        self.d, self.g, self.base, self.res = d, g, base_st, base_res
        self.st = {k: v.copy() for k, v in base_st.items()}
        self.target = base_res.dt / tighten

    def active(self, i):
        return self.g.first_active <= i < self.g.active_size

    def _size(self, fld, idx, cell, value_of, start, mean_shift=None):
        """Amplitude m for which dt_cell of `cell` is the target when st[fld][idx] = value_of(m)."""
        i, j = cell
        old = self.st[fld][idx]

        def f(m):
            self.st[fld][idx] = value_of(m)
            vm = self.res.vmean[i] + (mean_shift(m) if mean_shift else 0.0)
            return _cell_dt(self.d, self.g, self.st, vm, i, j)
        try:
            return _solve(f, self.target, start)
        finally:
            self.st[fld][idx] = old

    def _ref_ring(self, i):
        """The active ring whose size rule a dead plant in ring i borrows."""
        return min(max(i, self.g.first_active), self.g.active_size - 1)

    def vr(self, i, j, sign):
        """v_r at face (i, j); dead where neither cell i nor cell i-1 is active.  (A positive v_r at face active_size
        only expands cell active_size-1: neither a plant nor dead, and make_plants does not ask for it.)"""
        g = self.g
        kind = "vr+" if sign > 0 else "vr-"
        name = f"{kind}@face{i}c{j}"
        live_i, live_im = self.active(i), i >= 1 and self.active(i - 1)
        rings = tuple(k for k in (i - 1, i) if 0 <= k < g.nr)
        if sign > 0:
            cell, term = ((i, j), "artvisc") if live_i else (None, None)   # cell i-1 only expands
        elif live_im:
            cell, term = (i - 1, j), "artvisc"
        elif live_i:
            cell, term = (i, j), "vr"
        else:
            cell, term = None, None
        base = float(self.base["vrad"][i, j])
        scale = float(g.cs_iso[min(i, g.nr - 1)])
        if cell is None:   # dead: the amplitude that binds at the nearest active face of the same column
            ref = self._ref_ring(min(i, g.nr - 1))
            m = self._size("vrad", (ref, j), (ref, j), lambda m: float(self.base["vrad"][ref, j]) + m, scale)
            return Plant(name.replace(kind, "dead:" + kind), "dead", i, j, [("vrad", (i, j), base + sign * m)], rings)
        m = self._size("vrad", (i, j), cell, lambda m: base + sign * m, scale)
        return Plant(name, kind, i, j, [("vrad", (i, j), base + sign * m)], rings, ("cell",) + cell, term)

    def vphi(self, i, j, sign):
        g = self.g
        kind = "vphi+" if sign > 0 else "vphi-"
        base = float(self.base["vazi"][i, j])
        shift = lambda m: sign * m / g.nphi
        if not self.active(i):
            ref = self._ref_ring(i)
            b = float(self.base["vazi"][ref, j])
            m = self._size("vazi", (ref, j), (ref, j), lambda m: b + m, float(g.cs_iso[ref]), lambda m: m / g.nphi)
            # the cells of ring i do not count, but its mean does where a counted pair holds the ring (ring 0; ring
            # active_size): there the spike moves dt by m / Nphi through the shear limit and is no dead plant
            pairs = shear_pairs(g)
            dead = all(n not in pairs for n in (i - 1, i))
            return Plant(f"{'dead' if dead else 'mean'}:{kind}@r{i}c{j}", "dead" if dead else "mean", i, j,
                         [("vazi", (i, j), base + sign * m)], (i,))
        cell = (i, j) if sign > 0 else (i, (j - 1) % g.nphi)
        m = self._size("vazi", (i, j), cell, lambda m: base + sign * m, float(g.cs_iso[i]), shift)
        return Plant(f"{kind}@r{i}c{j}", kind, i, j, [("vazi", (i, j), base + sign * m)], (i,), ("cell",) + cell,
                     "artvisc")

    def _scalar(self, kind, fld, i, j, value_of, start, term):
        base = float(self.base[fld][i, j])
        ref = self._ref_ring(i)
        bref = float(self.base[fld][ref, j])
        m = self._size(fld, (ref, j), (ref, j), lambda m: value_of(bref, m), start)
        if not self.active(i):
            return Plant(f"dead:{kind}@r{i}c{j}", "dead", i, j, [(fld, (i, j), value_of(base, m))], (i,))
        return Plant(f"{kind}@r{i}c{j}", kind, i, j, [(fld, (i, j), value_of(base, m))], (i,), ("cell", i, j), term)

    def e(self, i, j):
        """c_s grows with sqrt(e) and the alpha viscosity with e: term 1 binds, or term 5 where the factor is large
        (a base dt far below the sound limit, as without FastTransport) -- the larger of the two at the planted cell."""
        p = self._scalar("e", "energy", i, j, lambda b, m: b * (1.0 + m), 1.0, "sound")
        if p.bind is not None:
            p.apply(self.st)
            g, st = self.g, self.st
            t = _terms(_PY, self.d, g, i, 0.0, 0.0, 0.0, 0.0, 0.0, float(st["sigma"][i, j]), float(st["energy"][i, j]), 0.0, 0.0)
            p.restore(self.st, self.base)
            p.term = "sound" if t[0] >= t[4] else "visc"
        return p

    def q(self, i, j):
        e = float(self.base["energy"][self._ref_ring(i), j])
        return self._scalar("q", "qplus", i, j, lambda b, m: b + m, e / self.res.dt, "heat")

    def cfac(self, i, j, which):
        """-CFL / c = the target: needs no search."""
        c = -self.d.cfl / self.target
        fld = "cfac_phi" if which == "phi" else "cfac_r"
        if not self.active(i):
            return Plant(f"dead:cfac_{which}@r{i}c{j}", "dead", i, j, [(fld, (i, j), c)], ())
        return Plant(f"cfac_{which}@r{i}c{j}", "cfac", i, j, [(fld, (i, j), c)], (i,), ("cell", i, j), "cfac")

    def shear(self, n):
        """The shear limit of pair (n, n+1) at the target, by a uniform offset of one of its two rings: ring 0 for
        pair (0, 1), the upper ring for the last pair (it is not active, and the pair above it does not count), the
        lower ring otherwise -- with the sign that brings the neighbouring pair's angular velocities together."""
        d, g = self.d, self.g
        assert d.fast_transport, "without FastTransport a ring offset is a plant of term 3, not of the shear limit"
        vm = self.res.vmean
        a = vm[n] * g.InvRmed[n] - vm[n + 1] * g.InvRmed[n + 1]
        want = d.cfl * g.dphi / self.target   # |a'| for the target limit
        sgn = 1.0 if a >= 0 else -1.0
        if n + 1 == g.active_size:
            ring, off = n + 1, -(sgn * want - a) * g.Rmed[n + 1]
        else:
            ring, off = n, (sgn * want - a) * g.Rmed[n]
        off *= 1.0 + 1e-9   # (the offset is rounded into every cell: stay on the tight side of the target)
        return Plant(f"shear@pair{n}_{n + 1}(ring{ring})", "shear", ring, -1,
                     [("vazi", (ring, slice(None)), self.base["vazi"][ring] + off)], (ring,), ("shear", n, n + 1), "shear")

    def dead_shear(self, ring, like):
        """The offset of the counted pair `like`, on a ring none of whose pairs count."""
        p = self.shear(like)
        off = float(p.changes[0][2][0] - self.base["vazi"][p.ring, 0])
        return Plant(f"dead:shear@ring{ring}", "dead", ring, -1,
                     [("vazi", (ring, slice(None)), self.base["vazi"][ring] + off)], (ring,))


# ---------------------------------------------------------------------------------------------------------------
# positions
def ring_shape(nphi, ideal, wide_blocks=-1):
    """(threads NT, cell pairs per thread MAXP) of k_cfl_rings for this ring length: with_cfl_ring_shape of
    kernels/launch.h (wide_blocks: the option cfl_wide_blocks).  A hand copy: the profiler reports the kernel's name,
    not its instance, so nothing but this function says where the block boundaries lie -- keep the two in step.  (A
    shape other than the one assumed here still has to give the oracle's dt at every plant; it would only move the
    planted columns off its own block boundaries.)"""
    wide = (not ideal) if wide_blocks < 0 else wide_blocks != 0
    if nphi > 4096:
        return 256, 16
    if nphi > 2048 and wide:
        return 512, 4
    return 256, 8


def columns(nphi, ideal, middle, wide_blocks=-1):
    """Columns of a ring to plant at.  Rings of up to 514 cells: every column of the middle ring; at the other rings
    the ring wrap and the first wavefront boundary of the pair kernel (cells 126-129).  Longer rings: both columns
    of the first and last cell pair of every (thread slot, wavefront) block of k_cfl_rings that exists at this ring
    length, and the wrap."""
    if nphi <= 514:
        if middle:
            return list(range(nphi))
        c = [0, 1, 126, 127, 128, 129, nphi - 2, nphi - 1]
    else:
        nt, maxp = ring_shape(nphi, ideal, wide_blocks)
        npair = nphi // 2
        c = [0, 1, nphi - 2, nphi - 1]
        for n in range(maxp):
            for w in range(nt // 64):
                first = n * nt + 64 * w
                last = min(first + 63, npair - 1)
                if first < npair:
                    c += [2 * first, 2 * first + 1, 2 * last, 2 * last + 1]
    return sorted({x for x in c if 0 <= x < nphi})


def plant_rings(g, split=False):
    """first_active - 1, first_active, a middle ring, active_size - 1, active_size; with the split reduction the
    rings on both sides of its two launch boundaries."""
    mid = (g.first_active + g.active_size) // 2
    r = [g.first_active - 1, g.first_active, mid, g.active_size - 1, g.active_size]
    if split:
        r += [CFL_EDGE_LO - 1, CFL_EDGE_LO, g.nr - CFL_EDGE_HI - 1, g.nr - CFL_EDGE_HI]
    return sorted({x for x in r if 0 <= x < g.nr}), mid


def make_plants(d, g, base_st, base_res, split=False, wide_blocks=-1, every_column=True):
    """All plants of a case, in the order the tests upload them."""
    P = Planter(d, g, base_st, base_res)
    ideal = d.eos == B.EOS_IDEAL
    rings, mid = plant_rings(g, split)
    out = []
    for i in rings:
        full = every_column and i == mid
        edge = {j for j in (0, 1, 126, 127, 128, 129, g.nphi - 2, g.nphi - 1) if 0 <= j < g.nphi}   # wrap, first wavefront boundary
        if g.nphi <= 514:
            cols = columns(g.nphi, ideal, full, wide_blocks)
        else:
            cols = sorted(edge | set(columns(g.nphi, ideal, True, wide_blocks))) if full else sorted(edge)
        for k, j in enumerate(cols):
            # long rings: every kind at the wrap and the wavefront boundary; at the block boundaries the two kinds
            # that tell a skipped slot and a wrong neighbour, and e or Q+ at every other one
            lean = g.nphi > 514 and j not in edge
            for sign in (1, -1):
                if not (sign > 0 and i == g.active_size) and not (lean and sign < 0):
                    out.append(P.vr(i, j, sign))   # (+ at face active_size binds nowhere and is not dead either)
                if not (lean and sign > 0):
                    out.append(P.vphi(i, j, sign))
            if ideal:
                out += [P.e(i, j), P.q(i, j)] if not lean else ([P.e(i, j)] if k % 4 == 0 else [P.q(i, j)] if k % 4 == 2 else [])
            if d.stabilize_viscosity == 2:
                out += [P.cfac(i, j, "phi"), P.cfac(i, j, "r")]
    # v_r rows that no active cell reads: 0 and Nr (and the ghost rows of a slab with neighbours)
    for i in sorted({0, g.nr} | set(range(0, g.first_active)) | set(range(g.active_size + 1, g.nr + 1))):
        for j in (0, g.nphi - 1):
            for sign in (1, -1):
                out.append(P.vr(i, j, sign))
    if d.fast_transport:
        pairs = shear_pairs(g)
        for n in sorted({pairs[0], pairs[1], mid, pairs[-1]}):
            out.append(P.shear(n))
        for ring in range(g.nr):   # rings whose two pairs both do not count (ghost rings of a slab with neighbours)
            if all(n not in pairs for n in (ring - 1, ring) if 0 <= n < g.nr - 1):
                out.append(P.dead_shear(ring, mid))
    seen, uniq = set(), []
    for p in out:   # (a dead row that is also next to a planted ring comes up twice)
        if p.name not in seen:
            seen.add(p.name)
            uniq.append(p)
    out = uniq
    for p in out:
        p.fields = tuple(sorted({c[0] for c in p.changes}))
    return out


def const_nu_for(d, g, res):
    """A constant viscosity with which term 5 of the narrowest ring is PLANT_TIGHTEN times the base limit."""
    i = g.first_active + int(np.argmin(g.cell[g.first_active:g.active_size]))
    return PLANT_TIGHTEN * (d.cfl / res.dt) * g.cell[i] ** 2 / (4.0 * _lf(d))


# ---------------------------------------------------------------------------------------------------------------
# cases, and one library evaluating them
@dataclass(frozen=True)
class Case:
    """One grid shape and descriptor variant.  `options` are the product's kernel switches (the oracle has none);
    `path`: the kernels the product must run ("rings", "cells")."""
    name: str
    nphi: int
    ideal: bool = False
    path: str = "rings"
    options: tuple = ()
    nr: int = 24
    kw: tuple = ()          # case_desc keywords
    const_nu: bool = False
    rank: int = 0
    nranks: int = 1

    @property
    def wide_blocks(self):
        return dict(self.options).get("cfl_wide_blocks", -1)


def _both(name, nphi, path, **kw):
    return [Case(f"{name}-iso", nphi, False, path, **kw), Case(f"{name}-ideal", nphi, True, path, **kw)]


SHAPE_CASES = (
    _both("cells17", 17, "cells") + _both("cells96", 96, "cells") + _both("cells263", 263, "cells") +
    _both("cells8194", 8194, "cells") +
    _both("stab2_320", 320, "cells", kw=(("stabilize", 2),)) +
    _both("rings128", 128, "rings") + _both("rings320", 320, "rings") + _both("rings514", 514, "rings") +
    _both("rings2048", 2048, "rings") +
    [Case("rings512x4_2050-iso", 2050), Case("rings512x4_4096-iso", 4096),
     Case("rings512x4_4096-ideal", 4096, True, options=(("cfl_wide_blocks", 1),)),
     Case("rings256x8_4096-iso", 4096, options=(("cfl_wide_blocks", 0),))] +
    _both("rings256x16_4098", 4098, "rings") + _both("rings256x16_6144", 6144, "rings") +
    _both("rings256x16_8192", 8192, "rings") +
    _both("cells_for_rings320", 320, "cells", options=(("cfl_rings", 0),)) +
    _both("cells_for_rings4096", 4096, "cells", options=(("cfl_rings", 0),)))
VARIANT_CASES = (
    _both("leapfrog320", 320, "rings", kw=(("leapfrog", True),)) + _both("sn320", 320, "rings", kw=(("av", "SN"),)) +
    _both("nofast320", 320, "rings", kw=(("fast", False),)) + _both("constnu320", 320, "rings", const_nu=True) +
    _both("avnone320", 320, "rings", kw=(("av", "None"),)))
SLAB_CASES = [Case(f"slab{r}of3-{'ideal' if a else 'iso'}", 320, a, nr=40, rank=r, nranks=3)
              for r in range(3) for a in (False, True)]
ALL_CASES = SHAPE_CASES + VARIANT_CASES + SLAB_CASES

_SETUPS = {}


def setup_case(lib, case: Case, split=False):
    """(d0, radii, geometry, base state, its Result, plants) of a case; computed once per process."""
    key = (case, split)
    if key not in _SETUPS:
        d = case_desc(lib, case.nr, case.nphi, case.ideal, rank=case.rank, nranks=case.nranks, **dict(case.kw))
        d0, radii, g, base = base_state(lib, d)
        res = condition_cfl(d0, g, base)
        if case.const_nu:
            d0.viscous_alpha, d0.constant_viscosity = 0.0, const_nu_for(d0, g, res)
            res = condition_cfl(d0, g, base)
        plants = make_plants(d0, g, base, res, split=split, wide_blocks=case.wide_blocks)
        _SETUPS[key] = (d0, radii, g, base, res, plants)
    return _SETUPS[key]


class Session:
    """One context of one library holding the base state of a case; `cfl(plant)` uploads what the plant changes
    (and takes back what the plant before it changed), refreshes the derived grids after an upload of e, and
    returns the library's dt."""

    def __init__(self, lib, d0, radii, base, options=()):
        from fargocpt_amd import driver
        self.lib, self.base = lib, base
        self.work = {k: v.copy() for k, v in base.items()}
        self.ctx = driver.make_context(lib, d0, fields=tuple(base[k] for k in ("sigma", "vrad", "vazi", "energy")),
                                       radii=radii)
        for k, v in options:
            self.ctx.set_option(k, v)
        for k in base:   # (init_physics applied the boundary conditions and left its own Q-: the base state again)
            self.ctx.upload(FIELD_IDS[k], base[k])
        self.ctx.recalculate_derived()
        self.dirty = set()

    def load(self, plant=None):
        want = set(plant.fields) if plant is not None else set()
        touched = want | self.dirty
        for f in self.dirty - want:
            self.ctx.upload(FIELD_IDS[f], self.base[f])
        if plant is not None:
            plant.apply(self.work)
            for f in want:
                self.ctx.upload(FIELD_IDS[f], self.work[f])
            plant.restore(self.work, self.base)
        self.dirty = want
        if touched & {"energy", "sigma"}:   # the sound-speed and viscosity grids are otherwise those of the state before
            self.ctx.recalculate_derived()

    def cfl(self, plant=None):
        self.load(plant)
        return self.ctx.cfl()

    def close(self):
        self.ctx.close()


_ORACLE_DTS = {}


def oracle_dts(product, oracle, case: Case, split=False):
    """(base dt, [dt of every plant]) of the oracle for a case; computed once per process.  (`product`: the host
    helpers that build the descriptor and the grid; they need no GPU.)"""
    key = (case, split)
    if key not in _ORACLE_DTS:
        d0, radii, _, base, _, plants = setup_case(product, case, split)
        s = Session(oracle, d0, radii, base)
        dt0 = s.cfl()
        dts = [s.cfl(p) for p in plants]
        assert s.cfl() == dt0
        s.close()
        _ORACLE_DTS[key] = (dt0, dts)
    return _ORACLE_DTS[key]
