"""Known answers for the ghost-ring conditions and the wave damping (plain numpy, no GPU, no oracle).

`ghost_rings` restates boundary_conditions/{zero_gradient,reference,reflecting,outflow,keplerian_radial,
keplerian_azimuthal,zero_shear}.cpp and `damped` restates damping.cpp:311-427 (reference target), :429-557 (zero
target) and :559-700 (mean target), both from the reference's files and in float64; `after_call` puts them in the
order of boundary_conditions.cpp:65-114 (the damping first, then Sigma, e, v_r, v_phi).  Because the damping runs
before the conditions, the ghost rings of any state that a boundary call has left are a closed-form function of that
same state's active rings and of the `*0` grids: a second statement of the operator, independent of the oracle, that
holds bit for bit for every condition that copies a value.

What the reference does and the statement keeps:
  * reflecting v_r has no rank guard (reflecting.cpp:15-40): it writes rows 0, 1 and Nr-1, Nr of every slab;
  * the mean target leaves each damped ring's mean in column 0 of the ring's `*0` grid (damping.cpp:579-586);
  * the zero target of Sigma is sigma_floor * sigma0 at the inner edge (damping.cpp:469-473) and 0.0 at the outer edge
    (damping.cpp:535).  The HIP library and the oracle use the floor at both edges; no case below puts the zero target
    on the outer Sigma, so the difference is written down here and not asserted anywhere;
  * the energy grid is damped only with the ideal EOS, its ghost rings are written with either EOS.

Planted states: `rough_states.noisy` (Sigma, e +-10-30 %, v_r of both signs up to 0.3 c_s, v_phi jitter) for the state
and, with another seed, for the `*0` grids, so that a reference value is never mistaken for the current one; the
direct-call states also carry exact +0.0, -0.0 and values of both signs in rows 2 and Nr-2 of v_r (what outflow and
reflecting read).  `CASES` covers every (variable, condition, side); `GHOST_BINDS_DT` is a state whose next CFL steps
are set by a value that only the boundary call puts into rows 1 and Nr-1 of v_r.
tests/test_boundary_plants_oracle.py holds all of this to its purpose on the CPU.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np

from fargocpt_amd import binding as B, driver
from tests import rough_states as R

EPS = 2.0 ** -52
ZG, REF, REFL, OUT, KEP, ZS, NONE = (B.BC_ZEROGRADIENT, B.BC_REFERENCE, B.BC_REFLECTING, B.BC_OUTFLOW, B.BC_KEPLERIAN,
                                     B.BC_ZEROSHEAR, B.BC_NONE)
BC_NAMES = {ZG: "zero_gradient", REF: "reference", REFL: "reflecting", OUT: "outflow", KEP: "keplerian",
            ZS: "zero_shear", NONE: "none"}
QUANTITIES = ("vrad", "vazi", "sigma", "energy")        # the order of damping_vector (damping.cpp:218-270)
FIELD_IDS = {"sigma": B.F_SIGMA, "vrad": B.F_VRAD, "vazi": B.F_VAZI, "energy": B.F_ENERGY}
FIELD0_IDS = {"sigma": B.F_SIGMA0, "vrad": B.F_VRAD0, "vazi": B.F_VAZI0, "energy": B.F_ENERGY0}
GRIDS = ((16, 8), (24, 67), (40, 320))
SEED0 = 1000     # the `*0` grids: the state's generator with seed + SEED0


# ---------------------------------------------------------------------------------------------------------------
# geometry
def slab_radii(lib, d, radii):
    """The interface radii of the slab's rings and of the one ring beyond them (Nr + 2 values: the outer Keplerian v_r
    reads Rmed[Nr]) out of the global grid's."""
    s = lib.split_domain(d)
    return np.asarray(radii[s.imin:s.imin + s.nr + 2], dtype=np.float64).copy()


def rmed(radii):
    """Rmed of init.cpp:169-225: (2/3) (Rsup^3 - Rinf^3) / (Rsup^2 - Rinf^2)."""
    ri, rs = np.asarray(radii[:-1], dtype=np.float64), np.asarray(radii[1:], dtype=np.float64)
    return (2.0 / 3.0 * (rs * rs * rs - ri * ri * ri)) / (rs * rs - ri * ri)


def _v_kepler(d, r):
    return np.sqrt(d.G * d.hydro_center_mass / r)     # compute_v_kepler (Theo.cpp)


# ---------------------------------------------------------------------------------------------------------------
# the ghost rings
@dataclass
class Ghost:
    rows: tuple            # the rows of the grid the conditions may write
    value: np.ndarray      # [len(rows), nphi]: what they hold afterwards (meaningless where not written)
    written: np.ndarray    # [len(rows)] bool
    bar: np.ndarray        # [len(rows), nphi] absolute bar; 0: equal bits, the sign of zero included


def _scalar_ghost(x, x0, types, is_first, is_last):
    nr, nphi = x.shape
    g = Ghost((0, nr - 1), np.zeros((2, nphi)), np.zeros(2, dtype=bool), np.zeros((2, nphi)))
    for side, (row, act, edge) in enumerate(((0, 1, is_first), (nr - 1, nr - 2, is_last))):
        if not edge:
            continue
        if types[side] == ZG:       # zero_gradient.cpp:16-25, :52-62
            g.value[side], g.written[side] = x[act], True
        elif types[side] == REF:    # reference.cpp:16-25, :52-62
            g.value[side], g.written[side] = x0[row], True
    return g


def ghost_rings(d, radii, state, state0, is_first, is_last):
    """What the conditions of `d` leave in the ghost rings, from the active rings of `state` (grids of one slab:
    sigma, vazi, energy [Nr, Nphi], vrad [Nr + 1, Nphi]), the `*0` grids `state0` and the slab's Nr + 2 interface
    `radii` (slab_radii): {"sigma", "energy", "vazi": Ghost of rows 0 / Nr-1; "vrad": Ghost of rows 0, 1 / Nr-1, Nr}.  BC_NONE and
    the guarded side of a slab with a neighbour write nothing; reflecting v_r writes on every slab."""
    rm = rmed(radii)
    nr, nphi = state["sigma"].shape
    out = {"sigma": _scalar_ghost(state["sigma"], state0["sigma"], d.bc_sigma, is_first, is_last)}
    if "energy" in state:   # (a state downloaded without the grid that the isothermal EOS does not evolve)
        out["energy"] = _scalar_ghost(state["energy"], state0["energy"], d.bc_energy, is_first, is_last)
    # ---- v_r: rows 0, 1 from row 2; rows Nr, Nr-1 from row Nr-2 (the vector grid's max_radial is Nr)
    vr, vr0 = state["vrad"], state0["vrad"]
    g = Ghost((0, 1, nr - 1, nr), np.zeros((4, nphi)), np.zeros(4, dtype=bool), np.zeros((4, nphi)))
    for side, edge in enumerate((is_first, is_last)):
        far, near, act = (0, 1, 2) if side == 0 else (nr, nr - 1, nr - 2)
        kf, kn = (0, 1) if side == 0 else (3, 2)
        t = d.bc_vrad[side]
        if t == REFL:               # reflecting.cpp:15-40: no rank guard
            g.value[kf], g.value[kn] = -vr[act], 0.0
        elif not edge or t == NONE:
            continue
        elif t == ZG:               # zero_gradient.cpp:27-37, :64-75
            g.value[kf] = g.value[kn] = vr[act]
        elif t == REF:              # reference.cpp:27-37, :64-75
            g.value[kf], g.value[kn] = vr0[far], vr0[near]
        elif t == OUT:              # outflow.cpp:26-34, :48-56: inflow is cut to zero, outflow is kept
            inflow = (vr[act] > 0.0) if side == 0 else (vr[act] < 0.0)
            g.value[kf] = g.value[kn] = np.where(inflow, 0.0, vr[act])
        elif t == KEP:              # keplerian_radial.cpp:30-37, :54-61: c v_K(Rmed[k]) on the two rows
            c = d.keplerian_vrad_factor[side]
            for k, row in ((kf, far), (kn, near)):
                g.value[k] = c * _v_kepler(d, rm[row])
                g.bar[k] = 8.0 * EPS * np.abs(g.value[k])
        else:
            continue
        g.written[kf] = g.written[kn] = True
    out["vrad"] = g
    # ---- v_phi
    va, va0 = state["vazi"], state0["vazi"]
    g = Ghost((0, nr - 1), np.zeros((2, nphi)), np.zeros(2, dtype=bool), np.zeros((2, nphi)))
    for side, (row, act, edge) in enumerate(((0, 1, is_first), (nr - 1, nr - 2, is_last))):
        t = d.bc_vaz[side]
        if not edge or t == NONE:
            continue
        if t == ZG:
            g.value[side] = va[act]
        elif t == REF:
            g.value[side] = va0[row]
        elif t == KEP:              # keplerian_azimuthal.cpp:29-37, :51-59: c v_K - r OmegaFrame
            a, b = d.keplerian_vaz_factor[side] * _v_kepler(d, rm[row]), rm[row] * d.omega_frame
            g.value[side] = a - b
            g.bar[side] = 8.0 * EPS * (abs(a) + abs(b))
        elif t == ZS:               # zero_shear.cpp:28-34, :46-52: r (v(active) / r(active))
            g.value[side] = rm[row] * (va[act] / rm[act])
            g.bar[side] = 4.0 * EPS * np.abs(g.value[side])
        else:
            continue
        g.written[side] = True
    out["vazi"] = g
    return out


def ghost_mismatch(d, radii, state, state0, is_first=True, is_last=True, fields=QUANTITIES):
    """The written ghost rows of `state` against `ghost_rings` of its own active rings: a list of messages (empty:
    all hold) and, per kind of bar, the largest deviation in units of the bar (bit rows: the count of wrong cells)."""
    bad, worst = [], {}
    for name, g in ghost_rings(d, radii, state, state0, is_first, is_last).items():
        if name not in fields:
            continue
        for k, row in enumerate(g.rows):
            if not g.written[k]:
                continue
            got, want, bar = state[name][row], g.value[k], g.bar[k]
            exact = bar == 0.0
            wrong = exact & ((got != want) | (np.signbit(got) != np.signbit(want)))
            dev = np.where(exact, 0.0, np.abs(got - want) / np.where(exact, 1.0, bar))
            dev = np.where(np.isnan(got), np.inf, dev)
            cond = BC_NAMES[{"sigma": d.bc_sigma, "energy": d.bc_energy, "vrad": d.bc_vrad,
                             "vazi": d.bc_vaz}[name][0 if row < 2 else 1]]
            key = f"{name}:{cond}"
            worst[key] = max(worst.get(key, 0.0), float(wrong.sum()) if exact.all() else float(dev.max()))
            if wrong.any() or (dev > 1.0).any():
                j = int(np.argmax(wrong)) if wrong.any() else int(np.argmax(dev))
                bad.append(f"{name} row {row} ({cond}): {int(wrong.sum())} cells with other bits, largest deviation "
                           f"{float(dev.max()):.3g} bars, e.g. column {j}: {got[j]!r} vs {want[j]!r}")
    return bad, worst


# ---------------------------------------------------------------------------------------------------------------
# the wave damping
def _damping_radius(radii, which):
    """Ra of the vector grid's Nr + 1 rows, Rb of a scalar grid's Nr rows (`radii`: slab_radii)."""
    return np.asarray(radii[:-1], dtype=np.float64) if which == "vrad" else rmed(radii)[:-1]


def damping_zone(d, radii, which, side):
    """(lo, hi, rlim, redge, tau) of one damping zone of the slab, rows lo .. hi inclusive; lo > hi: none here.
    Scalars are placed by Rmed, v_r by Rinf; the zone ends at the last ring whose radius does not exceed the limit
    (get_rmed_id / get_rinf_id, find_cell_id.cpp), the outer zone starts one ring further out."""
    radius = _damping_radius(radii, which)
    top = len(radius) - 1
    omega_k = lambda r: math.sqrt(d.G * d.hydro_center_mass / (r * r * r))
    if side == 0:
        rlim = d.rmin * d.damping_inner_limit
        if not (d.damping_inner_limit > 1.0 and radius[0] < rlim):
            return 0, -1, rlim, d.rmin, 1.0
        hi = int(np.searchsorted(radius, rlim, side="right")) - 1
        return 0, min(max(hi, 0), top), rlim, d.rmin, d.damping_time_factor * 2.0 * math.pi / omega_k(d.rmin)
    rlim = d.rmax * d.damping_outer_limit
    if not (d.damping_outer_limit < 1.0 and radius[top] > rlim):
        return 0, -1, rlim, d.rmax, 1.0
    lo = int(np.searchsorted(radius, rlim, side="right"))
    tau = d.damping_time_factor * 2.0 * math.pi / omega_k(d.damping_time_radius_outer)
    return min(max(lo, 0), top), top, rlim, d.rmax, tau


def damp_type(d, which, side):
    return {"vrad": d.damp_vrad, "vazi": d.damp_vaz, "sigma": d.damp_sigma, "energy": d.damp_energy}[which][side]


def damped(d, radii, q, q0, dt, which, side):
    """X' = (X - X0) exp(-dt f / tau) + X0 over the rings of one zone, f = ((r - r_lim) / (r_edge - r_lim))^2.
    -> (the damped copy of q, lo, hi, absolute bar [shape of q, 0 outside the zone], ring means or None).
    X0: the `*0` grid (reference), the ring's mean taken with math.fsum (mean), or zero -- for Sigma the absolute floor
    at the inner edge and 0.0 at the outer one (see the module docstring)."""
    out, bar = q.copy(), np.zeros_like(q)
    t = damp_type(d, which, side)
    lo, hi, rlim, redge, tau = damping_zone(d, radii, which, side)
    if t == B.DAMP_NONE or not d.damping or lo > hi:
        return out, 0, -1, bar, None
    radius = _damping_radius(radii, which)
    nphi = q.shape[1]
    means = {}
    for i in range(lo, hi + 1):
        factor = ((radius[i] - rlim) / (redge - rlim)) ** 2
        ef = math.exp(-dt * factor / tau)
        extra = 0.0
        if t == B.DAMP_REFERENCE:
            x0 = q0[i]
        elif t == B.DAMP_MEAN:
            x0 = means[i] = math.fsum(q[i]) / nphi
            extra = nphi * EPS * float(np.mean(np.abs(q[i])))     # the ring sum in any order
        else:
            x0 = d.sigma_floor * d.sigma0 if (which == "sigma" and side == 0) else 0.0
        out[i] = (q[i] - x0) * ef + x0
        bar[i] = 16.0 * EPS * (np.abs(q[i]) + np.abs(x0)) * (1.0 + dt * factor / tau) + extra
    return out, lo, hi, bar, (means if t == B.DAMP_MEAN else None)


def after_call(d, radii, state, state0, dt, final, is_first, is_last, ideal):
    """apply_boundary_condition(dt, final) on a state (boundary_conditions.cpp:65-114): the damping of every quantity
    and side in the order of damping_vector, then the conditions.
    -> (expected grids, absolute bars of the damped rows, the `*0` grids with the means the mean target leaves in
    column 0, {grid: the ghost rows the conditions wrote}, absolute bars of the `*0` grids: the ring sum's, on those
    means).  The written ghost rows are best held against `ghost_rings`
    of the state under test itself (ghost_mismatch), which needs no bar for a copied value."""
    st = {k: v.copy() for k, v in state.items()}
    st0 = {k: v.copy() for k, v in state0.items()}
    bars = {k: np.zeros_like(v) for k, v in state.items()}
    bars0 = {k: np.zeros_like(v) for k, v in state0.items()}
    if final and d.damping:
        for which in QUANTITIES:
            if which == "energy" and not ideal:    # dropped from damping_vector without the ideal EOS
                continue
            for side in (0, 1):
                before = st[which]
                st[which], lo, hi, bar, means = damped(d, radii, before, st0[which], dt, which, side)
                bars[which] = np.maximum(bars[which], bar)
                for i, m in (means or {}).items():
                    st0[which][i, 0] = m
                    bars0[which][i, 0] = before.shape[1] * EPS * float(np.mean(np.abs(before[i])))
    written = {}
    for name, g in ghost_rings(d, radii, st, st0, is_first, is_last).items():
        written[name] = [row for k, row in enumerate(g.rows) if g.written[k]]
        for k, row in enumerate(g.rows):
            if g.written[k]:
                st[name][row] = g.value[k]
    return st, bars, st0, written, bars0


# ---------------------------------------------------------------------------------------------------------------
# cases
@dataclass(frozen=True)
class Case:
    name: str
    sigma: tuple
    energy: tuple
    vrad: tuple
    vaz: tuple
    omega_frame: float
    damping: bool = True
    damp: tuple = ()                  # ((quantity, (inner, outer)), ...); quantities not named: none
    kep_vrad: tuple = (0.003, -0.002)  # c v_K as a radial velocity: 0.06 and -0.04 c_s at h = 0.05
    kep_vaz: tuple = (0.995, 1.004)
    seed: int = 3
    damping_limits: tuple = (1.6, 0.65)   # zones of >= 3 rings on the coarsest grid (16 rings)

    def conditions(self):
        return {"sigma": self.sigma, "energy": self.energy, "vrad": self.vrad, "vazi": self.vaz}

    def damps(self):
        return self.damping and any(t != B.DAMP_NONE for _, ts in self.damp for t in ts)

    def has_mean(self):
        return self.damping and any(t == B.DAMP_MEAN for _, ts in self.damp for t in ts)


_DR, _DZ, _DM, _DN = B.DAMP_REFERENCE, B.DAMP_ZERO, B.DAMP_MEAN, B.DAMP_NONE
CASES = (
    Case("reflect_out", (ZG, REF), (REF, NONE), (REFL, OUT), (KEP, ZS), 1.0,
         damp=(("vrad", (_DR, _DR)), ("vazi", (_DR, _DR)), ("sigma", (_DR, _DR)), ("energy", (_DR, _DR)))),
    # (no damping of the inner v_r and this seed: on 16 x 8 the inner edge flows one way in all 8 columns by the third
    #  step otherwise, and one of the two inner outflow branches is not reached; seeds 12, 31, 49, 54, 59 of 1 .. 79 hold)
    Case("out_reflect", (REF, NONE), (NONE, ZG), (OUT, REFL), (ZS, KEP), 0.0,
         damp=(("vrad", (_DN, _DZ)), ("sigma", (_DZ, _DN)), ("energy", (_DN, _DZ))), seed=12),
    Case("zg_ref_undamped", (NONE, ZG), (ZG, REF), (ZG, REF), (REF, ZG), 1.0, damping=False),
    Case("ref_kep_mean", (ZG, NONE), (REF, ZG), (REF, KEP), (ZG, NONE), 0.0,
         damp=(("vrad", (_DN, _DM)), ("vazi", (_DN, _DM)), ("sigma", (_DM, _DR)), ("energy", (_DN, _DM)))),
    Case("kep_none_mixed", (REF, ZG), (ZG, NONE), (KEP, NONE), (NONE, REF), 1.0,
         damp=(("vrad", (_DR, _DZ)), ("vazi", (_DZ, _DR)), ("sigma", (_DR, _DR)), ("energy", (_DZ, _DR)))),
    Case("none_zg", (NONE, REF), (NONE, REF), (NONE, ZG), (KEP, REF), 0.0,
         damp=(("vazi", (_DR, _DN)), ("energy", (_DZ, _DN)))),
)
CASE_BY_NAME = {c.name: c for c in CASES}
WANTED = ({("sigma", t) for t in (ZG, REF, NONE)} | {("energy", t) for t in (ZG, REF, NONE)} |
          {("vrad", t) for t in (ZG, REF, REFL, OUT, KEP, NONE)} | {("vazi", t) for t in (ZG, REF, KEP, ZS, NONE)})


def desc(lib, case, nr, nphi, ideal, rank=0, nranks=1, leapfrog=False):
    """The descriptor of a case on a slab of `nr` rings (a global grid of nr * nranks)."""
    d = R.case_desc(lib, nr * nranks, nphi, physics="visc" if ideal else "iso", kind="noisy", leapfrog=leapfrog)
    d.rank, d.nranks = rank, nranks
    d.omega_frame = case.omega_frame
    for side in (0, 1):
        d.bc_sigma[side], d.bc_energy[side] = case.sigma[side], case.energy[side]
        d.bc_vrad[side], d.bc_vaz[side] = case.vrad[side], case.vaz[side]
        d.keplerian_vrad_factor[side], d.keplerian_vaz_factor[side] = case.kep_vrad[side], case.kep_vaz[side]
        for arr in (d.damp_vrad, d.damp_vaz, d.damp_sigma, d.damp_energy):
            arr[side] = B.DAMP_NONE
    for which, types in case.damp:
        arr = {"vrad": d.damp_vrad, "vazi": d.damp_vaz, "sigma": d.damp_sigma, "energy": d.damp_energy}[which]
        arr[0], arr[1] = types
    d.damping = 1 if case.damping else 0
    d.damping_inner_limit, d.damping_outer_limit = case.damping_limits
    return d


def _named(fields):
    return {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in zip(("sigma", "vrad", "vazi", "energy"), fields)}


_STATES = {}


def planted(lib, case, nr, nphi, ideal, nranks=1, leapfrog=False, signed_zeros=False, plant=None):
    """(descriptor of the global grid, global radii, state, `*0` grids) of a case, global grids by name; computed once
    per process and never changed by a caller.  `signed_zeros`: the direct-call pattern in rows 2 and Nr-2 of v_r, by
    column modulo 8: +0.0, -0.0, +|v|, -|v|, then four columns as they were.  `plant(d0, radii, st, st0)` may change
    the grids once more (GHOST_BINDS_DT)."""
    key = (case, nr, nphi, ideal, nranks, leapfrog, signed_zeros, plant)
    if key not in _STATES:
        d = desc(lib, case, nr, nphi, ideal, 0, nranks, leapfrog)
        d0, radii, fields = R.make_state(lib, d, "noisy", seed=case.seed)
        _, _, fields0 = R.make_state(lib, d, "noisy", seed=case.seed + SEED0)
        st, st0 = _named(fields), _named(fields0)
        if signed_zeros:
            j = np.arange(nphi)
            for row in (2, st["vrad"].shape[0] - 3):
                v = st["vrad"][row]
                mag = np.maximum(np.abs(v), 1e-3 * np.abs(v).max())
                st["vrad"][row] = np.where(j % 8 == 0, 0.0, np.where(j % 8 == 1, -0.0, np.where(
                    j % 8 == 2, mag, np.where(j % 8 == 3, -mag, v))))
        if plant is not None:
            plant(d0, radii, st, st0)
        for v in list(st.values()) + list(st0.values()):
            v.setflags(write=False)
        _STATES[key] = (d0, radii, st, st0)
    return _STATES[key]


def cut(lib, d0, radii, grids, rank, nranks):
    """(descriptor, split, the slab's rows of global grids)."""
    dd = d0.copy()
    dd.rank, dd.nranks = rank, nranks
    s = lib.split_domain(dd)
    return dd, s, {k: np.ascontiguousarray(v[s.imin:s.imin + s.nr + (1 if k == "vrad" else 0)]) for k, v in grids.items()}


def make_slab(lib, d0, radii, st, st0, rank=0, nranks=1, options=()):
    """A context of `lib` holding the slab's part of a planted state and of its `*0` grids (uploaded after
    init_physics, which stores the initial state there), with the product's options set."""
    dd, s, sub = cut(lib, d0, radii, st, rank, nranks)
    _, _, sub0 = cut(lib, d0, radii, st0, rank, nranks)
    ctx = driver.make_context(lib, dd, fields=tuple(sub[k] for k in ("sigma", "vrad", "vazi", "energy")), radii=radii)
    for k, v in options:
        ctx.set_option(k, v)
    for k in sub0:
        ctx.upload(FIELD0_IDS[k], sub0[k])
    return ctx, dd, s, sub, sub0


def download(ctx, ideal=True):
    return {k: ctx.download(f) for k, f in FIELD_IDS.items() if ideal or k != "energy"}


def run(lib, d0, radii, st, st0, nsteps, mode="host", nslabs=1, options=(), noise=0.0, profile=None, each_step=None):
    """`nsteps` from a planted state.  mode "host": cfl -> calculate_timestep -> step -> post (driver.SlabSet), with
    `each_step(k, SlabSet)` after every step; "device": fcpt_run_steps on one slab.  `noise`: cell-wise relative noise on the
    state (seeded).  `profile`: kernel names to count on slab 0.
    -> SimpleNamespace(state: global grids, dts, time, prof, options: the options read back)."""
    if noise:
        rng = np.random.default_rng(7)
        st = {k: v * (1.0 + noise * rng.standard_normal(v.shape)) for k, v in st.items()}
    ctxs = [make_slab(lib, d0, radii, st, st0, r, nslabs, options)[0] for r in range(nslabs)]
    try:
        S = driver.SlabSet(ctxs)
        S.prepare()
        prof, dts = {}, []
        if profile:
            names = lib.kernel_names()
            ctxs[0].profile_start([names.index(n) for n in profile], max_launches=256)
        if mode == "host":
            for k in range(nsteps):
                dts.append(S.step())
                if each_step is not None:
                    each_step(k, S)
        else:
            assert nslabs == 1
            assert ctxs[0].run_steps(nsteps) == nsteps
        if profile:
            prof = {n: c for n, (_, c) in ctxs[0].profile_stop().items()}
        state = S.gather()
        if "energy" in state and d0.eos != B.EOS_IDEAL:
            del state["energy"]
        back = {k: ctxs[0].get_option(k) for k, _ in options} if lib.has("get_option") else {}
        extra = {"graph_replays": ctxs[0].get_option("graph_replays")} if options and lib.has("get_option") else {}
        return SimpleNamespace(state=state, dts=dts, time=ctxs[0].clock.time, prof=prof, options=back, **extra)
    finally:
        for c in ctxs:
            c.close()


NSTEPS = 3
GRAPH_NSTEPS = 8     # fcpt_run_steps replays a captured graph only in calls of 8 steps and more
LEAPFROG_CASES = ("reflect_out", "kep_none_mixed")
SLAB_CASES = ("reflect_out", "out_reflect")     # reflecting and outflow v_r on three slabs
SLAB_GRIDS = ((48, 320), (48, 67))              # global grids cut into three slabs
_ORACLE_RUNS = {}


def oracle_run(product, oracle, case, nr, nphi, ideal, leapfrog=False, plant=None, nsteps=NSTEPS):
    """The oracle's host loop from the planted state of a case, once per process: `run`'s result with .snaps, the
    state after every step, and the case's (d0, radii, st, st0) as .planted."""
    key = (case, nr, nphi, ideal, leapfrog, plant, nsteps)
    if key not in _ORACLE_RUNS:
        p = planted(product, case, nr, nphi, ideal, leapfrog=leapfrog, plant=plant)
        snaps = []
        r = run(oracle, *p, nsteps, each_step=lambda k, S: snaps.append(download(S.ctxs[0], ideal)))
        r.snaps, r.planted = snaps, p
        _ORACLE_RUNS[key] = r
    return _ORACLE_RUNS[key]


def damping_times(d):
    """(tau of the inner zone, tau of the outer zone): DampingTimeFactor orbits at RMIN and at DampingTimeRadiusOuter."""
    omega_k = lambda r: math.sqrt(d.G * d.hydro_center_mass / (r * r * r))
    return (d.damping_time_factor * 2.0 * math.pi / omega_k(d.rmin),
            d.damping_time_factor * 2.0 * math.pi / omega_k(d.damping_time_radius_outer))


def _rows_mismatch(name, got, want, bar, skip_rows):
    bad, worst = [], 0.0
    for row in range(got.shape[0]):
        if row in skip_rows:
            continue
        exact = bar[row] == 0.0
        wrong = exact & ((got[row] != want[row]) | (np.signbit(got[row]) != np.signbit(want[row])))
        dev = np.where(exact, 0.0, np.abs(got[row] - want[row]) / np.where(exact, 1.0, bar[row]))
        dev = np.where(np.isnan(got[row]), np.inf, dev)
        worst = max(worst, float(dev.max()))
        if wrong.any() or (dev > 1.0).any():
            j = int(np.argmax(wrong)) if wrong.any() else int(np.argmax(dev))
            bad.append(f"{name} row {row}: {int(wrong.sum())} cells outside the damping zones changed bits, largest "
                       f"deviation {float(dev.max()):.3g} bars, e.g. column {j}: {got[row, j]!r} vs {want[row, j]!r}")
    return bad, worst


def direct_calls(lib, product, case, nr, nphi, ideal, rank=0, nranks=1, launches=None):
    """apply_boundary(0, False) and (dt, True), dt = 0.7 tau of the inner and of the outer zone, of `lib` on the planted
    direct-call state of a case, each from the same uploaded state: the rows the conditions do not write against
    `damped` (bit for bit outside the zones), the rows they write against `ghost_rings` of the downloaded state itself.
    -> (messages, {bar: largest deviation in units of the bar}).  `launches`: a dictionary that receives the launch counts
    of k_boundary and k_damping over the three calls (the product only)."""
    d0, radii, st, st0 = planted(product, case, nr, nphi, ideal, nranks, signed_zeros=True)
    ctx, dd, s, sub, sub0 = make_slab(lib, d0, radii, st, st0, rank, nranks)
    rad = slab_radii(product, dd, radii)
    first, last = bool(s.is_first), bool(s.is_last)
    bad, worst = [], {}
    try:
        if launches is not None:
            names = lib.kernel_names()
            ctx.profile_start([names.index("k_boundary"), names.index("k_damping")], max_launches=64)
        for dt, final in [(0.0, False)] + [(0.7 * tau, True) for tau in damping_times(dd)]:
            for k in sub:
                ctx.upload(FIELD_IDS[k], sub[k])
                ctx.upload(FIELD0_IDS[k], sub0[k])
            ctx.apply_boundary(dt, final)
            got = download(ctx)
            want, bars, want0, written, bars0 = after_call(dd, rad, sub, sub0, dt, final, first, last, ideal)
            tag = f"{case.name} {nr}x{nphi} {'ideal' if ideal else 'iso'} rank {rank}/{nranks} ({dt:.3g}, {final})"
            for name in got:
                b, w = _rows_mismatch(name, got[name], want[name], bars[name], written[name])
                bad += [f"{tag}: {m}" for m in b]
                worst["damping"] = max(worst.get("damping", 0.0), w)
            for name, f0 in FIELD0_IDS.items():     # the `*0` grids: untouched, but for the means of the mean target
                b, w = _rows_mismatch(name + "0", ctx.download(f0), want0[name], bars0[name], ())
                bad += [f"{tag}: {m}" for m in b]
                worst["mean"] = max(worst.get("mean", 0.0), w)
            b, w = ghost_mismatch(dd, rad, got, want0, first, last)
            bad += [f"{tag}: {m}" for m in b]
            for key, v in w.items():
                worst[key] = max(worst.get(key, 0.0), v)
        if launches is not None:
            launches.update({n: c for n, (_, c) in ctx.profile_stop().items()})
    finally:
        ctx.close()
    return bad, worst


def outflow_census(d, state):
    """Columns of a state that took each of the four outflow branches in the boundary call that left it: the kept
    value and the zero are both in the ghost row, the decision is read from row 2 / Nr-2."""
    vr = state["vrad"]
    c = {}
    if d.bc_vrad[0] == OUT:
        c["inner_keep"], c["inner_zero"] = int((vr[2] <= 0.0).sum()), int((vr[2] > 0.0).sum())
    if d.bc_vrad[1] == OUT:
        c["outer_keep"], c["outer_zero"] = int((vr[-3] >= 0.0).sum()), int((vr[-3] < 0.0).sum())
    return c


# ---------------------------------------------------------------------------------------------------------------
# a ghost value that sets the time step
GHOST_BINDS_DT = Case("ghost_binds_dt", (NONE, NONE), (ZG, ZG), (REF, REF), (KEP, NONE), 1.0,
                      damp=(("vrad", (_DR, _DR)), ("vazi", (_DR, _DR)), ("sigma", (_DR, _DR))))
BINDS_GRID = (40, 320)
BINDS_EVERY, BINDS_CS = 40, 2.0


def binds_plant(d0, radii, st, st0):
    """+2 c_s in row 1 and -2 c_s in row Nr-1 of VRAD0, in every 40th column: with reference v_r on both sides only
    the boundary call brings them into v_r, where they compress cells 1 and Nr-2, whose artificial-viscosity terms then
    set dt (the oracle's dt falls to 0.21 .. 0.28 of the unplanted run's in each of the four steps).  The opposite
    signs (-2 c_s inside, +2 c_s outside) only expand the two cells: dt then moves by 8.5e-4 in step 2, through the
    flow and not through the CFL terms of the two rings, which is less than the census asks and not what the plant
    is for."""
    nr = st["sigma"].shape[0]
    rm = rmed(radii[:nr + 1])      # (the global grid's radii)
    cs = d0.aspect_ratio * rm ** d0.flaring_index * _v_kepler(d0, rm)
    st0["vrad"][1, ::BINDS_EVERY] = BINDS_CS * cs[1]
    st0["vrad"][nr - 1, ::BINDS_EVERY] = -BINDS_CS * cs[nr - 2]
