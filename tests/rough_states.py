"""Rough initial states for the parity tests: noise, patches at the floors and ceilings, and discontinuities on
the seams of the marching kernels -- the inputs that drive the branches a smooth, slightly perturbed disk never
reaches (the density floor of the transport, the temperature floor and ceiling, the low-Sigma equilibrium of
SubStep3, the limiter's zero slope, the artificial viscosity's compressive faces).  Plain numpy, seeded: the same
case gives the same state everywhere.  Every state is physical (Sigma > 0, e > 0, every value finite).

`census(...)` counts how many cells or faces of an input state reach each branch, `post_census(...)` what the
oracle's first step did with it; tests/test_rough_states_census.py holds the generators to their purpose without a
GPU, tests/test_gpu_rough_states.py compares the HIP library with the oracle from these states.
"""
from __future__ import annotations

import numpy as np

from fargocpt_amd import binding as B, setups

MARCH_VALID = 59          # columns one segment of the marching source kernel advances (kernels/source_march.h)
TILE = 64                 # lanes of one column tile of the fused transport kernel (C = 1)
SEAMS = ((58, 59), (63, 64), (127, 128))   # column pairs on the seams above; (Nphi-1, 0) is the wrap
JUMP = 0.5                # a neighbour ratio beyond 1 +- JUMP counts as an edge
MIN_COUNT = 16            # cells or faces each intended branch must reach

# ---------------------------------------------------------------------------------------------------------------
# descriptors


def case_desc(lib, nr, nphi, physics="iso", kind="noisy", av="TW", leapfrog=False, massflow=False) -> B.Desc:
    """A planet_disk descriptor with the physics of one case.  `physics`: iso (locally isothermal), visc (ideal EOS,
    viscous heating), cool_const / cool_lin (+ surface cooling, Opacity Const / Lin), beta (+ beta cooling towards
    the temperature floor).  The floored states use a density floor of 1e-2 Sigma0 (low-Sigma threshold 0.1 Sigma0),
    so that a patch at the floor is a contrast of 1e2, not 1e9, against the disk around it."""
    adiabatic = physics != "iso"
    d = setups.planet_disk(lib, nr, nphi, adiabatic=adiabatic)
    d.artificial_viscosity = {"TW": B.ARTVISC_TW, "SN": B.ARTVISC_SN}[av]
    if leapfrog:
        d.integrator = B.INTEGRATOR_LEAPFROG
    if physics in ("cool_const", "cool_lin"):
        d.cooling_surface = 1
        d.opacity = B.OPACITY_CONST if physics == "cool_const" else B.OPACITY_LIN
        d.kappa_const = 1.0e4
    elif physics == "beta":
        d.cooling_beta, d.cooling_beta_value, d.cooling_beta_reference = 1, 10.0, B.BETAREF_FLOOR
    d.heating_cooling_cfl_limit = 10.0
    d.first_dt = 1.0   # no ramp from a fixed first step: both steps run at the CFL reduction's time step
    if kind == "shift_jump":
        d.damping = 0
    if kind == "floored":
        d.sigma_floor = 1.0e-2
    d.write_massflow = 1 if massflow else 0
    return d


def _cs(d, radii, sigma, energy):
    """Local sound speed of cells: h v_K(r) (isothermal) or sqrt(gamma (gamma-1) e / Sigma)."""
    nr = sigma.shape[0]
    ri = np.asarray(radii[:nr + 1])
    r = 0.5 * (ri[:-1] + ri[1:])
    if d.eos == B.EOS_IDEAL:
        g = d.adiabatic_index
        return np.sqrt(g * (g - 1.0) * energy / sigma)
    return np.broadcast_to((d.aspect_ratio * r ** d.flaring_index * np.sqrt(d.G * d.hydro_center_mass / r))[:, None],
                           sigma.shape).copy()


def _aspect(radii, nr, nphi):
    """min(1, r dphi / dr) of every ring (column vector): velocity jumps between neighbouring columns scaled by it
    strain long, thin cells no harder than square ones (the artificial viscosity's length is the radial width)."""
    ri = np.asarray(radii[:nr + 1])
    r = 0.5 * (ri[:-1] + ri[1:])
    return np.minimum(1.0, r * 2 * np.pi / nphi / (ri[1:] - ri[:-1]))[:, None]


def e_bounds(d, sigma):
    """(e_min, e_max) of cells: SetTemperatureFloorCeilValues (SourceEuler.cpp:136-202)."""
    f = d.Rgas / (d.adiabatic_index - 1.0)
    return d.minimum_temperature * sigma / d.mu * f, d.maximum_temperature * sigma / d.mu * f


def low_sigma_threshold(d) -> float:
    """SubStep3's low-Sigma threshold, in the operation order of the kernels and the oracle (source_march.h:729)."""
    return 10.0 * d.sigma0 * d.sigma_floor


def slab_edges(lib, d, nslabs):
    """First global ring of every slab but the first (where two slabs meet)."""
    out = []
    for rank in range(1, nslabs):
        dd = d.copy()
        dd.rank, dd.nranks = rank, nslabs
        out.append(int(lib.split_domain(dd).imin) + B.OVERLAP)
    return out


# ---------------------------------------------------------------------------------------------------------------
# states


def base_state(lib, d):
    """(descriptor of the global grid, radii, [Sigma, v_r, v_phi, e]) of lib.initial_fields.  For the ideal EOS the
    temperature ceiling becomes finite: 1.5 x the hottest initial cell, so that it binds only where a state puts it."""
    d0 = d.copy()
    d0.rank, d0.nranks = 0, 1
    radii = lib.radii(d0)
    fields = [f.copy() for f in lib.initial_fields(d0, radii)]   # (d0.sigma0 possibly rescaled)
    if d0.eos == B.EOS_IDEAL:
        t = fields[3] / fields[0] * d0.mu / d0.Rgas * (d0.adiabatic_index - 1.0)
        d0.maximum_temperature = 1.5 * float(t.max())
    return d0, radii, fields


def _ring_mean_free(x):
    return x - x.mean(axis=1, keepdims=True)


def noisy(lib, d, seed=0, nslabs=1):
    """10-30 % cell-wise noise in Sigma and e; v_r of both signs up to 0.3 c_s, with exact zeros on every fifth face
    of every fourth ring; v_phi jitter of 0.05 c_s with each ring's mean removed, so that no ring's FARGO shift moves
    (the fused transport stays on its fused path).  Both velocity amplitudes are scaled by _aspect."""
    d0, radii, (sig, vr, va, e) = base_state(lib, d)
    rng = np.random.default_rng(seed)
    nr, nphi = sig.shape
    amp = rng.uniform(0.1, 0.3, size=(nr, 1))
    sig *= 1.0 + amp * rng.uniform(-1.0, 1.0, size=sig.shape)
    if d0.eos == B.EOS_IDEAL:
        e *= 1.0 + amp * rng.uniform(-1.0, 1.0, size=e.shape)
    cs = _cs(d0, radii, sig, e)
    csf = np.vstack([cs[:1], 0.5 * (cs[:-1] + cs[1:]), cs[-1:]])
    asp = _aspect(radii, nr, nphi)
    vr = vr + 0.3 * csf * np.vstack([asp[:1], asp]) * rng.uniform(-1.0, 1.0, size=vr.shape)
    vr[1:-1:4, ::5] = 0.0
    va = va + _ring_mean_free(0.05 * _aspect(radii, nr, nphi) * cs * rng.uniform(-1.0, 1.0, size=va.shape))
    return d0, radii, [sig, vr, va, e]


def floored(lib, d, seed=0, nslabs=1):
    """Patches of 4 rings x 8 columns with Sigma at exactly the density floor, at 1.5 x the floor, at the low-Sigma
    threshold itself and one ulp below and above it; v_r diverging out of the floor patches at 0.5 c_s (the
    transport empties them and clamps Sigma at the floor).  For the ideal EOS also patches with e at 0.3 e_min, at
    e_min and at 3 e_max of the cell."""
    d0, radii, (sig, vr, va, e) = base_state(lib, d)
    rng = np.random.default_rng(seed)
    nr, nphi = sig.shape
    floor = d0.sigma_floor * d0.sigma0
    thr = low_sigma_threshold(d0)
    values = [floor, floor, floor, floor, 1.5 * floor, thr, np.nextafter(thr, 0.0), np.nextafter(thr, np.inf), thr]
    # patch origins: rings 2.. (inside SubStep3's rows), columns spread over the ring, every seam crossed by some
    rings = np.linspace(2, nr - 7, len(values) + 3).astype(int)
    cols = (np.arange(len(values) + 3) * max(9, nphi // (len(values) + 3)) + int(rng.integers(0, 4))) % nphi
    cw = min(8, max(2, nphi // 12))
    patches = []
    for k, v in enumerate(values):
        i0, j0 = int(rings[k]), int(cols[k])
        jj = (j0 + np.arange(cw)) % nphi
        sig[i0:i0 + 4][:, jj] = v
        patches.append((i0, jj))
        if v == floor:   # diverging v_r: out of the patch through its inner and outer faces
            cs = _cs(d0, radii, sig, e)[i0, jj]
            vr[i0][jj] = -0.5 * cs
            vr[i0 + 4][jj] = 0.5 * cs
    if d0.eos == B.EOS_IDEAL:
        emin, emax = e_bounds(d0, sig)
        for k, fac in enumerate(("below", "at", "above")):
            i0, j0 = int(rings[len(values) + k]), int(cols[len(values) + k])
            jj = (j0 + np.arange(cw)) % nphi
            blk = (slice(i0, i0 + 4), jj)
            if fac == "below":
                e[blk] = 0.3 * emin[blk]
            elif fac == "at":
                e[blk] = emin[blk]
            else:
                e[blk] = 3.0 * emax[blk]
        # the low-Sigma patches keep the temperature of the disk around them (pressure drops with Sigma)
    return d0, radii, [sig, vr, va, e]


def shock_edges(nphi):
    """(a, b) column intervals of the dense phase of the square wave: its edges lie on the seams 58/59 and 63/64,
    127/128 where the ring has them, and on the wrap Nphi-1/0."""
    iv = [(59, 64)] if nphi > 70 else []
    if nphi > 200:
        iv.append((128, 160))
    iv.append((nphi - max(4, min(20, nphi // 8)), nphi))
    return iv


def shocked(lib, d, seed=0, nslabs=1):
    """phi square waves: Sigma (and e) x 10 on the intervals of shock_edges, v_phi + 0.5 c_s (times _aspect) on them
    (the ring mean removed again): a compressive jump dv_phi < 0 at every interval's end; a radial step of x 10 across three rings
    with dv_r < 0, and in the multi-slab cases steps on the rings where slabs meet and FCPT_OVERLAP rings to
    either side of them."""
    d0, radii, (sig, vr, va, e) = base_state(lib, d)
    nr, nphi = sig.shape
    mask = np.zeros(nphi, dtype=bool)
    for a, b in shock_edges(nphi):
        mask[a:b] = True
    fac = np.where(mask, 10.0, 1.0)[None, :]
    cs = _cs(d0, radii, sig, e)
    sig *= fac
    e *= fac
    va = va + _ring_mean_free(0.5 * _aspect(radii, nr, nphi) * cs * np.where(mask, 1.0, 0.0)[None, :])
    # radial steps: rings [r0, r0 + 3) dense, their inner face moving out and their outer face in (dv_r < 0)
    starts = [nr // 2 - 1]
    for edge in slab_edges(lib, d0, nslabs):
        starts += [edge - B.OVERLAP, edge, edge + B.OVERLAP]
    csf = np.vstack([cs[:1], 0.5 * (cs[:-1] + cs[1:]), cs[-1:]])
    for r0 in starts:
        r0 = int(min(max(r0, 2), nr - 5))
        sig[r0:r0 + 3] *= 3.0 + 7.0 * (r0 == starts[0])
        if d0.eos == B.EOS_IDEAL:
            e[r0:r0 + 3] *= 3.0
        vr[r0] += 0.3 * csf[r0]
        vr[r0 + 3] -= 0.3 * csf[r0 + 3]
    return d0, radii, [sig, vr, va, e]


def shift_jump(lib, d, seed=0, nslabs=1):
    """The noisy state with v_phi of the inner half of the disk raised by ten cells' worth of azimuthal motion per
    sound-crossing step.  The CFL condition's shear limit keeps the jump within one cell per step (cfl.cpp:207-220);
    the case steps with 4x the CFL step, so that |Nshift[i] - Nshift[i-1]| > 1 at the ring where the jump sits and
    the fused transport must hand over to its fallback kernels."""
    d0, radii, (sig, vr, va, e) = noisy(lib, d, seed, nslabs)
    nr, nphi = sig.shape
    ri = np.asarray(radii[:nr + 1])
    r = 0.5 * (ri[:-1] + ri[1:])
    dx = r * 2 * np.pi / nphi
    cs = _cs(d0, radii, sig, e)[:, 0]
    dt_est = d0.cfl * (ri[1:] - ri[:-1]) / cs     # the sound-speed limit alone: an upper bound of the CFL step
    va[: nr // 2] += (10.0 * dx / dt_est.min())[: nr // 2, None]
    return d0, radii, [sig, vr, va, e]


GENERATORS = {"noisy": noisy, "floored": floored, "shocked": shocked, "shift_jump": shift_jump}


def make_state(lib, d, kind, seed=0, nslabs=1):
    d0, radii, fields = GENERATORS[kind](lib, d, seed, nslabs)
    fields = [np.ascontiguousarray(f) for f in fields]
    assert fields[0].min() > 0 and all(np.isfinite(f).all() for f in fields)
    if d0.eos == B.EOS_IDEAL:
        assert fields[3].min() > 0
    return d0, radii, fields


# ---------------------------------------------------------------------------------------------------------------
# census


def _limiter_zero(q, axis):
    """Cells where van Leer's slope vanishes: the one-sided differences do not have the same sign."""
    if axis == 1:
        dl = q - np.roll(q, 1, axis=1)
        dr = np.roll(q, -1, axis=1) - q
        return int((dl * dr <= 0).sum())
    dl = q[1:-1] - q[:-2]
    dr = q[2:] - q[1:-1]
    return int((dl * dr <= 0).sum())


def census(lib, d, fields, nslabs=1) -> dict:
    """How many cells or faces of an input state reach each branch (the state of the global grid)."""
    sig, vr, va, e = fields
    nr, nphi = sig.shape
    floor = d.sigma_floor * d.sigma0
    thr = low_sigma_threshold(d)
    c = {"sigma_at_floor": int((sig <= floor).sum()),
         "sigma_below_threshold": int(((sig > floor) & (sig < thr)).sum()),
         "vr_pos": int((vr[1:-1] > 0).sum()), "vr_neg": int((vr[1:-1] < 0).sum()),
         "vr_zero": int((vr[1:-1] == 0).sum()),
         "limiter_zero_r": _limiter_zero(sig, 0), "limiter_zero_phi": _limiter_zero(sig, 1),
         "compressive_r": int((vr[2:-1] - vr[1:-2] < 0).sum()),
         "compressive_phi": int((np.roll(va, -1, axis=1) - va < 0).sum())}
    if d.eos == B.EOS_IDEAL:
        emin, emax = e_bounds(d, sig)
        c["e_below_min"] = int((e < emin).sum())
        c["e_at_min"] = int((e == emin).sum())
        c["e_above_max"] = int((e > emax).sum())

    def jump(x, y):
        return (x / y > 1.0 + JUMP) | (y / x > 1.0 + JUMP)

    for a, b in SEAMS + ((nphi - 1, 0),):
        if b < nphi:
            name = "seam_wrap" if b == 0 else f"seam_{a}_{b}"
            c[name] = int(jump(sig[:, a], sig[:, b]).sum())
    for k, edge in enumerate(slab_edges(lib, d, nslabs)):
        for off in (-B.OVERLAP, 0, B.OVERLAP):
            i = edge + off
            c[f"slab{k}_ring_{off:+d}"] = int(jump(sig[i - 1], sig[i]).sum())
    return c


def post_census(d, before, after) -> dict:
    """What one oracle step did with a state (`before` the input, `after` the output, global grids with Q+ and Q-
    for the ideal EOS): cells with Sigma clamped at the floor, e clamped at e_min and at e_max, and cells of
    SubStep3's rows that took the low-Sigma branch (Q- set to Q+; Sigma does not change before SubStep3)."""
    floor = d.sigma_floor * d.sigma0
    c = {"sigma_clamped": int((after["sigma"] == floor).sum())}
    if d.eos == B.EOS_IDEAL:
        emin, emax = e_bounds(d, after["sigma"])
        e = after["energy"]
        c["e_clamped_min"] = int((np.abs(e / emin - 1.0) < 1e-13).sum())
        c["e_clamped_max"] = int((np.abs(e / emax - 1.0) < 1e-13).sum())
        rows = slice(1, before["sigma"].shape[0] - 1)
        low = before["sigma"][rows] < low_sigma_threshold(d)
        took = after["qminus"][rows] == after["qplus"][rows]
        c["low_sigma_branch"] = int((low & took).sum())
    return c


# ---------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_rough_states.py: (id, nr, nphi, physics, kind, options)
# options: slabs (radial slabs of the HIP run), av, leapfrog, massflow, dt_scale (steps of a multiple of the CFL step),
#          src: "march" | "fused" (the three out-of-place kernels of rings the march does not take), tr: "fused" | "two" | "fallback", cfl: "rings" | "cells" | None (not asserted)


def _cfl_path(nphi, physics):
    """The CFL kernels of fcpt_plan.cpp:cfl_by_rings: one block per ring (k_cfl_rings) for even rings of 128 .. 1024
    CFL_MAXP = 8192 cells, else k_ring_mean + k_cfl_cells.  The ideal EOS qualifies through its lazily derived
    quantities, which the marching source kernel implies (Nphi >= 128, fcpt_context.hip); no case here sets
    StabilizeViscosity 2, which would also exclude it."""
    return "rings" if nphi % 2 == 0 and 128 <= nphi <= 8192 else "cells"


def _case(nr, nphi, physics, kind, **opt):
    opt.setdefault("slabs", 1)
    opt.setdefault("src", "march" if nphi >= 128 else "fused")
    opt.setdefault("tr", "fused" if nphi >= 256 else "two")
    opt.setdefault("cfl", _cfl_path(nphi, physics))
    tag = "".join(f"_{k}" for k in ("av", "leapfrog", "massflow") if k in opt and opt[k] not in (False, "TW"))
    tag = tag.replace("_av", "_sn").replace("_leapfrog", "_lf")
    sl = f"_{opt['slabs']}slabs" if opt["slabs"] > 1 else ""
    return (f"{kind}_{physics}_{nr}x{nphi}{tag}{sl}", nr, nphi, physics, kind, opt)


CASES = (
    # every side of the size switches of kernels/launch.h, isothermal and ideal EOS, three kinds of state
    [_case(32, n, p, k) for n in (96, 128, 256, 320) for p in ("iso", "visc") for k in ("noisy", "floored", "shocked")]
    # cooling: the low-Sigma branch needs tau_eff > 0 (surface cooling); beta cooling towards the floor
    + [_case(32, n, p, "floored") for n in (128, 320) for p in ("cool_const", "cool_lin")]
    + [_case(32, 96, "cool_lin", "floored"), _case(32, 128, "beta", "noisy"), _case(32, 320, "beta", "floored")]
    # odd rings (CFL by cells), the 512-thread CFL form, wide rings, beyond 1024 CFL_MAXP (k_ring_mean)
    + [_case(32, 263, "iso", "shocked"), _case(32, 263, "visc", "floored"),
       _case(24, 2050, "iso", "noisy"),
       _case(24, 6144, "visc", "floored"), _case(24, 8194, "visc", "floored")]
    # (on rings of 2050 cells and more, only these states: a cell there is 20 .. 100 times longer than wide, and
    # from the shocked state, and from the noisy or isothermal floored ones on the widest rings, the oracle itself
    # amplifies 1e-15 noise by 2e3 .. 4e7 within two steps -- beyond the growth-based bar, or with time steps
    # that differ by 2.5e-12 after the first step; at 48 rings the 2050 states fare no better)
    # SN artificial viscosity, leapfrog
    + [_case(32, 320, "iso", "shocked", av="SN"), _case(32, 128, "visc", "shocked", av="SN"),
       _case(32, 96, "visc", "shocked", av="SN"),
       _case(32, 320, "visc", "floored", leapfrog=True), _case(32, 128, "iso", "shocked", leapfrog=True),
       _case(32, 96, "visc", "shocked", leapfrog=True)]
    # three slabs: steps on the rings where they meet and FCPT_OVERLAP rings away
    + [_case(48, 320, "iso", "shocked", slabs=3), _case(48, 320, "visc", "floored", slabs=3),
       _case(48, 128, "visc", "shocked", slabs=3), _case(48, 96, "iso", "shocked", slabs=3)]
    # WriteMassFlow; a ring-to-ring jump of the FARGO shift (the fused kernel hands over to the fallback)
    + [_case(32, 320, "iso", "noisy", massflow=True), _case(32, 128, "visc", "floored", massflow=True),
       _case(32, 320, "iso", "shift_jump", tr="fallback", dt_scale=4.0)]
)

# branches each kind of state must reach (>= MIN_COUNT cells or faces); "ideal:" only for the ideal EOS, "uncooled:"
# only for the ideal EOS without cooling
INTENDED = {
    "noisy": ["vr_pos", "vr_neg", "vr_zero", "limiter_zero_r", "limiter_zero_phi", "compressive_r", "compressive_phi"],
    "floored": ["sigma_at_floor", "sigma_below_threshold", "ideal:e_below_min", "ideal:e_at_min", "ideal:e_above_max"],
    "shocked": ["compressive_r", "compressive_phi", "limiter_zero_phi", "seams", "slabs"],
    "shift_jump": ["vr_pos", "vr_neg", "vr_zero"],
}
POST_INTENDED = {
    # (cooling moves a cell beyond the ceiling or below the floor back inside the range within the step)
    "floored": ["sigma_clamped", "uncooled:e_clamped_min", "uncooled:e_clamped_max", "ideal:low_sigma_branch"],
}
