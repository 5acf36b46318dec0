"""Exact symmetries of the gas step, as transforms of a run's inputs and results: the mirror phi -> -phi, the rotation
by whole cells, and two rescalings by powers of two (Sigma and e together; all lengths by 4).  The equations and the
staggered scheme obey them without any restatement of the scheme: a step from the transformed state, transformed back,
is the step from the state itself -- at rounding level for the mirror and the rotation (sums meet the columns in another
order), bit for bit for the rescalings (a power of two changes no mantissa).  A misread azimuthal index or a one-sided
difference taken on the wrong side breaks the mirror by 8e-2 .. 1.3 (one-token edits of the oracle, measured; DESIGN.md
section 3) -- not the rotation, under which a uniformly wrong index is covariant: the rotation is for seams and the
wrap --, and a constant that should scale breaks the rescalings; in the oracle and in the kernels alike, where a parity
test compares two copies of the same reading.

Plain numpy, no GPU.  Cell centres lie at phi_j = j dphi (the bodies' potential is evaluated there); v_phi sits on the
face between the columns j-1 and j, at (j - 1/2) dphi; v_r and MASSFLOW sit on radial faces at the cells' azimuth.

  mirror          cell-centred and radial-face grids: q'[i, j] = q[i, (-j) mod Nphi]; v_phi'[i, j] = -v_phi[i, (1-j) mod Nphi];
                  bodies (x, -y), indirect term (a_x, -a_y), omega_frame -> -omega_frame.  A mirrored disk is retrograde.
  rotate(k)       np.roll of every grid by k columns; bodies and indirect term turned by k dphi.
  scale_sigma(p)  Sigma, e, Q+, Q-, MASSFLOW and sigma0 times 2^p; velocities and dt unchanged.
  scale_length(s) s a power of 4: lengths x s, velocities x s^-1/2, times x s^3/2 (G M fixed): e x 1/s, the temperature
                  floor and ceiling x 1/s, omega_frame x s^-3/2, a constant nu x s^1/2, rmin, rmax and
                  damping_time_radius_outer x s, first_dt and monitor_timestep x s^3/2, the bodies' positions and cubic
                  smoothing radii x s, the indirect term x s^-2, Q+- x s^-5/2, MASSFLOW x s^2.  The radii are fcpt_radii of
                  the scaled descriptor.

What is NOT symmetric, and therefore refused by `check` (with the reason):
  * The CFL reduction is not mirror symmetric by construction: condition_cfl joins a cell's sound speed with v_r and the
    v_phi residual of the cell's LOWER faces only (cfl.cpp:222-330), so the mirrored disk takes another step length, at
    truncation level.  A mirror (and, for the sake of one rule, a rotation) comparison steps both orientations with the
    same forced step lengths (parity_runs.run_state, forced_dts).
  * Boundary conditions that build a prograde Keplerian value are not mirror covariant: BC_KEPLERIAN for v_phi writes
    +v_K - r Omega into the ghost ring whatever the disk's sense of rotation (the composites of fargocpt_amd/setups.py
    choose it), and the initial-condition generators do the same -- mirror runs upload their fields.  BC_KEPLERIAN for
    v_r is not part of the census either.
  * Terms that are not homogeneous by their physics: SubStep3 carries the radiation energy (~ e^3 / Sigma^4), so with any
    Q+ or Q- (viscous heating, surface or beta cooling, irradiation) the ideal-EOS energy is not scale-free.  The two
    rescalings take the isothermal EOS, or the ideal one with heating_viscous = 0 and no cooling.  The dissipation of
    the artificial viscosity stays in: it is bilinear in the velocities and homogeneous.
"""
from __future__ import annotations

import math

import numpy as np

from fargocpt_amd import binding as B, setups
from tests import rough_states as R

CELL = ("sigma", "energy", "qplus", "qminus", "temperature")
RFACE = ("vrad", "massflow")
PHIFACE = ("vazi",)


def _kind(name):
    if name in CELL:
        return "cell"
    if name in RFACE:
        return "rface"
    assert name in PHIFACE, name
    return "phiface"


def mirror_cells(q):
    """q'[i, j] = q[i, (-j) mod Nphi] (its own inverse)"""
    return np.ascontiguousarray(np.roll(q[:, ::-1], 1, axis=1))


def mirror_vphi(v):
    """v'[i, j] = -v[i, (1-j) mod Nphi] (its own inverse): the face (j - 1/2) dphi goes to ((1-j) - 1/2) dphi"""
    return np.ascontiguousarray(-np.roll(v[:, ::-1], 2, axis=1))


class Transform:
    """One symmetry: `desc`, `fields`, `bodies` transform a run's inputs, `grid(name, q)` one grid by its name,
    `back(out)` a run's result grids to the untransformed frame, `dt_back` its step lengths.  `exact`: whether the
    symmetry holds bit for bit.  `forced`: whether both orientations step with the same forced step lengths."""
    exact = False
    forced = True
    name = "identity"

    def desc(self, lib, d):
        """-> (descriptor, radii) of the transformed run"""
        return d.copy(), lib.radii(d)

    def grid(self, name, q):
        return q

    def grid_back(self, name, q):
        return q

    def fields(self, fields):
        return [np.ascontiguousarray(self.grid(n, f)) for n, f in zip(("sigma", "vrad", "vazi", "energy"), fields)]

    def back(self, out):
        return {n: np.ascontiguousarray(self.grid_back(n, q)) for n, q in out.items()}

    def bodies(self, bodies, d=None):
        """the bodies of the transformed run; `d`: the descriptor (the rotation's angle is k cells of its ring)"""
        return bodies

    def dt_back(self, dt):
        return dt

    def dt(self, dt):
        return dt

    def sentinel(self, q):
        return self.grid("qplus", q)

    def check(self, d):
        """AssertionError with the reason where the descriptor's options are not covariant under this transform."""


def _no_mean_under_reference(name, d):
    """DAMP_MEAN keeps each damped ring's mean in column 0 of the quantity's reference grid (damping.cpp:580-585 of the
    reference, and so the oracle and the kernels); BC_REFERENCE on the same side then copies that column into the ghost ring
    as if it were the initial value.  Column 0 is a place on the grid, so the pair is neither mirror nor rotation covariant
    (measured on shocked iso 32 x 96: 6e-3 and 0.75); the rescalings hold it bit for bit."""
    pairs = (("v_r", d.damp_vrad, d.bc_vrad), ("v_phi", d.damp_vaz, d.bc_vaz), ("Sigma", d.damp_sigma, d.bc_sigma),
             ("e", d.damp_energy, d.bc_energy))
    for q, damp, bc in pairs:
        for side, where in enumerate(("inner", "outer")):
            assert not (d.damping and damp[side] == B.DAMP_MEAN and bc[side] == B.BC_REFERENCE), (
                f"{name}: {q} is damped towards the ring mean and has BC_REFERENCE on the {where} side: the mean lives in "
                f"column 0 of the reference grid, which the boundary condition then reads as a reference value")


class Mirror(Transform):
    name = "mirror"

    def desc(self, lib, d):
        self.check(d)
        d = d.copy()
        d.omega_frame = -d.omega_frame
        return d, lib.radii(d)

    def grid(self, name, q):
        return mirror_vphi(q) if _kind(name) == "phiface" else mirror_cells(q)

    grid_back = grid

    def bodies(self, bodies, d=None):
        x, y, m, rsm, (ax, ay) = bodies
        return list(x), [-v for v in y], list(m), list(rsm), (ax, -ay)

    def check(self, d):
        _no_mean_under_reference(self.name, d)
        for side, where in enumerate(("inner", "outer")):
            assert d.bc_vaz[side] != B.BC_KEPLERIAN, (
                f"mirror: the {where} v_phi boundary is BC_KEPLERIAN, which writes the prograde +v_K - r Omega into the ghost "
                f"ring whatever the disk's sense of rotation: not mirror covariant (the ghost rings differ by O(1))")
            assert d.bc_vrad[side] != B.BC_KEPLERIAN, (
                f"mirror: the {where} v_r boundary is BC_KEPLERIAN, which the census of tests/test_symmetries_oracle.py "
                f"does not cover")


class Rotate(Transform):
    def __init__(self, k):
        self.k = int(k)
        self.name = f"rotate{self.k}"

    def desc(self, lib, d):
        self.check(d)
        return d.copy(), lib.radii(d)

    def check(self, d):
        _no_mean_under_reference(self.name, d)

    def grid(self, name, q):
        return np.ascontiguousarray(np.roll(q, self.k, axis=1))

    def grid_back(self, name, q):
        return np.ascontiguousarray(np.roll(q, -self.k, axis=1))

    def bodies(self, bodies, d):
        x, y, m, rsm, (ax, ay) = bodies
        angle = self.k * 2 * math.pi / d.nphi
        c, s = math.cos(angle), math.sin(angle)
        return ([c * u - s * v for u, v in zip(x, y)], [s * u + c * v for u, v in zip(x, y)], list(m), list(rsm),
                (c * ax - s * ay, s * ax + c * ay))


def _no_heating_cooling(name, d):
    if d.eos == B.EOS_IDEAL:
        assert not (d.heating_viscous or d.cooling_surface or d.cooling_beta), (
            f"{name}: with Q+ or Q- SubStep3 carries the radiation energy (~ e^3 / Sigma^4), which is not homogeneous: the "
            f"ideal-EOS energy is scale-free only with heating_viscous = 0 and no cooling")


class ScaleSigma(Transform):
    exact = True
    forced = False

    def __init__(self, p):
        self.f = 2.0 ** int(p)
        self.name = f"sigma_2^{int(p)}"

    def desc(self, lib, d):
        self.check(d)
        d = d.copy()
        d.sigma0 *= self.f
        return d, lib.radii(d)

    def grid(self, name, q):
        return q * self.f if name in ("sigma", "energy", "qplus", "qminus", "massflow") else q

    def grid_back(self, name, q):
        return q / self.f if name in ("sigma", "energy", "qplus", "qminus", "massflow") else q

    def check(self, d):
        _no_heating_cooling(self.name, d)


class ScaleLength(Transform):
    exact = True
    forced = False

    def __init__(self, s=4):
        self.s = float(s)
        self.rv = math.sqrt(self.s)          # 1 / the factor of velocities
        assert self.rv == int(self.rv) and self.rv in (2.0, 4.0, 8.0), "lengths scale by a power of 4 (velocities by a power of 2)"
        self.t = self.s * self.rv            # the factor of times
        self.name = f"length_x{int(s)}"
        self.factors = {"sigma": 1.0, "vrad": 1.0 / self.rv, "vazi": 1.0 / self.rv, "energy": 1.0 / self.s,
                        "temperature": 1.0 / self.s, "qplus": 1.0 / (self.s * self.t), "qminus": 1.0 / (self.s * self.t),
                        "massflow": self.s * self.s}

    def desc(self, lib, d):
        self.check(d)
        d = d.copy()
        d.rmin *= self.s
        d.rmax *= self.s
        d.damping_time_radius_outer *= self.s
        d.omega_frame /= self.t
        d.minimum_temperature /= self.s
        d.maximum_temperature /= self.s
        d.constant_viscosity *= self.s / self.rv
        d.first_dt *= self.t
        d.monitor_timestep *= self.t
        return d, lib.radii(d)

    def grid(self, name, q):
        return q * self.factors[name]

    def grid_back(self, name, q):
        return q / self.factors[name]

    def bodies(self, bodies, d=None):
        x, y, m, rsm, (ax, ay) = bodies
        s = self.s
        return [s * v for v in x], [s * v for v in y], list(m), [s * v for v in rsm], (ax / (s * s), ay / (s * s))

    def dt_back(self, dt):
        return dt / self.t

    def dt(self, dt):
        return dt * self.t

    def check(self, d):
        _no_heating_cooling(self.name, d)


def transform(spec) -> Transform:
    """"mirror" | ("rotate", k) | ("sigma", p) | ("length", s)"""
    if spec == "mirror":
        return Mirror()
    kind, arg = spec
    return {"rotate": Rotate, "sigma": ScaleSigma, "length": ScaleLength}[kind](arg)


# ---------------------------------------------------------------------------------------------------------------
# cases: a rough state (tests/rough_states.py) with a planet off the axis, boundary conditions that are covariant,
# and the transforms the case takes

PLANET_ANGLE = 0.7
INDIRECT = (1.0e-4, -2.0e-4)
ROT = 37
ALL4 = ("mirror", ("rotate", ROT), ("sigma", 5), ("sigma", -30), ("length", 4))
MR = ("mirror", ("rotate", ROT))
RSL = ALL4[1:]     # all but the mirror: the Keplerian boundary values are prograde by construction

BCS = {
    # name: (v_r, v_phi, Sigma and e) of both sides
    "zerogradient": (B.BC_ZEROGRADIENT, B.BC_ZEROGRADIENT, B.BC_ZEROGRADIENT),
    "reflecting": (B.BC_REFLECTING, B.BC_ZEROGRADIENT, B.BC_ZEROGRADIENT),
    "reference": (B.BC_REFERENCE, B.BC_REFERENCE, B.BC_REFERENCE),
    "outflow_zeroshear": (B.BC_OUTFLOW, B.BC_ZEROSHEAR, B.BC_ZEROGRADIENT),
    "keplerian": (B.BC_REFLECTING, B.BC_KEPLERIAN, B.BC_ZEROGRADIENT),     # (the composites of setups.py: refused by the mirror)
}
DAMPS = {"reference": B.DAMP_REFERENCE, "zero": B.DAMP_ZERO, "mean": B.DAMP_MEAN}


def jupiter(angle=PLANET_ANGLE, indirect=INDIRECT):
    """(x, y, m, cubic smoothing radii, indirect term): the star and a Jupiter on the unit circle at `angle`, Klahr & Kley
    smoothing inside 1/16, and an indirect term that points nowhere special."""
    return ([0.0, math.cos(angle)], [0.0, math.sin(angle)], [1.0, setups.M_JUP], [0.0, 0.0625], tuple(indirect))


def _case(name, nr, nphi, physics, kind, transforms, **opt):
    opt.setdefault("slabs", 1)
    opt.setdefault("steps", 3)
    opt.setdefault("bc", "reflecting")
    opt.setdefault("damp", "reference")
    opt.setdefault("src", "march" if nphi >= 128 else "fused")
    opt.setdefault("tr", "fused" if nphi >= 256 else "two")
    opt.setdefault("cfl", R._cfl_path(nphi, physics))
    return (name, nr, nphi, physics, kind, tuple(transforms), opt)


def case_desc(lib, case) -> B.Desc:
    """rough_states.case_desc with the options of a symmetry case.  physics "ideal0": the ideal EOS with
    heating_viscous = 0 (no Q+ but the artificial viscosity's dissipation, no Q-): the scale-free ideal gas."""
    name, nr, nphi, physics, kind, transforms, opt = case
    d = R.case_desc(lib, nr, nphi, "visc" if physics == "ideal0" else physics, kind, av=opt.get("av", "TW"),
                    leapfrog=opt.get("leapfrog", False), massflow=opt.get("massflow", False))
    if physics == "ideal0":
        d.heating_viscous = 0
    vr, va, sc = BCS[opt["bc"]]
    for side in (0, 1):
        d.bc_vrad[side], d.bc_vaz[side] = vr, va
        d.bc_sigma[side] = d.bc_energy[side] = sc
    for arr in (d.damp_vrad, d.damp_vaz, d.damp_sigma, d.damp_energy):
        arr[0] = arr[1] = DAMPS[opt["damp"]]
    if opt.get("limiter") == "mc":
        d.flux_limiter = B.LIMITER_MC
    if opt.get("fast") is False:
        d.fast_transport = 0
        d.cfl = 0.4
    if opt.get("accel"):
        d.body_force_from_potential = 0
    if opt.get("spacing") == "arithmetic":
        d.radial_spacing = B.SPACING_ARITHMETIC
    elif opt.get("spacing") == "exponential":
        d.radial_spacing = B.SPACING_EXPONENTIAL
        d.exponential_cell_size_factor = 2.0     # (the default has no root on this grid, see test_gpu_particles_parity.py)
    if opt.get("const_nu"):
        d.viscous_alpha, d.constant_viscosity = 0.0, opt["const_nu"]
    if opt.get("stab"):
        d.stabilize_viscosity, d.radial_viscosity_factor = opt["stab"], opt.get("rvf", 1.0)
    return d


def build(lib, case):
    """-> (descriptor of the global grid, radii, fields, bodies) of a case, untransformed"""
    name, nr, nphi, physics, kind, transforms, opt = case
    d0, radii, fields = R.make_state(lib, case_desc(lib, case), kind, nslabs=opt["slabs"])
    return d0, radii, fields, jupiter()


def transformed(lib, t: Transform, d0, radii, fields, bodies):
    """-> (descriptor, radii, fields, bodies) of the transformed run"""
    d1, radii1 = t.desc(lib, d0)
    return d1, radii1, t.fields(fields), t.bodies(bodies, d0)


# rings of 48 cells: a block of the out-of-place kernels is narrower than a wavefront there (their ROWU = false instances);
# the keywords are those of the 96-column twins.  In both tables below.
NARROW_48 = [
    _case("noisy_iso_32x48_stab1", 32, 48, "iso", "noisy", ALL4, stab=1, const_nu=1.0e-2, dt_scale=3.0),
    _case("shocked_visc_32x48_stab1", 32, 48, "visc", "shocked", MR, stab=1, const_nu=1.0e-2, dt_scale=3.0),
    _case("noisy_iso_32x48_stab2_rvf", 32, 48, "iso", "noisy", ALL4, stab=2, rvf=2.5, const_nu=1.0e-2),
    _case("noisy_ideal0_32x48_accel", 32, 48, "ideal0", "noisy", ALL4, accel=True, bc="outflow_zeroshear", damp="mean"),
    _case("noisy_iso_32x48_accel_lf", 32, 48, "iso", "noisy", ALL4, accel=True, leapfrog=True),
]

# (id, nr, nphi, physics, kind, transforms, options) -- the census of tests/test_symmetries_oracle.py, all at 32 x 96
# (one at 32 x 130, the three slabs at 48 x 96): both EOS, TW and SN, leapfrog, both limiters, standard transport, viscous
# heating with Lin surface cooling and beta cooling (mirror and rotation only), every covariant boundary condition and
# damping target, three slabs, accelerations instead of the potential, the shift jump at 4 x the CFL step
ORACLE_CASES = [
    _case("noisy_iso", 32, 96, "iso", "noisy", ALL4),
    _case("shocked_iso", 32, 96, "iso", "shocked", ALL4),
    _case("floored_iso", 32, 96, "iso", "floored", ALL4),
    _case("noisy_ideal0", 32, 96, "ideal0", "noisy", ALL4),
    _case("shocked_ideal0_sn", 32, 96, "ideal0", "shocked", ALL4, av="SN"),
    _case("noisy_visc", 32, 96, "visc", "noisy", MR),
    _case("shocked_visc", 32, 96, "visc", "shocked", MR),
    _case("noisy_cool_lin", 32, 96, "cool_lin", "noisy", MR),
    _case("shocked_cool_lin", 32, 96, "cool_lin", "shocked", MR),
    _case("noisy_beta", 32, 96, "beta", "noisy", MR),
    _case("shocked_visc_sn_130", 32, 130, "visc", "shocked", MR, av="SN"),
    _case("shocked_iso_sn", 32, 96, "iso", "shocked", ALL4, av="SN"),
    _case("noisy_iso_lf", 32, 96, "iso", "noisy", ALL4, leapfrog=True),
    _case("shocked_visc_lf", 32, 96, "visc", "shocked", MR, leapfrog=True),
    _case("noisy_iso_mc", 32, 96, "iso", "noisy", ALL4, limiter="mc"),
    _case("noisy_ideal0_mc", 32, 96, "ideal0", "noisy", ALL4, limiter="mc"),
    _case("noisy_iso_standard", 32, 96, "iso", "noisy", ALL4, fast=False),
    _case("noisy_iso_zerogradient", 32, 96, "iso", "noisy", ALL4, bc="zerogradient", damp="zero"),
    _case("noisy_visc_outflow_zeroshear", 32, 96, "visc", "noisy", MR, bc="outflow_zeroshear", damp="mean"),
    _case("noisy_ideal0_outflow_zeroshear", 32, 96, "ideal0", "noisy", ALL4, bc="outflow_zeroshear", damp="mean"),
    _case("shocked_iso_reference", 32, 96, "iso", "shocked", ALL4, bc="reference"),
    _case("noisy_ideal0_reference", 32, 96, "ideal0", "noisy", ALL4, bc="reference", damp="zero"),
    _case("shocked_iso_3slabs", 48, 96, "iso", "shocked", ALL4, slabs=3),
    _case("noisy_visc_3slabs", 48, 96, "visc", "noisy", MR, slabs=3),
    _case("noisy_iso_accel", 32, 96, "iso", "noisy", ALL4, accel=True),
    _case("noisy_visc_accel", 32, 96, "visc", "noisy", MR, accel=True),
    _case("noisy_iso_arithmetic_constnu", 32, 96, "iso", "noisy", ALL4, spacing="arithmetic", const_nu=1.0e-5),
    _case("noisy_iso_massflow", 32, 96, "iso", "noisy", ALL4, massflow=True),
    _case("noisy_iso_keplerian", 32, 96, "iso", "noisy", RSL, bc="keplerian"),
    _case("noisy_iso_exponential", 32, 96, "iso", "noisy", ALL4, spacing="exponential"),
    # StabilizeViscosity.  The correction 1 / (max(1 + dt c, 0) - dt c) of the viscous update (1) is exactly 1 unless
    # dt c < -1, and the bound -cfl / c on the step (2) binds only where it is shorter than the CFL step: with alpha = 1e-3
    # dt c stays at -5e-3 and the bound at 4, a hundred times the step -- the factors are computed and inert.  nu = 1e-2 at
    # 3 x the CFL step gives dt c = -1.8 (about 900 of 3072 faces below -1); nu = 1e-2 with a radial factor of 2.5 makes the
    # bound a third of the CFL step from the second step on (the factors are those of the step before: none in the first).
    # stabilizer_acts asserts both against the same state without the option.
    _case("noisy_iso_stab1", 32, 96, "iso", "noisy", ALL4, stab=1, const_nu=1.0e-2, dt_scale=3.0),
    _case("shocked_visc_stab1", 32, 96, "visc", "shocked", MR, stab=1, const_nu=1.0e-2, dt_scale=3.0),
    _case("noisy_iso_stab2_rvf", 32, 96, "iso", "noisy", ALL4, stab=2, rvf=2.5, const_nu=1.0e-2),
    # (with a radial factor of 2.5 the radial correction factor is the binding one; with 0.25 the azimuthal one, at 0.91 of
    # the CFL step: an index misread in either is seen only where that factor sets the step)
    _case("noisy_iso_stab2_rvf025", 32, 96, "iso", "noisy", ALL4, stab=2, rvf=0.25, const_nu=1.0e-2),
    # (three steps of this state amplify 1e-15 noise to 2.6e-10, two to 9.4e-11, beyond NOISE_CAP: one step, 1.3e-14 -- the
    # step in which |Nshift[i] - Nshift[i-1]| > 1; on rings of 320 cells two steps stay at 3.3e-14)
    _case("shift_jump_iso_4cfl", 32, 96, "iso", "shift_jump", ("mirror",), dt_scale=4.0, steps=1),
    _case("shift_jump_iso_32x320_4cfl", 32, 320, "iso", "shift_jump", ("mirror",), dt_scale=4.0, steps=2),
] + NARROW_48

# the cases of tests/test_gpu_symmetries.py: the smallest rings at which each kernel form still has its seams
#   48, 96: the three out-of-place source kernels (48: blocks narrower than a wavefront), two-kernel transport;  130: marching source with a ragged third segment, two-kernel transport;
#   256: fused transport, CFL by rings;  263: odd fused rings, CFL by cells;  320: six source segments and six fused tiles
# one case of each marching form steps on explicit ragged chunk lists (set_transport_chunks, set_source_chunks)
GPU_CASES = [
    _case("noisy_iso_32x96", 32, 96, "iso", "noisy", ALL4),
    _case("shocked_visc_32x96", 32, 96, "visc", "shocked", MR),
    _case("noisy_ideal0_32x96_accel", 32, 96, "ideal0", "noisy", ALL4, accel=True, bc="outflow_zeroshear", damp="mean"),
    _case("shocked_iso_32x130_sn", 32, 130, "iso", "shocked", ALL4, av="SN"),
    _case("noisy_cool_lin_32x130", 32, 130, "cool_lin", "noisy", MR),
    _case("noisy_ideal0_32x130_chunks", 32, 130, "ideal0", "noisy", ALL4, source_chunks=[5, 3, 14, 4], bc="reference", damp="zero"),
    _case("noisy_iso_32x256", 32, 256, "iso", "noisy", ALL4),
    _case("shocked_visc_32x256", 32, 256, "visc", "shocked", MR, chunks=[7, 3, 9], source_chunks=[4, 11, 3]),
    _case("floored_iso_32x256_mc", 32, 256, "iso", "floored", ALL4, limiter="mc", steps=2),
    _case("shocked_iso_32x263", 32, 263, "iso", "shocked", ALL4),
    _case("noisy_beta_32x263", 32, 263, "beta", "noisy", MR, chunks=[4, 100], source_chunks=[3, 3, 40]),
    _case("noisy_ideal0_32x263_lf", 32, 263, "ideal0", "noisy", ALL4, leapfrog=True, steps=2),
    _case("noisy_iso_32x320_chunks", 32, 320, "iso", "noisy", ALL4, chunks=[5, 3, 7], source_chunks=[3, 9, 4, 3], massflow=True),
    _case("shocked_visc_32x320_sn", 32, 320, "visc", "shocked", MR, av="SN"),
    _case("noisy_ideal0_32x320", 32, 320, "ideal0", "noisy", ALL4, bc="zerogradient"),
    _case("shocked_iso_48x320_3slabs", 48, 320, "iso", "shocked", ALL4, slabs=3, steps=2),
    _case("noisy_visc_48x130_3slabs", 48, 130, "visc", "noisy", MR, slabs=3, steps=2),
    _case("shift_jump_iso_32x320_4cfl", 32, 320, "iso", "shift_jump", ("mirror",), dt_scale=4.0, steps=2, tr="fallback"),
    # arithmetic radii with a constant nu (the per-ring tables and nu under lengths x 4); standard transport (the kernels'
    # own branches for fast_transport = 0) on the two-kernel and on the fused path; StabilizeViscosity
    _case("noisy_iso_32x96_arithmetic_constnu", 32, 96, "iso", "noisy", ALL4, spacing="arithmetic", const_nu=1.0e-5),
    _case("noisy_iso_32x256_arithmetic_constnu", 32, 256, "iso", "noisy", ALL4, spacing="arithmetic", const_nu=1.0e-5),
    _case("noisy_iso_32x96_standard", 32, 96, "iso", "noisy", ALL4, fast=False),
    _case("noisy_iso_32x256_standard", 32, 256, "iso", "noisy", ALL4, fast=False),
    _case("noisy_iso_32x263_keplerian", 32, 263, "iso", "noisy", RSL, bc="keplerian"),
    _case("noisy_iso_32x130_exponential", 32, 130, "iso", "noisy", ALL4, spacing="exponential"),
    _case("noisy_iso_32x130_stab1", 32, 130, "iso", "noisy", ALL4, stab=1, const_nu=1.0e-2, dt_scale=3.0),
    _case("noisy_iso_32x130_stab2_rvf", 32, 130, "iso", "noisy", ALL4, stab=2, rvf=2.5, const_nu=1.0e-2, cfl="cells"),
    _case("noisy_iso_40x130_stab2_rvf025", 40, 130, "iso", "noisy", ALL4, stab=2, rvf=0.25, const_nu=1.0e-2, cfl="cells"),
    # StabilizeViscosity and the accelerations on rings the march does not take: k_visc_factors ahead of k_visc_fused<CORR>,
    # k_src_fused<ACC> (the ORACLE_CASES of these names)
    _case("noisy_iso_stab1", 32, 96, "iso", "noisy", ALL4, stab=1, const_nu=1.0e-2, dt_scale=3.0),
    _case("shocked_visc_stab1", 32, 96, "visc", "shocked", MR, stab=1, const_nu=1.0e-2, dt_scale=3.0),
    _case("noisy_iso_stab2_rvf", 32, 96, "iso", "noisy", ALL4, stab=2, rvf=2.5, const_nu=1.0e-2),
    _case("noisy_iso_stab2_rvf025", 32, 96, "iso", "noisy", ALL4, stab=2, rvf=0.25, const_nu=1.0e-2),
] + NARROW_48

# the cases that also go through fcpt_run_steps, with graph replay: (id of GPU_CASES, transforms)
DEVICE_LOOP = [
    ("noisy_iso_32x256", ("mirror", ("sigma", 5), ("length", 4))),
    ("shocked_visc_32x96", ("mirror",)),
    ("noisy_ideal0_32x96_accel", (("rotate", ROT), ("sigma", -30), ("length", 4))),
]
GPU_BY_NAME = {c[0]: c for c in GPU_CASES}


# ---------------------------------------------------------------------------------------------------------------
# runs and bars shared by the oracle's census and the GPU test

NOISE = 1.0e-15
BAR_FLOOR = 1.0e-13     # no bar below this
BAR_MARGIN = 10.0       # bar = BAR_MARGIN x the oracle's response to NOISE: one noise realisation underestimates the
#                         spread, and tree sums and contractions meet the columns in another order in the two orientations
NOISE_CAP = 1.0e-12     # the census holds every mirror / rotation case's response below this: no bar above 1e-11


def oracle_base(oracle, case, state, nslabs=1):
    """The oracle from the untransformed state at its own CFL steps -> (grids, dt history)"""
    from tests.parity_runs import run_state
    d0, radii, fields, bodies = state
    opt = case[6]
    b, dts, _, _ = run_state(oracle, d0, radii, fields, nslabs, opt["steps"], "host", dt_scale=opt.get("dt_scale", 1.0),
                             bodies=bodies)
    return b, dts


def noise_response(oracle, case, state, dts, b=None):
    """The oracle's response to cell-wise NOISE on the untransformed state over the same steps and step lengths, in the
    measure of parity_runs.errors"""
    from tests.parity_runs import noise_growth
    d0, radii, fields, bodies = state
    return NOISE * noise_growth(oracle, d0, radii, fields, case[6]["steps"], b=b, bodies=bodies, forced_dts=list(dts))


def stabilizer_acts(oracle, case, state, base, dts):
    """A StabilizeViscosity case must let the option act (AssertionError otherwise): against the oracle from the same state
    and descriptor with stabilize_viscosity = 0, at the same multiple of the CFL step,
      1: the first CFL step is the same (the option is not in the CFL reduction) and the velocities differ after it by more
         than 1e-6 of the sound speed somewhere: faces with dt c < -1, where the correction is not 1;
      2: the first step is the same (the factors are those of the step before) and every later one is shorter than the
         twin's: the bound -cfl / c sets the step.  (The second step starts from the same state in both runs, so there only
         the bound can shorten it; the tests that call this also hold the transformed run's own CFL result to these steps
         at 1e-12, which the CFL reduction without the bound misses by 1e-5.)  -> the steps from the second on."""
    from tests.parity_runs import errors, run_state
    d0, radii, fields, bodies = state
    opt = case[6]
    d = d0.copy()
    d.stabilize_viscosity = 0
    twin, tdts, _, _ = run_state(oracle, d, radii, fields, 1, opt["steps"], "host", dt_scale=opt.get("dt_scale", 1.0),
                                 bodies=bodies)
    assert dts[0] == tdts[0], f"{case[0]}: the first step differs from the run without the option: {dts[0]!r} vs {tdts[0]!r}"
    if opt["stab"] == 1:
        errs = errors(d0, radii, base, twin, sum(tdts))
        moved = max(errs["vrad"][0], errs["vazi"][0])
        assert moved > 1.0e-6, f"{case[0]}: StabilizeViscosity 1 is inert in this state: the velocities differ by {moved:.1e}"
    else:
        assert len(dts) > 1 and all(a < b for a, b in zip(dts[1:], tdts[1:])), (
            f"{case[0]}: the viscous bound of StabilizeViscosity 2 does not set the step: {dts} vs {tdts}")
    return dts[1:]


def bar_of(response):
    return max(BAR_FLOOR, BAR_MARGIN * response)


def residual(d0, radii, back, base, time):
    """-> (worst cell-wise error of the transformed run brought back against the untransformed one, grid, (ring, column))"""
    from tests.parity_runs import errors
    errs = errors(d0, radii, back, base, time)
    k = max(errs, key=lambda n: errs[n][0])
    return errs[k][0], k, errs[k][1]


def same_bits(back, base):
    """The grids that differ in any bit: [(grid, cells that differ, (ring, column) of the first)]"""
    bad = []
    for k in base:
        ne = np.argwhere(back[k] != base[k])
        if ne.size:
            bad.append((k, len(ne), tuple(int(v) for v in ne[0])))
    return bad
