"""The per-ring tables fcpt_create uploads (csrc/fcpt_tables.cpp), bit for bit, without a GPU.

fcpt_selftest_ring_tables returns every table for a descriptor and a slab; `Expect` restates each column in numpy from
what the kernels of narrow rings read from the plain geometry arrays (kernels/source_fused.h, transport.h, cfl.h: the
marching kernels take the same factors from the packed rows), from the row structures' comments in
csrc/fcpt_internal.h and from the reference's damping ranges (boundary_conditions/damping.cpp:311-427).  Every
operation is one IEEE double operation in the kernels' order, so the comparison is of bit patterns.  The two columns
that go through pow (g_ra3, cs_ring) call math.pow per element: numpy's power need not be libm's."""
import math

import numpy as np
import pytest

from fargocpt_amd import binding as B, setups
from tests import cfl_plants

SRC_COLS = ("cs2_m cs2_m1 idr_m rinf_om_m inv_rinf_m inv_dxt_m inv_drsup_b inv_rmed_b lsq_b inv_rsum_c rmed_c rmed_cm1 "
            "inv_drmed2_c idr_c inv_dxtheta_c rinf_d1 rinf_d0 inv_drsuprb_d inv_rmed_d inv_drsup_d nu_d inv_rmed_r "
            "inv_rmed_rm1 idr_r rinf_r inv_rinf_r nu_avg_r inv_rmed_k two_inv_dra2_k ra1sq_k ra0sq_k inv_rmsum_k rmed_k "
            "rmed_km1 idr_k rinf_b1 rinf_b0 inv_drsuprb_b inv_omk_b inv_dxtheta_b").split()
RAD_COLS = "dr_lo dr_hi gphi idr_up".split()
THETA_COLS = "invsurf dxtheta inv_dxtheta dr_invsurf invr r_omega rmed pad".split()
DAMP_COLS = "fs ts fv tv tvr tva tsg ten pad0 pad1".split()
RING_COLS = ("cs_ring nu_ring g_dxtheta g_inv_dxtheta g_dr_invsurf g_r_omega g_inv_omk g_omk g_ra3 dfac_s dtau_s dfac_v "
             "dtau_v dtype_vr dtype_va dtype_sig dtype_e ring_ref_damped").split()
RANGE_COLS = "lo hi type rlim redge tau".split()
TABLES = {B.TABLE_SRC: SRC_COLS, B.TABLE_RAD: RAD_COLS, B.TABLE_THETA: THETA_COLS, B.TABLE_DAMP: DAMP_COLS,
          B.TABLE_RING: RING_COLS, B.TABLE_DAMP_RANGES: RANGE_COLS, B.TABLE_AZIMUTH: ["cosphi", "sinphi"]}

N, R, Z, M = B.DAMP_NONE, B.DAMP_REFERENCE, B.DAMP_ZERO, B.DAMP_MEAN
MIXED = dict(damp_vrad=(Z, R), damp_vaz=(R, Z), damp_sigma=(N, R), damp_energy=(R, N))


def _case(nr, nphi, rank=0, nranks=1, wide_zones=False, **fields):
    return dict(nr=nr, nphi=nphi, rank=rank, nranks=nranks, wide_zones=wide_zones, fields=fields)


CASES = {
    # nphi <= 16: the TW length scale is the smaller of the two cell widths (lsq_b), above it the larger; damping off
    "24x8-min-nodamping": _case(24, 8, damping=0),
    "32x32-max": _case(32, 32),
    # slab edges that are not grid edges, is_first / is_last differ (the split of test_split_domain)
    "slab0of2": _case(128, 16, 0, 2, wide_zones=True), "slab1of2": _case(128, 16, 1, 2, wide_zones=True),
    "arithmetic": _case(64, 24, radial_spacing=B.SPACING_ARITHMETIC),
    "logarithmic": _case(64, 24, radial_spacing=B.SPACING_LOGARITHMIC),
    "exponential": _case(64, 24, radial_spacing=B.SPACING_EXPONENTIAL),
    # planet_disk has alpha = 1e-3; a constant viscosity reaches nu_d and nu_avg_r by the other branch
    "constant-nu": _case(32, 32, viscous_alpha=0.0, constant_viscosity=1.0e-5),
    "flared": _case(32, 32, flaring_index=0.25, omega_frame=0.37),
    # zones several rings wide, every FCPT_DAMP_* type on some field and edge
    "damp-mixed": _case(64, 24, wide_zones=True, **MIXED),
    "damp-leapfrog": _case(64, 24, wide_zones=True, integrator=B.INTEGRATOR_LEAPFROG, **MIXED),
    "damp-mean": _case(64, 24, wide_zones=True, **dict(MIXED, damp_sigma=(M, R))),
}


def case_desc(lib, c):
    d = setups.planet_disk(lib, c["nr"], c["nphi"])
    d.rank, d.nranks = c["rank"], c["nranks"]
    if c["wide_zones"]:
        d.damping_inner_limit, d.damping_outer_limit = 1.35, 0.75
    for k, v in c["fields"].items():
        if isinstance(v, tuple):
            getattr(d, k)[0], getattr(d, k)[1] = v
        else:
            setattr(d, k, v)
    dfull = d.copy()
    dfull.rank, dfull.nranks = 0, 1
    return d, lib.radii(dfull)


def tables_of(lib, d, radii):
    return {t: lib.selftest_ring_tables(d, radii, t) for t in TABLES}


# ---------------------------------------------------------------------------------------------------------------
# the restatement
def _pick(a, idx, ok=None):
    """a[idx] where `ok` (default: idx >= 0: the arrays carry GEOM_PAD rings beyond the slab), else 0."""
    idx = np.asarray(idx)
    ok = (idx >= 0) if ok is None else ok
    return np.where(ok, a[np.clip(idx, 0, len(a) - 1)], 0.0)


class Expect:
    def __init__(self, lib, d, radii):
        self.d = d
        self.g = g = cfl_plants.geometry(lib, d, radii, pad=B.GEOM_PAD)
        nr = g.nr
        GM = d.G * d.hydro_center_mass
        rm = g.Rmed[:nr]
        # c_s = h v_K with h = AspectRatio r^FlaringIndex (SourceEuler.cpp:1080-1088); Omega_K = sqrt(G M / r^3)
        self.cs = np.array([(d.aspect_ratio * math.pow(r, d.flaring_index)) * math.sqrt(GM / r) for r in rm])
        self.omk = np.sqrt(GM / (rm * rm * rm))
        H = self.cs * (1.0 / self.omk)   # k_iso_cs_h, then k_viscosity: nu = alpha H c_s
        self.nu = d.viscous_alpha * H * self.cs
        self._damping()

    def nu_of(self, ring):
        """The viscosity the isothermal kernels find in ring `ring` (clamped to the slab): alpha, or the constant."""
        if self.d.viscous_alpha > 0:
            return self.nu[np.clip(ring, 0, self.g.nr - 1)]
        return np.full(np.shape(ring), self.d.constant_viscosity)

    # damping.cpp:311-427: rows 0 .. id(RMIN limit) and id(RMAX limit) + 1 .. last, ids clamped to the slab's rows
    def _damping(self):
        d, g, nr = self.d, self.g, self.g.nr
        types = [tuple(d.damp_vrad), tuple(d.damp_vaz), tuple(d.damp_sigma), tuple(d.damp_energy)]
        self.ranges = np.zeros((9, 6))
        self.fac = {True: np.zeros(nr + 1), False: np.zeros(nr + 1)}     # by is_vector
        self.tau = {True: np.ones(nr + 1), False: np.ones(nr + 1)}
        self.ty = np.zeros((4, nr + 1))
        any_, mean = False, False
        for q in range(4):
            vec = q == 0
            radius, rows = (g.Rinf, nr + 1) if vec else (g.Rmed, nr)
            for o in range(2):
                lo, hi, rlim, redge, tau = 0, -1, 0.0, 0.0, 0.0
                ty = types[q][o]
                if d.damping and ty != B.DAMP_NONE:
                    if o == 0 and d.damping_inner_limit > 1.0 and radius[0] < d.rmin * d.damping_inner_limit:
                        rlim, redge = d.rmin * d.damping_inner_limit, d.rmin
                        # the row whose radius is the last one not above the limit (get_rmed_id / get_rinf_id)
                        lo, hi = 0, min(max(int(np.searchsorted(radius, rlim, side="right")) - 1, 0), rows - 1)
                        tau = d.damping_time_factor * 2.0 * math.pi / math.sqrt(d.G * d.hydro_center_mass / (d.rmin * d.rmin * d.rmin))
                    if o == 1 and d.damping_outer_limit < 1.0 and radius[rows - 1] > d.rmax * d.damping_outer_limit:
                        rlim, redge = d.rmax * d.damping_outer_limit, d.rmax
                        lo, hi = min(max(int(np.searchsorted(radius, rlim, side="right")), 0), rows - 1), rows - 1
                        ro = d.damping_time_radius_outer
                        tau = d.damping_time_factor * 2.0 * math.pi / math.sqrt(d.G * d.hydro_center_mass / (ro * ro * ro))
                self.ranges[2 * q + o] = (lo, hi, ty, rlim, redge, tau)
                if ty == B.DAMP_NONE or lo > hi:
                    continue
                any_, mean = True, mean or ty == B.DAMP_MEAN
                i = np.arange(lo, hi + 1)
                f = (radius[i] - rlim) / (redge - rlim)
                self.fac[vec][i] = f * f
                self.tau[vec][i] = tau
                self.ty[q][i] = 1 if ty == B.DAMP_REFERENCE else 2   # (2 for "mean" too, which is never folded)
        self.damp_any = bool(d.damping and any_)
        # leapfrog kicks once more after the transport and "mean" needs a ring sum: neither folds into the transport
        self.damp_foldable = self.damp_any and not mean and d.integrator == B.INTEGRATOR_EULER
        self.ranges[8, :2] = (self.damp_any, self.damp_foldable)

    def ring(self):
        d, g, nr = self.d, self.g, self.g.nr
        rm, ri, rs = g.Rmed[:nr], g.Rinf[:nr], g.Rsup[:nr]
        out = np.zeros((nr + 2, len(RING_COLS)))
        c = {n: k for k, n in enumerate(RING_COLS)}
        out[:nr, c["cs_ring"]] = self.cs
        out[:nr, c["nu_ring"]] = self.nu
        out[:nr, c["g_dxtheta"]] = g.dphi * rm
        out[:nr, c["g_inv_dxtheta"]] = 1.0 / (g.dphi * rm)
        out[:nr, c["g_dr_invsurf"]] = (rs - ri) * g.InvSurf[:nr]
        out[:nr, c["g_r_omega"]] = rm * d.omega_frame
        out[:nr, c["g_inv_omk"]] = 1.0 / self.omk
        out[:nr, c["g_omk"]] = self.omk
        out[:nr + 1, c["g_ra3"]] = [math.pow(r, 3) for r in g.Rinf[:nr + 1]]
        out[:nr + 1, c["dfac_s"]], out[:nr + 1, c["dtau_s"]] = self.fac[False], self.tau[False]
        out[:nr + 1, c["dfac_v"]], out[:nr + 1, c["dtau_v"]] = self.fac[True], self.tau[True]
        for q, n in enumerate(("dtype_vr", "dtype_va", "dtype_sig", "dtype_e")):
            out[:nr + 1, c[n]] = self.ty[q]
        out[:nr, c["ring_ref_damped"]] = (self.ty[:, :nr] == 1).any(axis=0)
        return out

    def damp_rows(self):
        nr = self.g.nr
        out = np.zeros((nr + 1, len(DAMP_COLS)))
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = self.fac[False], self.tau[False], self.fac[True], self.tau[True]
        out[:, 4:8] = self.ty.T
        return out

    def theta(self):
        d, g, nr = self.d, self.g, self.g.nr
        rm = g.Rmed[:nr]
        return np.stack([g.InvSurf[:nr], g.dphi * rm, 1.0 / (g.dphi * rm), (g.Rsup[:nr] - g.Rinf[:nr]) * g.InvSurf[:nr],
                         g.InvRmed[:nr], rm * d.omega_frame, rm, np.zeros(nr)], axis=1)

    def rad(self):
        g, nr = self.g, self.g.nr
        k = np.arange(-1, nr + 1)
        kk = np.where((k > 0) & (k < nr), k, 1)   # an interface with a ring on both sides, else interface 1
        up = (k >= 0) & (k + 1 <= nr - 1)         # rings k and k + 1 both exist
        return np.stack([g.Rmed[kk] - g.Rmed[kk - 1], g.Rmed[kk + 1] - g.Rmed[kk], g.dphi * g.Rinf[kk],
                         _pick(g.InvDiffRmed, k + 1, up)], axis=1)

    def src(self):
        """Iteration m of the marching source kernel works on rings m (stage A), m - 1 (B, C, r-phi stress) and m - 2
        (diagonal stress, E); a clamped ring index where the kernel runs the stage on every iteration, a guarded one
        (zeros outside) where it tests the row range."""
        d, g, nr = self.d, self.g, self.g.nr
        m = np.arange(-2, nr + 6)
        crow = lambda r: np.clip(r, 0, nr - 1)
        f = {}
        # A: k_src_fused (pressure gradient of P = Sigma c_s^2 between rings m and m - 1, centrifugal term; v_phi)
        f["cs2_m"] = self.cs[crow(m)] * self.cs[crow(m)]
        f["cs2_m1"] = self.cs[crow(m - 1)] * self.cs[crow(m - 1)]
        f["idr_m"] = _pick(g.InvDiffRmed, m)
        f["rinf_om_m"] = _pick(g.Rinf, m) * d.omega_frame
        f["inv_rinf_m"] = _pick(g.InvRinf, m)
        f["inv_dxt_m"] = _pick(2.0 / (g.dphi * (g.Rsup + g.Rinf)), m, (m >= 0) & (m <= nr))
        # B: tw_q_at of ring crow(m - 1), and the energy equation's factors of the same ring (k_av_fused: compression heating, SN dissipation)
        b = crow(m - 1)
        dr, rdphi = g.Rinf[b + 1] - g.Rinf[b], g.Rmed[b] * g.dphi
        dx = np.minimum(dr, rdphi) if d.nphi <= 16 else np.maximum(dr, rdphi)
        f["inv_drsup_b"], f["inv_rmed_b"] = g.InvDiffRsup[b], g.InvRmed[b]
        f["lsq_b"] = (d.artificial_viscosity_factor * d.artificial_viscosity_factor) * (dx * dx)
        f["rinf_b1"], f["rinf_b0"], f["inv_drsuprb_b"] = g.Rinf[b + 1], g.Rinf[b], g.InvDiffRsupRb[b]
        rb = g.Rmed[b]
        f["inv_omk_b"] = 1.0 / np.sqrt(d.G * d.hydro_center_mass / (rb * rb * rb))
        f["inv_dxtheta_b"] = 1.0 / (g.dphi * rb)
        # C: the TW velocity updates of k_av_fused on ring m - 1
        c = m - 1
        ok = (c >= 1) & (c <= nr)
        rsum = g.Rsup + g.Rinf
        drmed2 = np.zeros_like(g.Rmed)
        drmed2[1:] = g.Rmed[1:] * g.Rmed[1:] - g.Rmed[:-1] * g.Rmed[:-1]
        f["inv_rsum_c"] = _pick(1.0 / rsum, c, ok)
        f["rmed_c"], f["rmed_cm1"] = _pick(g.Rmed, c, ok), _pick(g.Rmed, c - 1, ok)
        with np.errstate(divide="ignore"):
            f["inv_drmed2_c"] = _pick(1.0 / drmed2, c, ok)
        f["idr_c"] = _pick(g.InvDiffRmed, c)
        f["inv_dxtheta_c"] = _pick(g.InvRmed, c) * g.invdphi
        # D: tau_diag_at of ring crow(m - 2) ...
        dd = crow(m - 2)
        f["rinf_d1"], f["rinf_d0"], f["inv_drsuprb_d"] = g.Rinf[dd + 1], g.Rinf[dd], g.InvDiffRsupRb[dd]
        f["inv_rmed_d"], f["inv_drsup_d"], f["nu_d"] = g.InvRmed[dd], g.InvDiffRsup[dd], self.nu_of(m - 2)
        # ... and tau_rp_at of rows 1 .. nr - 1 (ring m - 1): the four-cell mean of a viscosity that is constant along a ring
        ok = (c >= 1) & (c <= nr - 1)
        f["inv_rmed_r"], f["inv_rmed_rm1"] = _pick(g.InvRmed, c, ok), _pick(g.InvRmed, c - 1, ok)
        f["idr_r"], f["rinf_r"], f["inv_rinf_r"] = _pick(g.InvDiffRmed, c, ok), _pick(g.Rinf, c, ok), _pick(g.InvRinf, c, ok)
        nu1, nu2 = self.nu_of(c), self.nu_of(c - 1)
        f["nu_avg_r"] = np.where(ok, 0.25 * (nu1 + nu2 + nu1 + nu2), 0.0)
        # E: the velocity updates of k_visc_fused on ring m - 2
        k = m - 2
        ok = (k >= 1) & (k <= nr)
        ra1, ra0 = _pick(g.Rinf, k + 1, ok), _pick(g.Rinf, k, ok)
        f["inv_rmed_k"] = _pick(g.InvRmed, k, ok)
        with np.errstate(divide="ignore", invalid="ignore"):
            f["two_inv_dra2_k"] = np.where(ok, 2.0 / (ra1 * ra1 - ra0 * ra0), 0.0)
            f["inv_rmsum_k"] = np.where(ok, 1.0 / (_pick(g.Rmed, k, ok) + _pick(g.Rmed, k - 1, ok)), 0.0)
        f["ra1sq_k"], f["ra0sq_k"] = ra1 * ra1, ra0 * ra0
        f["rmed_k"], f["rmed_km1"], f["idr_k"] = _pick(g.Rmed, k, ok), _pick(g.Rmed, k - 1, ok), _pick(g.InvDiffRmed, k, ok)
        return np.stack([f[n] for n in SRC_COLS], axis=1)

    def azimuth(self):
        g = self.g
        return np.array([[math.cos(g.dphi * float(j)), math.sin(g.dphi * float(j))] for j in range(g.nphi)])

    def all(self):
        return {B.TABLE_SRC: self.src(), B.TABLE_RAD: self.rad(), B.TABLE_THETA: self.theta(), B.TABLE_DAMP: self.damp_rows(),
                B.TABLE_RING: self.ring(), B.TABLE_DAMP_RANGES: self.ranges, B.TABLE_AZIMUTH: self.azimuth()}


# ---------------------------------------------------------------------------------------------------------------
_RESULTS = {}


def _result(product, name):
    if name not in _RESULTS:
        d, radii = case_desc(product, CASES[name])
        _RESULTS[name] = (d, tables_of(product, d, radii), Expect(product, d, radii))
    return _RESULTS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_column_of_every_table_bit_for_bit(product, name):
    d, got, exp = _result(product, name)
    want = exp.all()
    bad = []
    for t, cols in TABLES.items():
        a, b = got[t], np.ascontiguousarray(want[t], dtype=np.float64)
        assert a.shape == b.shape == (b.shape[0], len(cols)), (t, a.shape, b.shape)
        ne = a.view(np.uint64) != b.view(np.uint64)
        bad += [(t, cols[c], int(ne[:, c].sum()), int(np.argmax(ne[:, c]))) for c in range(len(cols)) if ne[:, c].any()]
    assert not bad, bad   # (table, column, rows that differ, first of them)


def test_the_cases_reach_the_branches_they_are_meant_for(product):
    s0, s1 = (_result(product, n)[2].g for n in ("slab0of2", "slab1of2"))
    assert (s0.is_first, s0.is_last, s1.is_first, s1.is_last) == (True, False, False, True) and s1.imin > 0
    flags = {n: tuple(_result(product, n)[1][B.TABLE_DAMP_RANGES][8, :2]) for n in CASES}
    assert flags["24x8-min-nodamping"] == (0.0, 0.0) and flags["damp-mixed"] == (1.0, 1.0)
    assert flags["damp-leapfrog"] == (1.0, 0.0) and flags["damp-mean"] == (1.0, 0.0)
    ranges = _result(product, "damp-mixed")[1][B.TABLE_DAMP_RANGES][:8]
    on = ranges[:, 0] <= ranges[:, 1]
    assert on.sum() == 6 and (ranges[on, 1] - ranges[on, 0] >= 3).all()   # zones several rings wide
    seen = {int(t) for n in ("damp-mixed", "damp-mean") for t in _result(product, n)[1][B.TABLE_DAMP_RANGES][:8, 2]}
    assert seen == {N, R, Z, M}
    # the inner zone lies in slab 0 only, the outer one in slab 1 only
    r0, r1 = (_result(product, n)[1][B.TABLE_DAMP_RANGES][:8] for n in ("slab0of2", "slab1of2"))
    assert (r0[0::2, 0] <= r0[0::2, 1]).all() and (r0[1::2, 0] > r0[1::2, 1]).all()
    assert (r1[0::2, 0] > r1[0::2, 1]).all() and (r1[1::2, 0] <= r1[1::2, 1]).all()
    d8, d32 = _result(product, "24x8-min-nodamping"), _result(product, "32x32-max")
    for (d, got, exp), smaller in ((d8, True), (d32, False)):
        g = exp.g
        dr, rdphi = g.Rinf[1] - g.Rinf[0], g.Rmed[0] * g.dphi
        assert dr != rdphi
        dx = min(dr, rdphi) if smaller else max(dr, rdphi)
        assert got[B.TABLE_SRC][2, SRC_COLS.index("lsq_b")] == (d.artificial_viscosity_factor * d.artificial_viscosity_factor) * (dx * dx)
    assert (_result(product, "constant-nu")[1][B.TABLE_SRC][:, SRC_COLS.index("nu_d")] == 1.0e-5).all()


@pytest.mark.parametrize("name", ["24x8-min-nodamping", "slab1of2", "exponential", "constant-nu"])
def test_rows_outside_the_grid(product, name):
    """Rows m = -2, -1 and nr + 1 .. nr + 5 of SrcRow: what the kernel guards by a row range is exactly zero there, what
    it reads on every iteration holds the value of the nearest ring of the slab."""
    d, got, exp = _result(product, name)
    src, nr = got[B.TABLE_SRC], exp.g.nr
    col = lambda n: src[:, SRC_COLS.index(n)]
    row = lambda m: m + 2
    guarded = {   # field -> iterations m at which its ring lies inside the stage's row range
        "inv_dxt_m": range(0, nr + 1),
        **{n: range(2, nr + 2) for n in ("inv_rsum_c", "rmed_c", "rmed_cm1", "inv_drmed2_c")},
        **{n: range(2, nr + 1) for n in ("inv_rmed_r", "inv_rmed_rm1", "idr_r", "rinf_r", "inv_rinf_r", "nu_avg_r")},
        **{n: range(3, nr + 3) for n in ("inv_rmed_k", "two_inv_dra2_k", "ra1sq_k", "ra0sq_k", "inv_rmsum_k", "rmed_k", "rmed_km1", "idr_k")},
    }
    for n, inside in guarded.items():
        for m in range(-2, nr + 6):
            v = col(n)[row(m)]
            if m not in inside:
                assert v == 0.0 and not np.signbit(v), (n, m, v)
            else:
                assert v != 0.0, (n, m)
    clamped = {"cs2_m": 0, "cs2_m1": 1, "inv_drsup_b": 1, "inv_rmed_b": 1, "lsq_b": 1, "rinf_b1": 1, "rinf_b0": 1, "inv_drsuprb_b": 1,
               "inv_omk_b": 1, "inv_dxtheta_b": 1, "rinf_d1": 2, "rinf_d0": 2, "inv_drsuprb_d": 2, "inv_rmed_d": 2, "inv_drsup_d": 2,
               "nu_d": 2}   # field -> its ring is crow(m - this)
    for n, back in clamped.items():
        v = col(n)
        for m in range(-2, nr + 6):
            ring = min(max(m - back, 0), nr - 1)
            assert v[row(m)] == v[row(ring + back)] != 0.0, (n, m)
