// The host-only stages of fcpt_create: what it refuses, every per-ring table the kernels read, and the scalars of
// the kernels' Dev view.  Plain arithmetic on the descriptor, the split and the geometry: no HIP, no environment.
// The marching kernels depend on these tables bit for bit; fcpt_selftest_ring_tables returns them on any machine.
#include "fcpt_internal.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace fcpt {

int validate_create(const fcpt_desc *d, const double *radii)
{
    if (!d || !radii) {
        set_error("null argument");
        return FCPT_EINVAL;
    }
    if (d->struct_size != sizeof(fcpt_desc) || d->abi_version != FCPT_ABI_VERSION) {
        set_error("descriptor ABI mismatch: size %u (expected %zu), version %u (expected %d)", d->struct_size,
                  sizeof(fcpt_desc), d->abi_version, FCPT_ABI_VERSION);
        return FCPT_EINVAL;
    }
    if (d->stabilize_viscosity < 0 || d->stabilize_viscosity > 2) {
        set_error("StabilizeViscosity must be 0, 1 or 2");
        return FCPT_EINVAL;
    }
    if (d->cooling_surface && d->eos == FCPT_EOS_IDEAL && (d->opacity < FCPT_OPACITY_LIN || d->opacity > FCPT_OPACITY_SIMPLE)) {
        set_error("Opacity: Lin, Bell, Constant and Simple are the laws of the path (src/opacity.cpp:10-43)");
        return FCPT_EINVAL;
    }
    // the exponential spacing's Newton iteration (init.cpp:113-131) collapses to NaN for coarse grids
    for (int i = 0; d->nr_global >= 1 && i <= d->nr_global + FCPT_GEOM_PAD; ++i)
        if (!std::isfinite(radii[i]) || radii[i] <= 0.0 || (i > 0 && !(radii[i] > radii[i - 1]))) {
            set_error("radii[%d] = %g: the interfaces must be finite, positive and strictly increasing", i, radii[i]);
            return FCPT_EINVAL;
        }
    if ((long long)(d->nr_global + 1) * (long long)d->nphi >= (1ll << 31)) {
        set_error("grid too large for 32-bit cell indices");
        return FCPT_EINVAL;
    }
    return FCPT_OK;
}

double omega_kepler(const fcpt_desc &d, double r) { return std::sqrt(d.G * d.hydro_center_mass / (r * r * r)); }

// damping.cpp:311-427: which rows a damping call touches and its time scale
DampRange damp_range(const fcpt_desc &d, const fcpt_split &s, const HostGeometry &g, int is_vector, int type, int outer)
{
    DampRange r;
    r.lo = 0;
    r.hi = -1;
    r.type = type;
    r.rlim = r.redge = r.tau = 0;
    if (!d.damping || type == FCPT_DAMP_NONE)
        return r;
    const std::vector<double> &radius = is_vector ? g.Rinf : g.Rmed;
    const int nr = s.nr;
    const int size_radial = is_vector ? nr + 1 : nr;
    auto clamp = [&](int id) {
        const int mx = nr - (is_vector ? 0 : 1);
        return id < 0 ? 0 : (id > mx ? mx : id);
    };
    if (!outer) {
        if (!((d.damping_inner_limit > 1.0) && (radius[0] < d.rmin * d.damping_inner_limit)))
            return r;
        const double rl = d.rmin * d.damping_inner_limit;
        const int limit = clamp(is_vector ? rinf_id(d, s, g, rl) : rmed_id(d, s, g, rl));
        r.lo = 0;
        r.hi = limit;
        r.rlim = rl;
        r.redge = d.rmin;
        r.tau = d.damping_time_factor * 2.0 * M_PI / omega_kepler(d, d.rmin);
    } else {
        if (!((d.damping_outer_limit < 1.0) && (radius[size_radial - 1] > d.rmax * d.damping_outer_limit)))
            return r;
        const double rl = d.rmax * d.damping_outer_limit;
        const int limit = clamp((is_vector ? rinf_id(d, s, g, rl) : rmed_id(d, s, g, rl)) + 1);
        r.lo = limit;
        r.hi = size_radial - 1;
        r.rlim = rl;
        r.redge = d.rmax;
        r.tau = d.damping_time_factor * 2.0 * M_PI / omega_kepler(d, d.damping_time_radius_outer);
    }
    return r;
}

namespace {

void build_plain_arrays(const fcpt_desc &d, const fcpt_split &s, const HostGeometry &g, RingTables &t)
{
    const int nr = s.nr, nphi = d.nphi;
    t.cosphi.assign(nphi, 0.0);
    t.sinphi.assign(nphi, 0.0);
    t.cs_ring.assign(nr, 0.0);
    for (int j = 0; j < nphi; ++j) { // SideEuler.cpp:60-63
        t.cosphi[j] = std::cos(g.dphi * (double)j);
        t.sinphi[j] = std::sin(g.dphi * (double)j);
    }
    for (int i = 0; i < nr; ++i) { // SourceEuler.cpp:1080-1088
        const double vK = std::sqrt(d.G * d.hydro_center_mass / g.Rmed[i]);
        const double h = d.aspect_ratio * std::pow(g.Rmed[i], d.flaring_index);
        t.cs_ring[i] = h * vK;
    }
    for (auto *v : {&t.g_dxtheta, &t.g_inv_dxtheta, &t.g_dr_invsurf, &t.g_r_omega, &t.g_inv_omk, &t.g_omk})
        v->assign(nr + 1, 0.0);
    for (int i = 0; i < nr; ++i) {
        t.g_dxtheta[i] = g.dphi * g.Rmed[i];
        t.g_inv_dxtheta[i] = 1.0 / t.g_dxtheta[i];
        t.g_dr_invsurf[i] = (g.Rsup[i] - g.Rinf[i]) * g.InvSurf[i];
        t.g_r_omega[i] = g.Rmed[i] * d.omega_frame;
        t.g_omk[i] = omega_kepler(d, g.Rmed[i]);
        t.g_inv_omk[i] = 1.0 / omega_kepler(d, g.Rmed[i]);
    }
    t.g_ra3.assign(nr + 2, 0.0);
    for (int i = 0; i <= nr; ++i)
        t.g_ra3[i] = std::pow(g.Rinf[i], 3);
    // isothermal alpha viscosity per ring, exactly as k_iso_cs_h + k_viscosity evaluate it:
    // H = cs * (1 / Omega_K), nu = alpha * H * cs
    t.nu_ring.assign(nr, 0.0);
    for (int i = 0; i < nr; ++i) {
        const double H = t.cs_ring[i] * (1.0 / omega_kepler(d, g.Rmed[i]));
        t.nu_ring[i] = d.viscous_alpha * H * t.cs_ring[i];
    }
}

void build_rad_theta_rows(const fcpt_split &s, const HostGeometry &g, RingTables &t)
{
    const int nr = s.nr;
    t.rad.assign(nr + 2, RadRow());
    for (int k = -1; k <= nr; ++k) {
        const bool open = k > 0 && k < nr;
        const int kk = open ? k : 1;
        RadRow &r = t.rad[k + 1];
        r.dr_lo = g.Rmed[kk] - g.Rmed[kk - 1];
        r.dr_hi = g.Rmed[kk + 1] - g.Rmed[kk];
        r.gphi = g.dphi * g.Rinf[kk];
        r.idr_up = (k + 1 >= 1 && k + 1 <= nr - 1) ? g.InvDiffRmed[k + 1] : 0.0;
    }
    t.theta.resize(nr);
    for (int i = 0; i < nr; ++i)
        t.theta[i] = ThetaRow{g.InvSurf[i], t.g_dxtheta[i], t.g_inv_dxtheta[i], t.g_dr_invsurf[i], g.InvRmed[i], t.g_r_omega[i], g.Rmed[i], 0.0};
}

// per-iteration rows of the marching source kernel (k_source_march): every per-ring factor
// with the index expression and operation order of the kernel's former array reads
void build_src_rows(const fcpt_desc &d, const fcpt_split &s, const HostGeometry &g, RingTables &t)
{
    const int nr = s.nr, nphi = d.nphi;
    const std::vector<double> &cs_ring = t.cs_ring, &nu_ring = t.nu_ring;
    auto at = [](const std::vector<double> &v, int i) { return (i >= 0 && i < (int)v.size()) ? v[i] : 0.0; };
    auto crow = [nr](int r) { return r < 0 ? 0 : (r > nr - 1 ? nr - 1 : r); };
    const bool alpha = d.viscous_alpha > 0;
    auto nu_of = [&](int r) { return alpha ? nu_ring[crow(r)] : d.constant_viscosity; };
    const double C2 = d.artificial_viscosity_factor * d.artificial_viscosity_factor;
    std::vector<SrcRow> &rows = t.src;
    rows.resize(nr + 8);
    for (int m = -2; m <= nr + 5; ++m) {
        SrcRow &R = rows[m + 2];
        std::memset(&R, 0, sizeof(R));
        {
            const int rc0 = crow(m), rc1 = crow(m - 1);
            R.cs2_m = cs_ring[rc0] * cs_ring[rc0];
            R.cs2_m1 = cs_ring[rc1] * cs_ring[rc1];
            R.idr_m = at(g.InvDiffRmed, m);
            R.rinf_om_m = at(g.Rinf, m) * d.omega_frame;
            R.inv_rinf_m = at(g.InvRinf, m);
            R.inv_dxt_m = (m >= 0 && m <= nr) ? 2.0 / (g.dphi * (g.Rsup[m] + g.Rinf[m])) : 0.0;
        }
        {
            const int r = crow(m - 1);
            R.inv_drsup_b = g.InvDiffRsup[r];
            R.inv_rmed_b = g.InvRmed[r];
            const double Dr = g.Rinf[r + 1] - g.Rinf[r];
            const double rDphi = g.Rmed[r] * g.dphi;
            const double dx = nphi <= 16 ? std::min(Dr, rDphi) : std::max(Dr, rDphi);
            R.lsq_b = C2 * (dx * dx);
            R.rinf_b1 = g.Rinf[r + 1];
            R.rinf_b0 = g.Rinf[r];
            R.inv_drsuprb_b = g.InvDiffRsupRb[r];
            const double rm = g.Rmed[r];
            R.inv_omk_b = 1.0 / omega_kepler(d, rm);
            R.inv_dxtheta_b = 1.0 / (g.dphi * rm);
        }
        {
            const int r = m - 1;
            if (r >= 1 && r <= nr) {
                R.inv_rsum_c = 1.0 / (g.Rsup[r] + g.Rinf[r]);
                R.rmed_c = g.Rmed[r];
                R.rmed_cm1 = g.Rmed[r - 1];
                R.inv_drmed2_c = 1.0 / (g.Rmed[r] * g.Rmed[r] - g.Rmed[r - 1] * g.Rmed[r - 1]);
            }
            R.idr_c = at(g.InvDiffRmed, r);
            R.inv_dxtheta_c = at(g.InvRmed, r) * g.invdphi;
        }
        {
            const int r = crow(m - 2);
            R.rinf_d1 = g.Rinf[r + 1];
            R.rinf_d0 = g.Rinf[r];
            R.inv_drsuprb_d = g.InvDiffRsupRb[r];
            R.inv_rmed_d = g.InvRmed[r];
            R.inv_drsup_d = g.InvDiffRsup[r];
            R.nu_d = nu_of(m - 2);
        }
        {
            const int r = m - 1;
            if (r >= 1 && r <= nr - 1) {
                R.inv_rmed_r = g.InvRmed[r];
                R.inv_rmed_rm1 = g.InvRmed[r - 1];
                R.idr_r = g.InvDiffRmed[r];
                R.rinf_r = g.Rinf[r];
                R.inv_rinf_r = g.InvRinf[r];
                const double nu1 = nu_of(r), nu2 = nu_of(r - 1);
                R.nu_avg_r = 0.25 * (nu1 + nu2 + nu1 + nu2);
            }
        }
        {
            const int k = m - 2;
            if (k >= 1 && k <= nr) {
                const double ra1 = at(g.Rinf, k + 1), ra0 = g.Rinf[k];
                R.inv_rmed_k = at(g.InvRmed, k);
                R.two_inv_dra2_k = 2.0 * (1.0 / (ra1 * ra1 - ra0 * ra0));
                R.ra1sq_k = ra1 * ra1;
                R.ra0sq_k = ra0 * ra0;
                R.inv_rmsum_k = 1.0 / (g.Rmed[k] + g.Rmed[k - 1]);
                R.rmed_k = g.Rmed[k];
                R.rmed_km1 = g.Rmed[k - 1];
                R.idr_k = at(g.InvDiffRmed, k);
            }
        }
    }
}

// per-ring damping tables for the fused end-of-transport kernel (reference / zero targets;
// "mean" needs a ring reduction and keeps the separate k_damping launches)
void build_damping(const fcpt_desc &d, const fcpt_split &s, const HostGeometry &g, RingTables &t)
{
    const int nr = s.nr;
    const int dtype[4][2] = {{d.damp_vrad[0], d.damp_vrad[1]},
                             {d.damp_vaz[0], d.damp_vaz[1]},
                             {d.damp_sigma[0], d.damp_sigma[1]},
                             {d.damp_energy[0], d.damp_energy[1]}};
    for (int q = 0; q < 4; ++q)
        for (int o = 0; o < 2; ++o)
            t.damp[q][o] = damp_range(d, s, g, q == 0, dtype[q][o], o);
    std::vector<double> &fs = t.fs, &ts = t.ts, &fv = t.fv, &tv = t.tv;
    fs.assign(nr + 1, 0.0);
    ts.assign(nr + 1, 1.0);
    fv.assign(nr + 1, 0.0);
    tv.assign(nr + 1, 1.0);
    std::vector<int> *ty = t.dtype;
    bool any = false, mean = false;
    for (int q = 0; q < 4; ++q) {
        ty[q].assign(nr + 1, 0);
        for (int o = 0; o < 2; ++o) {
            const DampRange &r = t.damp[q][o];
            if (r.type == FCPT_DAMP_NONE || r.lo > r.hi)
                continue;
            any = true;
            mean = mean || r.type == FCPT_DAMP_MEAN;
            const std::vector<double> &radius = q == 0 ? g.Rinf : g.Rmed;
            for (int i = r.lo; i <= r.hi; ++i) {
                const double f = (radius[i] - r.rlim) / (r.redge - r.rlim);
                (q == 0 ? fv : fs)[i] = f * f;
                (q == 0 ? tv : ts)[i] = r.tau;
                ty[q][i] = r.type == FCPT_DAMP_REFERENCE ? 1 : 2;
            }
        }
    }
    t.damp_rows.resize(nr + 1);
    for (int i = 0; i <= nr; ++i)
        t.damp_rows[i] = DampRow{fs[i], ts[i], fv[i], tv[i], ty[0][i], ty[1][i], ty[2][i], ty[3][i], {0.0, 0.0}};
    t.ring_ref_damped.assign(nr, 0);
    for (int i = 0; i < nr; ++i)
        t.ring_ref_damped[i] = (ty[0][i] == 1 || ty[1][i] == 1 || ty[2][i] == 1 || ty[3][i] == 1) ? 1 : 0;
    // leapfrog kicks the gas once more after the transport, so its damping cannot be folded in
    t.damp_any = d.damping && any;
    t.damp_foldable = d.damping && any && !mean && d.integrator == FCPT_INTEGRATOR_EULER;
}

} // namespace

// per-iteration rows of k_transport_fused: for iteration m (interface k = m - 1, ring i = m - 2, next ring m + 1) the
// fields of the per-type rows at the indices the kernel's clamped loads used -- interface max(k, -1), ring i and ring
// m + 1 replaced by ring 0 where they lie outside the grid
void build_tf_rows(int nr, const std::vector<RadRow> &rad, const std::vector<ThetaRow> &theta, const std::vector<DampRow> &damp,
                   std::vector<TfRow> &rows)
{
    rows.resize((size_t)nr + TF_ROW_GUARD);
    for (int m = -3; m <= nr + 1; ++m) {
        const int k = m - 1, i = m - 2;
        const RadRow &rk = rad[(size_t)((k < -1 ? -1 : k) + 1)];
        const int ic = (i >= 0 && i < nr) ? i : 0;
        const ThetaRow &ti = theta[(size_t)ic];
        const ThetaRow &tn = theta[(size_t)((m + 1 >= 0 && m + 1 < nr) ? m + 1 : 0)];
        const DampRow &di = damp[(size_t)ic];
        TfRow &R = rows[(size_t)(m + 3)];
        std::memset(&R, 0, sizeof(R));
        R.dr_lo = rk.dr_lo, R.dr_hi = rk.dr_hi, R.idr_up = rk.idr_up, R.gphi = rk.gphi;
        R.invsurf = ti.invsurf, R.dxtheta = ti.dxtheta, R.inv_dxtheta = ti.inv_dxtheta, R.invr = ti.invr, R.r_omega = ti.r_omega;
        R.dr_invsurf = ti.dr_invsurf;
        R.r_next = tn.rmed, R.romega_next = tn.r_omega;
        R.tvr = di.tvr, R.tva = di.tva, R.tsg = di.tsg, R.ten = di.ten;
    }
}

void build_ring_tables(const fcpt_desc &d, const fcpt_split &s, const HostGeometry &g, RingTables &t)
{
    build_plain_arrays(d, s, g, t);
    build_rad_theta_rows(s, g, t);
    build_src_rows(d, s, g, t);
    build_damping(d, s, g, t);
    build_tf_rows(s.nr, t.rad, t.theta, t.damp_rows, t.tf);
}

void fill_parameters(const fcpt_desc &d, const fcpt_split &s, const HostGeometry &g, Dev &P)
{
    P.nr = s.nr;
    P.nphi = d.nphi;
    P.dphi = g.dphi;
    P.invdphi = g.invdphi;
    P.zero_no_ghost = s.zero_no_ghost;
    P.one_no_ghost_vr = s.one_no_ghost_vr;
    P.max_no_ghost = s.max_no_ghost;
    P.maxmo_no_ghost_vr = s.maxmo_no_ghost_vr;
    P.first_active = s.radial_first_active;
    P.active_size = s.radial_active_size;
    P.is_first = s.is_first;
    P.is_last = s.is_last;
    P.stabilize = d.stabilize_viscosity;
    P.accel_force = d.body_force_from_potential ? 0 : 1;
    P.adiabatic = d.eos == FCPT_EOS_IDEAL;
    P.art_visc = d.artificial_viscosity;
    P.art_visc_dissipation = d.artificial_viscosity_dissipation;
    P.heating_viscous = d.heating_viscous;
    P.fast_transport = d.fast_transport;
    P.limiter = d.flux_limiter;
    P.leapfrog = d.integrator == FCPT_INTEGRATOR_LEAPFROG;
    P.alpha_viscosity = d.viscous_alpha > 0;
    P.gamma = d.adiabatic_index;
    P.mu = d.mu;
    P.Rgas = d.Rgas;
    P.G = d.G;
    P.Mc = d.hydro_center_mass;
    P.sigma_sb = d.sigma_sb;
    P.c_light = d.c_light;
    P.aspect_ratio = d.aspect_ratio;
    P.flaring_index = d.flaring_index;
    P.tmin = d.minimum_temperature;
    P.cooling_surface = d.cooling_surface;
    P.opacity = d.opacity;
    P.cooling_beta = d.cooling_beta;
    P.cooling_beta_reference = d.cooling_beta_reference;
    P.cooling_radiative_factor = d.cooling_radiative_factor;
    P.kappa_const = d.kappa_const;
    P.kappa_factor = d.kappa_factor;
    P.tau_factor = d.tau_factor;
    P.tau_min = d.tau_min;
    P.density_factor = d.density_factor;
    P.cooling_beta_value = d.cooling_beta_value;
    P.cooling_beta_ramp_up = d.cooling_beta_ramp_up;
    P.temperature_cgs = d.temperature_cgs;
    P.density_cgs = d.density_cgs;
    P.opacity_cgs = d.opacity_cgs;
    P.emin_fac = d.minimum_temperature / d.mu * d.Rgas / (d.adiabatic_index - 1.0);
    P.emax_fac = d.maximum_temperature / d.mu * d.Rgas / (d.adiabatic_index - 1.0);
    P.b_fac = d.mu * (d.adiabatic_index - 1.0) / d.Rgas;
    P.alpha_fac = 2.0 * 4.0 * d.sigma_sb / d.c_light;
    P.tmax = d.maximum_temperature;
    P.sigma_floor_abs = d.sigma_floor * d.sigma0;
    P.sigma_floor_rel = d.sigma_floor;
    P.sigma0_val = d.sigma0;
    P.alpha = d.viscous_alpha;
    P.nu_const = d.constant_viscosity;
    P.radial_viscosity_factor = d.radial_viscosity_factor;
    P.art_visc_factor = d.artificial_viscosity_factor;
    P.heating_viscous_factor = d.heating_viscous_factor;
    P.omega_frame = d.omega_frame;
    P.thickness_smoothing = d.thickness_smoothing;
    P.cfl = d.cfl;
    P.cfl_max_var = d.cfl_max_var;
    P.heating_cooling_cfl_limit = d.heating_cooling_cfl_limit;
    P.monitor_timestep = d.monitor_timestep;
    for (int k = 0; k < 2; ++k) {
        P.bc_sigma[k] = d.bc_sigma[k];
        P.bc_energy[k] = d.bc_energy[k];
        P.bc_vrad[k] = d.bc_vrad[k];
        P.bc_vaz[k] = d.bc_vaz[k];
        P.kep_vaz[k] = d.keplerian_vaz_factor[k];
        P.kep_vrad[k] = d.keplerian_vrad_factor[k];
    }
    // default body: the central star at the origin
    P.nbodies = 1;
    P.bm[0] = d.hydro_center_mass;
}

} // namespace fcpt

using namespace fcpt;

namespace {

// one table of `t` as rows x cols doubles (fargocpt_hip.h: FCPT_TABLE_*); the column count of the selection
int table_columns(const RingTables &t, int nr, int table, std::vector<double> &v)
{
    auto rows_of = [&v](const auto &rows, int cols) { // row structs of doubles only
        v.resize(rows.size() * (size_t)cols);
        if (!rows.empty())
            std::memcpy(v.data(), rows.data(), v.size() * sizeof(double));
        return cols;
    };
    switch (table) {
    case FCPT_TABLE_SRC:
        return rows_of(t.src, (int)(sizeof(SrcRow) / sizeof(double)));
    case FCPT_TABLE_RAD:
        return rows_of(t.rad, (int)(sizeof(RadRow) / sizeof(double)));
    case FCPT_TABLE_THETA:
        return rows_of(t.theta, (int)(sizeof(ThetaRow) / sizeof(double)));
    case FCPT_TABLE_DAMP:
        for (const DampRow &r : t.damp_rows)
            v.insert(v.end(), {r.fs, r.ts, r.fv, r.tv, (double)r.tvr, (double)r.tva, (double)r.tsg, (double)r.ten, r.pad[0], r.pad[1]});
        return 10;
    case FCPT_TABLE_RING: {
        auto at = [](const auto &a, int i) { return i < (int)a.size() ? (double)a[i] : 0.0; };
        for (int i = 0; i < nr + 2; ++i)
            v.insert(v.end(), {at(t.cs_ring, i), at(t.nu_ring, i), at(t.g_dxtheta, i), at(t.g_inv_dxtheta, i), at(t.g_dr_invsurf, i),
                               at(t.g_r_omega, i), at(t.g_inv_omk, i), at(t.g_omk, i), at(t.g_ra3, i), at(t.fs, i), at(t.ts, i),
                               at(t.fv, i), at(t.tv, i), at(t.dtype[0], i), at(t.dtype[1], i), at(t.dtype[2], i), at(t.dtype[3], i),
                               at(t.ring_ref_damped, i)});
        return 18;
    }
    case FCPT_TABLE_DAMP_RANGES:
        for (int q = 0; q < 4; ++q)
            for (int o = 0; o < 2; ++o) {
                const DampRange &r = t.damp[q][o];
                v.insert(v.end(), {(double)r.lo, (double)r.hi, (double)r.type, r.rlim, r.redge, r.tau});
            }
        v.insert(v.end(), {t.damp_any ? 1.0 : 0.0, t.damp_foldable ? 1.0 : 0.0, 0.0, 0.0, 0.0, 0.0});
        return 6;
    case FCPT_TABLE_AZIMUTH:
        for (size_t j = 0; j < t.cosphi.size(); ++j)
            v.insert(v.end(), {t.cosphi[j], t.sinphi[j]});
        return 2;
    case FCPT_TABLE_TF:
        for (const TfRow &r : t.tf)
            v.insert(v.end(), {r.dr_lo, r.dr_hi, r.idr_up, r.invsurf, r.dxtheta, r.inv_dxtheta, r.invr, r.r_omega, r.r_next, r.romega_next,
                               (double)r.tvr, (double)r.tva, (double)r.tsg, (double)r.ten, r.gphi, r.dr_invsurf});
        return 16;
    }
    return 0;
}

} // namespace

// test hook: the per-ring tables of fcpt_create as pure host logic
extern "C" int fcpt_selftest_ring_tables(const fcpt_desc *d, const double *radii, int32_t table, double *out, int64_t capacity,
                                         int32_t *rows, int32_t *cols)
{
    if (!rows || !cols || capacity < 0 || (capacity > 0 && !out)) {
        set_error("null argument");
        return FCPT_EINVAL;
    }
    if (int rc = validate_create(d, radii))
        return rc;
    fcpt_split s;
    if (int rc = split_domain(*d, s))
        return rc;
    HostGeometry g;
    build_geometry(*d, s, radii, g);
    RingTables t;
    build_ring_tables(*d, s, g, t);
    std::vector<double> v;
    const int nc = table_columns(t, s.nr, table, v);
    if (!nc) {
        set_error("fcpt_selftest_ring_tables: unknown table %d", (int)table);
        return FCPT_EINVAL;
    }
    *cols = nc;
    *rows = (int32_t)(v.size() / (size_t)nc);
    if (capacity > 0)
        std::memcpy(out, v.data(), std::min(v.size(), (size_t)capacity) * sizeof(double));
    return FCPT_OK;
}
