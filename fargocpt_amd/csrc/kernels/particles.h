// Part of fcpt_kernels.hip (one translation unit, namespace fcpt): Lagrangian dust particles with gas drag
// and turbulent diffusion.
// Not a stand-alone header: included once, in the order given there.
//
// k_particles_step restates, per particle and statement by statement (paths relative to the reference's src/):
//   update_velocities_from_indirect_term  particles/particles.cpp:1326-1341  (polar form)
//   integrate_exponential_midpoint        particles/particles.cpp:1579-1672  (Zhu et al. 2014, Mignone et al. 2019)
//     calculate_gas_drag_expmid :1247-1273, interpolate_quantities :1216-1244, find_nearest :115-133,
//     interpolate_bilinear :1062-1127, calc_tstop :1130-1214, calculate_dust_smoothing :896-912,
//     calculate_derivitives_from_star_and_planets(_in_cart) :981-1060
//   the escape test of move()             particles/particles.cpp:2019-2031
//   rotate                                particles/particles.cpp:2394-2395
//   diffuse_dust, kick_length             particles/dust_diffusion.cpp:29-97, with the deviate of kernels/philox.h
//   check_tstop                           particles/particles.cpp:1277-1311  (drag off, diffusion on)
//
// Shape: one lane per live particle, structure-of-arrays state, no atomics, no LDS, no waits between workgroups.
// The ring and column of a particle differ from lane to lane, so the per-ring arrays are read through plain vector
// loads here (the ROWU / readfirstlane promotion of the grid kernels does not apply), and the gathers from the
// phi-contiguous grids are element-granular: what keeps them cheap is the order of the particles, which the kernel
// does not choose (fcpt_particles_set keeps the caller's order).  Bodies and scalars arrive as kernel arguments.
//
// rho = Sigma / (density_factor H) and T are formed in registers at the corners of the interpolation cell from
// Sigma (and e for the ideal EOS) with the expressions of k_iso_cs_h / k_temperature / k_adi_derived; no RHO or
// TEMPERATURE grid is read.
//
// DEPARTURE from the reference: for a particle beyond Rmed[Nr-1] the reference reads row Nr of a scalar grid, which
// is out of bounds.  Here the lower row of the b grid (cell centres) is clamped to [0, Nr-2] -- linear extrapolation
// from the last two rows, the mirror of what the reference's release build does below Rmed[0] -- and the lower row
// of the a grid (interfaces) to [0, Nr-1].

// particles.cpp:84-95
__device__ __forceinline__ double particle_check_angle(double phi)
{
    if (phi >= 2.0 * M_PI)
        return phi - 2.0 * M_PI;
    if (phi < 0.0)
        return phi + 2.0 * M_PI;
    return phi;
}

// Largest i in [0, nr-1] with Rinf[i] <= r (get_rinf_id with the release build's clamp).  The closed form of the
// spacing gives the guess; where it is off (rounding at an interface, a radii array of the caller's own) a binary
// search over the context's array decides, so the result is right for any monotonic grid.
// SLAB: the context is one of several slabs (fcpt_particles_slabs).  cf_rmin is the global Rmin, so the closed form counts
// global rows: the slab's first row, A.row0, comes off the guess, in integers, before it is checked against the local Rinf.
template <bool SLAB = false>
__device__ __forceinline__ int particle_rinf_id(const double *Rinf, int nr, const ParticleArgs &A, double r)
{
    double did;
    if (A.spacing == FCPT_SPACING_LOGARITHMIC)
        did = log(r / A.cf_rmin) * A.cf_inv_log_growth;
    else if (A.spacing == FCPT_SPACING_ARITHMETIC)
        did = (r - A.cf_rmin) * A.cf_growth;
    else
        did = log((r - A.cf_rmin) * A.cf_opt_const + 1.0) * A.cf_inv_log_growth;
    int g;
    if (SLAB)
        g = (int)floor(dmin(dmax(did, -1.0), (double)(A.row0 + nr))) + 1 - A.row0;
    else
        g = (int)floor(dmin(dmax(did, -1.0), (double)nr)) + 1;
    g = g < 0 ? 0 : (g > nr - 1 ? nr - 1 : g);
    if (Rinf[g] <= r && (g == nr - 1 || r < Rinf[g + 1]))
        return g;
    int lo = 0, hi = nr - 1; // invariant: the answer is in [lo, hi]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (Rinf[mid] <= r)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// Sigma, T and H of cell (i, j) as the derived-quantity kernels form them
struct ParticleGas {
    double rho, T;
};
template <bool ADI> __device__ __forceinline__ double particle_scale_height(const Dev &P, int i, int j)
{
    if (!ADI)
        return P.cs_ring.p[i] * P.g_inv_omk.p[i];
    const double cs = sqrt(P.gamma * (P.gamma - 1.0) * P.energy[IDX(i, j)] / P.sigma[IDX(i, j)]);
    return cs / sqrt(P.gamma) * P.g_inv_omk.p[i];
}
template <bool ADI> __device__ __forceinline__ ParticleGas particle_gas(const Dev &P, int i, int j)
{
    const double sg = P.sigma[IDX(i, j)];
    ParticleGas g;
    if (ADI) {
        const double e = P.energy[IDX(i, j)];
        const double cs = sqrt(P.gamma * (P.gamma - 1.0) * e / sg);
        const double H = cs / sqrt(P.gamma) * P.g_inv_omk.p[i];
        g.T = P.mu / P.Rgas * (P.gamma - 1.0) * e / sg;
        g.rho = sg / (P.density_factor * H);
    } else {
        const double cs = P.cs_ring.p[i];
        g.T = P.mu / P.Rgas * (cs * cs);
        g.rho = sg / (P.density_factor * (cs * P.g_inv_omk.p[i]));
    }
    return g;
}
// particles.cpp:1116-1124
__device__ __forceinline__ double particle_bilinear(double Qmm, double Qpm, double Qmp, double Qpp, double rm, double rp, double phim,
                                                    double phip, double dphi, double r, double phi)
{
    const double Qm = ((phip - phi) * Qmm + (phi - phim) * Qmp) / dphi;
    const double Qp = ((phip - phi) * Qpm + (phi - phim) * Qpp) / dphi;
    return ((rp - r) * Qm + (r - rm) * Qp) / (rp - rm);
}

// The gas at (r_tmp, phi1), r_tmp inside the grid: find_nearest + the four bilinear interpolations of
// interpolate_quantities (:1216-1244).  ib_raw and ja are the cell of calculate_dust_smoothing.
struct ParticleGasAt {
    double rho, temperature, vg_radial, vg_azimuthal;
    int ib_raw, ja;
};
template <bool ADI, bool SLAB = false>
__device__ __forceinline__ ParticleGasAt particle_interpolate(const Dev &P, const ParticleArgs &A, double r_tmp, double phi1)
{
    const int nr = P.nr, nphi = P.nphi;
    const double *Rinf = P.Rinf.p, *Rmed = P.Rmed.p;
    const int ia = particle_rinf_id<SLAB>(Rinf, nr, A, r_tmp);
    const int ib_raw = r_tmp >= Rmed[ia] ? ia : ia - 1; // Rinf[ia] < Rmed[ia] < Rinf[ia+1]
    const int ib = ib_raw < 0 ? 0 : (ib_raw > nr - 2 ? nr - 2 : ib_raw);
    // (phi1 is in [0, 2 pi]: where the product rounds up to nphi the particle still belongs to the last column)
    int ja = (int)floor(phi1 * P.invdphi);
    ja = ja < 0 ? 0 : (ja > nphi - 1 ? nphi - 1 : ja);
    const int jap = ja == nphi - 1 ? 0 : ja + 1;
    int jb = (int)floor((phi1 - 0.5 * P.dphi) * P.invdphi) % nphi;
    jb = jb < 0 ? jb + nphi : jb;
    const int jbp = jb == nphi - 1 ? 0 : jb + 1;
    // cell-centred columns: the three cases at the seam (particles.cpp:1096-1113)
    double phim_b, phip_b;
    if (jb == nphi - 1) {
        if (phi1 < M_PI) {
            phim_b = -0.5 * P.dphi;
            phip_b = 0.5 * P.dphi;
        } else {
            phim_b = (jb + 0.5) * P.dphi;
            phip_b = (jb + 1.5) * P.dphi;
        }
    } else {
        phim_b = (jb + 0.5) * P.dphi;
        phip_b = (jbp + 0.5) * P.dphi;
    }
    const double phim_a = ja * P.dphi, phip_a = (double)(ja + 1) * P.dphi; // :1085-1094
    const double rbm = Rmed[ib], rbp = Rmed[ib + 1], ram = Rinf[ia], rap = Rinf[ia + 1];

    const ParticleGas gmm = particle_gas<ADI>(P, ib, jb), gpm = particle_gas<ADI>(P, ib + 1, jb);
    const ParticleGas gmp = particle_gas<ADI>(P, ib, jbp), gpp = particle_gas<ADI>(P, ib + 1, jbp);
    ParticleGasAt g;
    g.rho = particle_bilinear(gmm.rho, gpm.rho, gmp.rho, gpp.rho, rbm, rbp, phim_b, phip_b, P.dphi, r_tmp, phi1);
    g.temperature = particle_bilinear(gmm.T, gpm.T, gmp.T, gpp.T, rbm, rbp, phim_b, phip_b, P.dphi, r_tmp, phi1);
    g.vg_radial = particle_bilinear(P.vrad[IDX(ia, jb)], P.vrad[IDX(ia + 1, jb)], P.vrad[IDX(ia, jbp)], P.vrad[IDX(ia + 1, jbp)], ram, rap,
                                    phim_b, phip_b, P.dphi, r_tmp, phi1);
    g.vg_azimuthal = particle_bilinear(P.vazi[IDX(ib, ja)], P.vazi[IDX(ib + 1, ja)], P.vazi[IDX(ib, jap)], P.vazi[IDX(ib + 1, jap)], rbm,
                                       rbp, phim_a, phip_a, P.dphi, r_tmp, phi1) +
                     r_tmp * P.omega_frame;
    g.ib_raw = ib_raw;
    g.ja = ja;
    return g;
}

// calc_tstop (:1130-1214) -> the number of the reference's die() guard that trips (:1163-1208), or 0 and tstop
__device__ __forceinline__ int particle_calc_tstop(const ParticleArgs &A, double radius, double rho, double vrel, double temperature,
                                                   double &tstop)
{
    const double m0 = A.molecule_mass, a0 = A.molecule_radius;
    const double vthermal = sqrt(8.0 * A.k_B * temperature / (M_PI * m0));
    const double cross_section = M_PI * (a0 * a0);
    const double nu = 1.0 / 3.0 * m0 * vthermal / cross_section;
    const double l = m0 / M_PI / (a0 * a0) / rho;
    const double c_s = vthermal * sqrt(M_PI / 8.0);
    const double Kn = 0.5 * l / radius;
    const double Ma = vrel / c_s;
    const double Re = 2.0 * radius * rho * vrel / nu;
    const double CdE = 2.0 * sqrt(Ma * Ma + 128.0 / 9.0 / M_PI);
    // the Stokes coefficient's four branches: the power shared by the first three is one call with selected operands
    const double pw = pow(Re <= 1.e-3 ? 2.0 * radius * rho / nu : Re, Re <= 500.0 ? -0.313 : 1.397);
    double CdS;
    if (Re <= 1.e-3)
        CdS = 24.0 * nu / (2.0 * radius * rho * c_s) + 3.6 / c_s * pow(vrel, 0.687) * pw;
    else if (Re <= 500.0)
        CdS = 24.0 * Ma / Re + 3.6 * Ma * pw;
    else if (Re <= 1500.0)
        CdS = Ma * 9.5e-5 * pw;
    else
        CdS = Ma * 2.61;
    const double Cd = (9.0 * Kn * Kn * CdE + CdS) / (3.0 * Kn + 1.0) / (3.0 * Kn + 1.0);
    int guard = 0;
    if (Ma < 1.e-20)
        guard = 1;
    else if (Ma > 1.e20)
        guard = 2;
    else if (CdE < 1.e-20)
        guard = 3;
    else if (CdE > 1.e20)
        guard = 4;
    else if (CdS < 1.e-30)
        guard = 5;
    else if (CdS > 1.e30)
        guard = 6;
    else if (Cd < 1.e-20)
        guard = 7;
    else if (Cd > 1.e20)
        guard = 8;
    if (guard)
        return guard;
    tstop = 4.0 * l * A.particle_density / (3.0 * rho * Cd * c_s * Kn);
    return 0;
}

// Cell (i, j) for the diffusion kick: rho as particle_gas forms it, and D_g = alpha c_s H
// (dust_diffusion.cpp:102-119; c_s is the sound speed of the EOS, H = c_s / (sqrt(gamma) Omega_K) for the ideal one)
template <bool ADI> __device__ __forceinline__ double particle_rho(const Dev &P, int i, int j)
{
    return particle_gas<ADI>(P, i, j).rho;
}
template <bool ADI> __device__ __forceinline__ double particle_gas_diffusion(const Dev &P, int i, int j)
{
    if (ADI) {
        const double cs = sqrt(P.gamma * (P.gamma - 1.0) * P.energy[IDX(i, j)] / P.sigma[IDX(i, j)]);
        return P.alpha * cs * (cs / sqrt(P.gamma) * P.g_inv_omk.p[i]);
    }
    const double cs = P.cs_ring.p[i];
    return P.alpha * cs * (cs * P.g_inv_omk.p[i]);
}

// Guard 11 (SLAB only; integer tests, no floating expression of the step is touched): the step needs a gas row beyond the
// slab's rings on a side that has a neighbour, where a one-slab run reads real gas and the clamps above would extrapolate.
// `row` is the lower row of a cell-centred interpolation (rows row, row + 1, and up to row + 2 of v_r, whose row nr the
// ghost exchange does not refresh: lo = 0, hi = nr - 3) or the row of the diffusion kick (rows row - 1 .. row + 1, and the
// one-slab rule that leaves d rho / dr zero in rows 0 and Nr - 1 of the GLOBAL grid: lo = 1, hi = nr - 2).  A position
// outside [Rinf[0], Rinf[nr]) of the slab ends at row -1 or nr - 1 by the clamps and trips as well.
#define PARTICLE_GUARD_OFF_SLAB 11
#define PARTICLE_GUARD_MESSAGE 12
// the guard number of a branch that exists on one slab as well: guard 11 comes first
template <bool SLAB> __device__ __forceinline__ int particle_guard(bool off_slab, int guard)
{
    return SLAB && off_slab ? PARTICLE_GUARD_OFF_SLAB : guard;
}
template <bool SLAB> __device__ __forceinline__ bool particle_off_slab(const Dev &P, int row, int lo, int hi)
{
    return SLAB && ((!P.is_first && row < lo) || (!P.is_last && row > hi));
}

// The three per-step scalars of a launch.  fcpt_particles_step passes them by value (A.step_offset is null); queued by
// fcpt_run_steps they come from the device clock, because a replayed hipGraph repeats its arguments: the step length in
// force, OmegaFrame * dt as ONE rounded product -- what the host-stepped loop passes; written inline the product could be
// contracted into the subtraction that uses it and differ in the last bit -- and the hydro-iteration count plus the offset
// fcpt_run_steps left at its entry (wrapping).  DEV is fixed at compile time, not a test of A.step_offset at run time: the
// uniform select costs the host-argument kernels up to three VGPRs, and those kernels are pinned to the bits and registers
// they had.  k_particles_step and k_particles_step_explicit take DEV as their fourth template argument.
// The clock is read ahead of the kernel's stores, through the scalar cache.
// DEV and SLAB together (fcpt_run_steps on several slabs) are k_particles_step<., ., ., true, true> and
// k_particles_step_explicit<., ., ., true, true>: the two departures touch different statements (the three scalars; the cell
// search and guard 11), so the combination keeps the bits each of them keeps.
template <bool DEV> __device__ __forceinline__ double particle_dt(const Dev &P, const ParticleArgs &A)
{
    return DEV ? P.clk->dt : A.dt;
}
template <bool DEV> __device__ __forceinline__ double particle_frame_angle(const Dev &P, const ParticleArgs &A, double dt)
{
    if (!DEV)
        return A.frame_angle;
    // (the product must be rounded on its own, as the host-stepped loop passes it: __dmul_rn is a plain product to this
    //  compiler, which would contract it with the subtraction that follows; the empty asm statement keeps them apart)
    double angle = P.omega_frame * dt;
    asm("" : "+v"(angle));
    return angle;
}
template <bool DEV> __device__ __forceinline__ unsigned long long particle_counter(const Dev &P, const ParticleArgs &A)
{
    return DEV ? *A.step_offset + P.clk->n_hydro_iter : A.step;
}

// DRAG: ParticleGasDragEnabled; DIFF: ParticleDustDiffusion (the Brownian radial kick of dust_diffusion.cpp:29-97 after
// Charnoz et al. 2011, between the midpoint step and move()).  <ADI, true, false> is the drag-only step.
// With the drag off tstop = 1e100 and exp_tstop and h1 are formed from it as the reference writes them; the Stokes
// number of the step is then 1e100 Omega_K(r3) (DIFF off, :1671) or check_tstop's (:1277-1311, DIFF on, :1549-1551):
// a second interpolation, at the end position, and calc_tstop with the velocities of the end of the step.
// DEPARTURE from the reference: rho, d rho / dr and D_g of the kick come from the current Sigma (and e); the reference
// evaluates them at init and refreshes them only under Disk: yes, from a RHO it refreshes only with the drag on.
// SLAB: one of several slabs -- the cell search counts from the slab's first row and guard 11 is held; nothing else differs.
template <bool ADI, bool DRAG, bool DIFF, bool DEV, bool SLAB = false>
__global__ void __launch_bounds__(256) k_particles_step(const Dev P, const ParticleArgs A)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= A.n || !A.alive[n])
        return;
    const double dt = particle_dt<DEV>(P, A);
    const unsigned long long clock_counter = DIFF && DEV ? particle_counter<DEV>(P, A) : 0ull; // ahead of the stores
    const double r0 = A.r[n], phi0 = A.phi[n], radius = A.radius[n], stokes_old = A.stokes[n];
    double r_dot0, phi_dot0;
    { // update_velocities_from_indirect_term
        double s, c;
        sincos(phi0, &s, &c);
        r_dot0 = A.r_dot[n] + dt * (A.indirect_x * c + A.indirect_y * s);
        phi_dot0 = A.phi_dot[n] + dt * (-A.indirect_x * s + A.indirect_y * c) / r0;
    }
    const double l0 = r0 * r0 * phi_dot0;
    const double hfdt = 0.5 * dt;
    // half drift
    const double r1 = r0 + r_dot0 * hfdt;
    const double phi1 = particle_check_angle(phi0 + 0.5 * (l0 / (r0 * r0) + l0 / (r1 * r1)) * hfdt);

    const int nr = P.nr, nphi = P.nphi;
    const double *Rinf = P.Rinf.p, *Rmed = P.Rmed.p;
    const double r_tmp = fmin(fmax(r1, Rinf[0]), Rinf[nr]); // Rsup[nr-1] = Rinf[nr]
    double tstop = 1e100, minus_r_dotel_r = 0.0, minus_l_rel = 0.0;
    int ib_raw, ja;
    bool off_slab = false; // guard 11 (SLAB): joins the guards of calc_tstop where they branch, or waits for the stores
    if (DRAG) {
        const ParticleGasAt g = particle_interpolate<ADI, SLAB>(P, A, r_tmp, phi1);
        ib_raw = g.ib_raw;
        ja = g.ja;
        off_slab = particle_off_slab<SLAB>(P, ib_raw, 0, nr - 3);
        // calculate_gas_drag_expmid
        minus_r_dotel_r = g.vg_radial - r_dot0;
        minus_l_rel = r1 * g.vg_azimuthal - l0;
        const double vrel_phi = g.vg_azimuthal - phi_dot0 * r0;
        const double vrel = sqrt(minus_r_dotel_r * minus_r_dotel_r + vrel_phi * vrel_phi);
        // the reference's die() guards: the particle stays as it was and is reported
        if (const int guard = particle_guard<SLAB>(off_slab, particle_calc_tstop(A, radius, g.rho, vrel, g.temperature, tstop))) {
            *A.status = (unsigned long long)guard | ((unsigned long long)n << 8); // any one of the tripped particles
            return;
        }
    } else { // the cell of the smoothing length alone
        const int ia = particle_rinf_id<SLAB>(Rinf, nr, A, r_tmp);
        ib_raw = r_tmp >= Rmed[ia] ? ia : ia - 1;
        ja = (int)floor(phi1 * P.invdphi);
        ja = ja < 0 ? 0 : (ja > nphi - 1 ? nphi - 1 : ja);
        off_slab = particle_off_slab<SLAB>(P, ib_raw, 0, nr - 3);
    }

    // ---- calculate_dust_smoothing: H of cell (rmed_id(r1), inf_azimuthal_id(phi1)) ------------------------------
    const int is = ib_raw < 0 ? 0 : ib_raw; // (<= nr-1 already)
    const double H_dust = particle_scale_height<ADI>(P, is, ja) * sqrt(P.alpha / (P.alpha + stokes_old));
    const double epsilon_sq = (H_dust * P.thickness_smoothing) * (H_dust * P.thickness_smoothing);

    // ---- gravity of the bodies, star included -------------------------------------------------------------------
    double grav_r_ddot = 0.0, minus_grav_l_dot = 0.0;
    if (A.gravity_cartesian) {
        double s, c;
        sincos(phi1, &s, &c);
        const double x = r1 * c, y = r1 * s;
        double ax = 0.0, ay = 0.0;
        for (int k = 0; k < P.nbodies; ++k) {
            const double x_dist = x - P.bx[k], y_dist = y - P.by[k];
            const double dist2 = x_dist * x_dist + y_dist * y_dist + epsilon_sq;
            const double dist = sqrt(dist2);
            ax += -P.G * P.bm[k] * x_dist / (dist * dist2);
            ay += -P.G * P.bm[k] * y_dist / (dist * dist2);
        }
        grav_r_ddot = ax * c + ay * s;
        minus_grav_l_dot = (-ax * s + ay * c) * r1;
    } else {
        for (int k = 0; k < P.nbodies; ++k) {
            double s, c;
            sincos(phi1 - A.bphi[k], &s, &c);
            const double rp = A.br[k];
            const double d = sqrt(r1 * r1 + rp * rp - 2.0 * r1 * rp * c);
            const double d2s = d * d + epsilon_sq;
            grav_r_ddot -= P.G * P.bm[k] * (r1 - rp * c) / (d2s * d);
            minus_grav_l_dot -= P.G * P.bm[k] * r1 * rp * s / (d2s * d);
        }
    }

    // ---- kick: exponential propagator (Mignone et al. 2019, eq. 33) ---------------------------------------------
    const double exp_tstop = exp(-dt / tstop);
    const double h1 = tstop * (-expm1(-dt / tstop));
    double l2 = exp_tstop * l0 + h1 * minus_grav_l_dot;
    if (DRAG)
        l2 += h1 * (minus_l_rel + l0) / tstop;
    double r_dot2 = exp_tstop * r_dot0;
    r_dot2 += h1 * 0.5 * (l0 * l0 + l2 * l2) / (r1 * r1 * r1);
    r_dot2 += h1 * grav_r_ddot;
    if (DRAG)
        r_dot2 += h1 * (minus_r_dotel_r + r_dot0) / tstop;
    // second half drift
    const double r3 = r1 + r_dot2 * hfdt;
    double phi3 = particle_check_angle(phi1 + 0.5 * (l2 / (r1 * r1) + l2 / (r3 * r3)) * hfdt);
    if (!DIFF) {
        if (SLAB && !DRAG && off_slab) {
            *A.status = (unsigned long long)PARTICLE_GUARD_OFF_SLAB | ((unsigned long long)n << 8);
            return;
        }
        // move(): escaped particles leave; rotate(): the frame's turn over the step
        const double r3sq = r3 * r3;
        if (r3sq > A.escape_max_sq || r3sq < A.escape_min_sq)
            A.alive[n] = 0;
        phi3 = particle_check_angle(phi3 - particle_frame_angle<DEV>(P, A, dt));
        A.r[n] = r3;
        A.phi[n] = phi3;
        A.r_dot[n] = r_dot2;
        A.phi_dot[n] = l2 / r3sq;
        A.stokes[n] = tstop * sqrt(P.G * P.Mc / (r3 * r3 * r3));
        return;
    }
    const double phi_dot3 = l2 / (r3 * r3);
    const double omega_k3 = sqrt(P.G * P.Mc / (r3 * r3 * r3));
    if (!DRAG) { // check_tstop at the end position
        const ParticleGasAt g = particle_interpolate<ADI, SLAB>(P, A, fmin(fmax(r3, Rinf[0]), Rinf[nr]), phi3);
        off_slab = off_slab || particle_off_slab<SLAB>(P, g.ib_raw, 0, nr - 3);
        const double dv_r = g.vg_radial - r_dot2;
        const double dv_phi = g.vg_azimuthal - phi_dot3 * r3;
        if (const int guard = particle_guard<SLAB>(
                off_slab, particle_calc_tstop(A, radius, g.rho, sqrt(dv_r * dv_r + dv_phi * dv_phi), g.temperature, tstop))) {
            *A.status = (unsigned long long)guard | ((unsigned long long)n << 8);
            return;
        }
    }
    const double stokes = tstop * omega_k3;
    // ---- diffuse_dust / kick_length: values of the particle's cell, no interpolation -------------------------------
    const double St2 = stokes * stokes;
    const double Sc = (1.0 + St2) * (1.0 + St2) / (1.0 + 4.0 * St2); // Youdin & Lithwick 2007, eq. 37
    const int ik = particle_rinf_id<SLAB>(Rinf, nr, A, r3);
    const bool off_kick = particle_off_slab<SLAB>(P, ik, 1, nr - 2);
    int jk = (int)floor(phi3 * P.invdphi);
    jk = jk < 0 ? 0 : (jk > nphi - 1 ? nphi - 1 : jk);
    const double Dd = particle_gas_diffusion<ADI>(P, ik, jk) / Sc;
    const double rho = particle_rho<ADI>(P, ik, jk);
    // compute_gas_density_radial_derivative: rows 0 and Nr-1 stay zero
    double drho_dr = 0.0;
    if (ik >= 1 && ik <= nr - 2)
        drho_dr = (particle_rho<ADI>(P, ik + 1, jk) - particle_rho<ADI>(P, ik - 1, jk)) / (Rmed[ik + 1] - Rmed[ik - 1]);
    const double mean = Dd / rho * drho_dr * dt * dt * omega_k3;
    const double sigma = sqrt(2.0 * Dd * dt);
    const double snv = particle_std_normal(A.seed, A.id[n], DEV ? clock_counter : A.step);
    const double q = sigma * snv / r3;
    const double corr_2d = r3 * (sqrt(1.0 + q * q) - 1.0); // the missing diffusion tangential to r
    const double r4 = r3 + (mean + snv * sigma + corr_2d);
    if (SLAB && off_kick) { // (ahead of the first store)
        *A.status = (unsigned long long)PARTICLE_GUARD_OFF_SLAB | ((unsigned long long)n << 8);
        return;
    }
    // move() on the kicked radius (r4 <= 0 has left as well); rotate()
    const double r4sq = r4 * r4;
    if (r4sq > A.escape_max_sq || r4sq < A.escape_min_sq || !(r4 > 0.0))
        A.alive[n] = 0;
    phi3 = particle_check_angle(phi3 - particle_frame_angle<DEV>(P, A, dt));
    A.r[n] = r4;
    A.phi[n] = phi3;
    A.r_dot[n] = r_dot2;
    A.phi_dot[n] = phi_dot3 * pow(r3 / r4, 1.5); // a circular orbit stays one
    A.stokes[n] = stokes;
}

// the deviates of fcpt_particles_normals: what k_particles_step<., ., true> draws at counter `step`, per slot
__global__ void __launch_bounds__(256) k_particles_normals(int n, const unsigned long long *id, unsigned long long seed,
                                                           unsigned long long step, double *snv)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < n)
        snv[k] = particle_std_normal(seed, id[k], step);
}

// particle_counter()'s offset: the counter of the call's first step minus the iteration count it starts at (wrapping)
__global__ void k_particles_counter_offset(unsigned long long *offset, unsigned long long counter, const DevClock *clk)
{
    *offset = counter - clk->n_hydro_iter;
}

// ---------------------------------------------------------------------------------------------------------------------
// ParticleIntegrator: explicit -- integrate_explicit_adaptive (particles/particles.cpp:1677-2014): an explicit drag kick,
// then an embedded Cash-Karp RK5(4) with a step size per particle.  Restated statement by statement:
//   update_velocities_from_indirect_term       :1314-1343 (polar, or :1322-1324 with CART)
//   update_velocities_from_gas_drag(_cart)     :1428-1504 (:1345-1418)
//   the adaptive loop                          :1693-2012, calculate_dust_smoothing :896-912,
//     calculate_accelerations_from_star_and_planets(_cart) :914-952 (:954-979), softening inside the square root
//   the escape test of move()                  :2019-2031 (x^2 + y^2 with CART)
//   rotate                                     :2369-2397
//   init_particle_timestep                     :248-374 (k_particles_timestep_init)
// CART: CartesianParticles -- r, phi, r_dot, phi_dot hold x, y, v_x, v_y.
// The state lives in registers and is written once, at the end: a particle that trips a guard stays exactly as it was,
// timestep and facold included.  Guards 1..8 are calc_tstop's; two more:
//   9   the attempt cap.  The reference's while (!last) has no bound: a NaN or zero step spins for ever.  Here accepted
//       plus rejected substeps are counted in an integer and capped at max_attempts.
//   10  t_stop < 10 dt in the drag kick.  DEPARTURE: check_tstop (:1303-1309) exits the reference on this condition once,
//       at start-up; here it is held at every step.
// The number of substeps differs from lane to lane; a wavefront runs as long as its slowest lane.

#define PARTICLES_EXPLICIT_BLOCK 256
#define PARTICLE_GUARD_ATTEMPTS 9
#define PARTICLE_GUARD_STIFF 10

// t_particle::get_angle with CartesianParticles (particle.cpp:25-39)
__device__ __forceinline__ double particle_angle_cart(double x, double y)
{
    const double phi = atan2(y, x);
    return phi < 0.0 ? phi + 2.0 * M_PI : phi;
}

// d(velocity)/dt from all bodies, star included; (q1, q2, v1, v2) is (r, phi, r_dot, phi_dot) or (x, y, v_x, v_y)
template <bool CART>
__device__ __forceinline__ void particle_accel(const Dev &P, const ParticleArgs &A, double q1, double q2, double v1, double v2,
                                               double epsilon_sq, double &a1, double &a2)
{
    if (CART) {
        a1 = 0.0;
        a2 = 0.0;
        for (int k = 0; k < P.nbodies; ++k) {
            const double dx = P.bx[k] - q1, dy = P.by[k] - q2;
            double r2 = dx * dx + dy * dy;
            r2 += epsilon_sq;
            const double r = sqrt(r2);
            const double factor = P.G * P.bm[k] / (r * r2);
            a1 += factor * dx;
            a2 += factor * dy;
        }
    } else {
        a1 = q1 * v2 * v2; // centrifugal
        a2 = -2.0 * v1 / q1 * v2;
        for (int k = 0; k < P.nbodies; ++k) {
            double s, c;
            sincos(q2 - A.bphi[k], &s, &c);
            const double rp = A.br[k];
            const double d = sqrt(q1 * q1 + rp * rp - 2.0 * q1 * rp * c + epsilon_sq);
            const double factor = P.G * P.bm[k] / (d * (d * d));
            a1 -= factor * (q1 - rp * c);
            a2 -= factor * rp * s / q1;
        }
    }
}

// DEV false: dt and frame_angle are kernel arguments; true: they come from the device clock (particle_dt).  SLAB: one of
// several slabs (fcpt_particles_slabs) -- the slab's cell search and guard 11 (particle_rinf_id, particle_off_slab); nothing
// else differs.  DEV and SLAB together: fcpt_run_steps on several slabs.
template <bool ADI, bool DRAG, bool CART, bool DEV = false, bool SLAB = false>
__global__ void __launch_bounds__(PARTICLES_EXPLICIT_BLOCK)
    k_particles_step_explicit(const Dev P, const ParticleArgs A, const ParticleAdaptive X)
{
    const int n = blockIdx.x * PARTICLES_EXPLICIT_BLOCK + threadIdx.x;
    if (n >= A.n || !A.alive[n])
        return;
    const double dt = particle_dt<DEV>(P, A);
    const int nr = P.nr, nphi = P.nphi;
    const double *Rinf = P.Rinf.p, *Rmed = P.Rmed.p;
    double q1 = A.r[n], q2 = A.phi[n], v1 = A.r_dot[n], v2 = A.phi_dot[n], stokes = A.stokes[n];
    double h = X.timestep[n], facold = X.facold[n];

    // ---- update_velocities_from_indirect_term ------------------------------------------------------------------------
    if (CART) {
        v1 = A.indirect_x * dt + v1;
        v2 = A.indirect_y * dt + v2;
    } else {
        double s, c;
        sincos(q2, &s, &c);
        const double v1_old = v1;
        v1 = v1_old + dt * (A.indirect_x * c + A.indirect_y * s);
        v2 = v2 + dt * (-A.indirect_x * s + A.indirect_y * c) / q1;
    }

    // ---- update_velocities_from_gas_drag(_cart) ----------------------------------------------------------------------
    if (DRAG) {
        const double r = CART ? sqrt(q1 * q1 + q2 * q2) : q1;
        const double phi = CART ? particle_angle_cart(q1, q2) : q2;
        if (!((r < X.rmin) || (r > X.rmax))) { // RMIN, RMAX: inside [Rinf[0], Rinf[nr]]
            const ParticleGasAt g = particle_interpolate<ADI, SLAB>(P, A, r, phi);
            const bool off_slab = particle_off_slab<SLAB>(P, g.ib_raw, 0, nr - 3);
            double vrel_1, vrel_2, s = 0.0, c = 1.0;
            if (CART) {
                sincos(phi, &s, &c);
                const double vg_x = c * g.vg_radial - s * g.vg_azimuthal;
                const double vg_y = s * g.vg_radial + c * g.vg_azimuthal;
                vrel_1 = v1 - vg_x;
                vrel_2 = v2 - vg_y;
            } else {
                vrel_1 = v1 - g.vg_radial;
                vrel_2 = r * v2 - g.vg_azimuthal;
            }
            const double vrel = sqrt(vrel_1 * vrel_1 + vrel_2 * vrel_2);
            double tstop;
            int guard = particle_calc_tstop(A, A.radius[n], g.rho, vrel, g.temperature, tstop);
            if (!guard && tstop < 10.0 * dt)
                guard = PARTICLE_GUARD_STIFF;
            guard = particle_guard<SLAB>(off_slab, guard);
            if (guard) {
                *A.status = (unsigned long long)guard | ((unsigned long long)n << 8);
                return;
            }
            if (CART) {
                v1 += dt * (-vrel_1 / tstop);
                v2 += dt * (-vrel_2 / tstop);
            } else {
                v1 += dt * (-vrel_1 / tstop);
                v2 += dt * (-vrel_2 / r / tstop);
            }
            stokes = tstop * sqrt(P.G * P.Mc / (r * r * r));
        }
    }

    // ---- the adaptive loop -------------------------------------------------------------------------------------------
    const double beta = 0.04, fac1 = 0.2, fac2 = 10.0, safe = 0.9;
    const double expo1 = 0.2 - beta * 0.75;
    const double facc1 = 1.0 / fac1, facc2 = 1.0 / fac2;
    const double e1 = 37.0 / 378.0 - 2825.0 / 27648.0;
    const double e3 = 250.0 / 621.0 - 18575.0 / 48384.0;
    const double e4 = 125.0 / 594.0 - 13525 / 55296.0;
    const double e5 = -277.0 / 14336.0;
    const double e6 = 512.0 / 1771.0 - 1.0 / 4.0;
    const double atoli = 1e-14, rtoli = 1e-12;
    const double smoothing_factor = sqrt(P.alpha / (P.alpha + stokes)) * P.thickness_smoothing; // the Stokes number is fixed here
    double a1_out = 0.0, a2_out = 0.0;
    double elapsed = 0.0; // dt_particle_temp
    bool last = false, reject = false;
    unsigned int accepted = 0, rejected = 0;
    const unsigned int cap = (unsigned int)X.max_attempts;
    bool off_substep = false; // guard 11 (SLAB): a substep's cell beyond the slab's rings; leaves with guard 9's branch
    while (!last) {
        // guard 9: an integer comparison, which no NaN in h, err or the state can defeat
        if (accepted + rejected >= cap || (SLAB && off_substep)) {
            *A.status = (unsigned long long)particle_guard<SLAB>(off_substep, PARTICLE_GUARD_ATTEMPTS) | ((unsigned long long)n << 8);
            return;
        }
        double ts = h; // timestep; h is particles[i].timestep, which old_timestep aliases (:1726)
        bool update_timestep = true;
        if (elapsed + ts * 1.01 > dt) {
            ts = dt - elapsed;
            last = true;
            update_timestep = false;
        }
        // calculate_dust_smoothing at the current position
        double epsilon_sq;
        {
            const double r = CART ? sqrt(q1 * q1 + q2 * q2) : q1;
            const double phi = CART ? particle_angle_cart(q1, q2) : q2;
            const int ia = particle_rinf_id<SLAB>(Rinf, nr, A, r);
            int is = r >= Rmed[ia] ? ia : ia - 1; // get_rmed_id with the release build's clamp
            off_substep = off_substep || particle_off_slab<SLAB>(P, is, 0, nr - 3);
            is = is < 0 ? 0 : is;
            int ja = (int)floor(phi * P.invdphi);
            ja = ja < 0 ? 0 : (ja > nphi - 1 ? nphi - 1 : ja);
            const double rsmooth = particle_scale_height<ADI>(P, is, ja) * smoothing_factor;
            epsilon_sq = rsmooth * rsmooth;
        }
        // Cash-Karp: k?_q = velocity, k?_v = acceleration of stage ?
        double k1_q1 = v1, k1_q2 = v2, k1_v1, k1_v2;
        particle_accel<CART>(P, A, q1, q2, v1, v2, epsilon_sq, k1_v1, k1_v2);

        double t_q1 = q1 + ts * 0.2 * k1_q1, t_q2 = q2 + ts * 0.2 * k1_q2;
        double t_v1 = v1 + ts * 0.2 * k1_v1, t_v2 = v2 + ts * 0.2 * k1_v2;
        double k2_q1 = t_v1, k2_q2 = t_v2, k2_v1, k2_v2;
        particle_accel<CART>(P, A, t_q1, t_q2, t_v1, t_v2, epsilon_sq, k2_v1, k2_v2);

        t_q1 = q1 + ts * (0.075 * k1_q1 + 0.225 * k2_q1);
        t_q2 = q2 + ts * (0.075 * k1_q2 + 0.225 * k2_q2);
        t_v1 = v1 + ts * (0.075 * k1_v1 + 0.225 * k2_v1);
        t_v2 = v2 + ts * (0.075 * k1_v2 + 0.225 * k2_v2);
        const double k3_q1 = t_v1, k3_q2 = t_v2;
        double k3_v1, k3_v2;
        particle_accel<CART>(P, A, t_q1, t_q2, t_v1, t_v2, epsilon_sq, k3_v1, k3_v2);

        t_q1 = q1 + ts * (0.3 * k1_q1 - 0.9 * k2_q1 + 1.2 * k3_q1);
        t_q2 = q2 + ts * (0.3 * k1_q2 - 0.9 * k2_q2 + 1.2 * k3_q2);
        t_v1 = v1 + ts * (0.3 * k1_v1 - 0.9 * k2_v1 + 1.2 * k3_v1);
        t_v2 = v2 + ts * (0.3 * k1_v2 - 0.9 * k2_v2 + 1.2 * k3_v2);
        const double k4_q1 = t_v1, k4_q2 = t_v2;
        double k4_v1, k4_v2;
        particle_accel<CART>(P, A, t_q1, t_q2, t_v1, t_v2, epsilon_sq, k4_v1, k4_v2);

        t_q1 = q1 + ts * (-11.0 / 54.0 * k1_q1 + 2.5 * k2_q1 - 70.0 / 27.0 * k3_q1 + 35.0 / 27.0 * k4_q1);
        t_q2 = q2 + ts * (-11.0 / 54.0 * k1_q2 + 2.5 * k2_q2 - 70.0 / 27.0 * k3_q2 + 35.0 / 27.0 * k4_q2);
        t_v1 = v1 + ts * (-11.0 / 54.0 * k1_v1 + 2.5 * k2_v1 - 70.0 / 27.0 * k3_v1 + 35.0 / 27.0 * k4_v1);
        t_v2 = v2 + ts * (-11.0 / 54.0 * k1_v2 + 2.5 * k2_v2 - 70.0 / 27.0 * k3_v2 + 35.0 / 27.0 * k4_v2);
        const double k5_q1 = t_v1, k5_q2 = t_v2;
        double k5_v1, k5_v2;
        particle_accel<CART>(P, A, t_q1, t_q2, t_v1, t_v2, epsilon_sq, k5_v1, k5_v2);

        t_q1 = q1 + ts * (1631.0 / 55296.0 * k1_q1 + 175.0 / 512.0 * k2_q1 + 575.0 / 13824.0 * k3_q1 + 44275.0 / 110592.0 * k4_q1 +
                          253.0 / 4096.0 * k5_q1);
        t_q2 = q2 + ts * (1631.0 / 55296.0 * k1_q2 + 175.0 / 512.0 * k2_q2 + 575.0 / 13824.0 * k3_q2 + 44275.0 / 110592.0 * k4_q2 +
                          253.0 / 4096.0 * k5_q2);
        t_v1 = v1 + ts * (1631.0 / 55296.0 * k1_v1 + 175.0 / 512.0 * k2_v1 + 575.0 / 13824.0 * k3_v1 + 44275.0 / 110592.0 * k4_v1 +
                          253.0 / 4096.0 * k5_v1);
        t_v2 = v2 + ts * (1631.0 / 55296.0 * k1_v2 + 175.0 / 512.0 * k2_v2 + 575.0 / 13824.0 * k3_v2 + 44275.0 / 110592.0 * k4_v2 +
                          253.0 / 4096.0 * k5_v2);
        const double k6_q1 = t_v1, k6_q2 = t_v2;
        double k6_v1, k6_v2;
        particle_accel<CART>(P, A, t_q1, t_q2, t_v1, t_v2, epsilon_sq, k6_v1, k6_v2);

        // the fifth-order solution
        const double q1_new = q1 + ts * (37.0 / 378.0 * k1_q1 + 250.0 / 621.0 * k3_q1 + 125.0 / 594.0 * k4_q1 + 512.0 / 1771.0 * k6_q1);
        double q2_new = q2 + ts * (37.0 / 378.0 * k1_q2 + 250.0 / 621.0 * k3_q2 + 125.0 / 594.0 * k4_q2 + 512.0 / 1771.0 * k6_q2);
        if (!CART)
            q2_new = particle_check_angle(q2_new);
        const double a1_new = 37.0 / 378.0 * k1_v1 + 250.0 / 621.0 * k3_v1 + 125.0 / 594.0 * k4_v1 + 512.0 / 1771.0 * k6_v1;
        const double a2_new = 37.0 / 378.0 * k1_v2 + 250.0 / 621.0 * k3_v2 + 125.0 / 594.0 * k4_v2 + 512.0 / 1771.0 * k6_v2;
        const double v1_new = v1 + ts * a1_new;
        const double v2_new = v2 + ts * a2_new;

        // error estimates, in the registers of stage 2 as the reference reuses k2_*
        k2_q1 = ts * (e1 * k1_q1 + e3 * k3_q1 + e4 * k4_q1 + e5 * k5_q1 + e6 * k6_q1);
        k2_q2 = ts * (e1 * k1_q2 + e3 * k3_q2 + e4 * k4_q2 + e5 * k5_q2 + e6 * k6_q2);
        k2_v1 = ts * (e1 * k1_v1 + e3 * k3_v1 + e4 * k4_v1 + e5 * k5_v1 + e6 * k6_v1);
        k2_v2 = ts * (e1 * k1_v2 + e3 * k3_v2 + e4 * k4_v2 + e5 * k5_v2 + e6 * k6_v2);
        double err = 0.0, sqr;
        sqr = k2_q1 / (atoli + rtoli * fmax(fabs(q1), fabs(q1_new)));
        err += sqr * sqr;
        sqr = k2_q2 / (atoli + rtoli * fmax(fabs(q2), fabs(q2_new)));
        err += sqr * sqr;
        sqr = k2_v1 / (atoli + rtoli * fmax(fabs(v1), fabs(v1_new)));
        err += sqr * sqr;
        sqr = k2_v2 / (atoli + rtoli * fmax(fabs(v2), fabs(v2_new)));
        err += sqr * sqr;
        err = sqrt(err / 4.0);

        const double fac11 = pow(err, expo1);
        double fac = fac11 / pow(facold, beta); // Lund stabilisation
        fac = fmax(facc2, fmin(facc1, fac / safe));
        if (!update_timestep) // clipped to reach dt: the step does not grow
            fac = fmax(fac, 1.0);
        // AS WRITTEN IN THE REFERENCE (:1726, :1981-2007): old_timestep is a reference to particles[i].timestep, so after
        // this statement it already holds the new value.  On a rejection the stored step is therefore divided a second
        // time, and on an acceptance after a rejection the fmin of the two changes nothing.
        h = h / fac;
        if (err <= 1.0) {
            facold = fmax(err, 1.0e-4);
            elapsed += ts;
            q1 = q1_new;
            q2 = q2_new;
            v1 = v1_new;
            v2 = v2_new;
            a1_out = a1_new;
            a2_out = a2_new;
            if (reject)
                h = fmin(fabs(h), fabs(h));
            reject = false;
            ++accepted;
        } else {
            h = h / fmin(facc1, fac11 / safe);
            reject = true;
            last = false;
            ++rejected;
        }
    }

    if (SLAB && off_substep) { // (the last substep's cell)
        *A.status = (unsigned long long)PARTICLE_GUARD_OFF_SLAB | ((unsigned long long)n << 8);
        return;
    }
    // ---- move(): escaped particles leave; rotate(): the frame's turn over the step -----------------------------------
    const double rsq = CART ? q1 * q1 + q2 * q2 : q1 * q1;
    if (rsq > A.escape_max_sq || rsq < A.escape_min_sq)
        A.alive[n] = 0;
    const double frame_angle = particle_frame_angle<DEV>(P, A, dt);
    if (CART) {
        double s, c;
        sincos(frame_angle, &s, &c);
        const double x_old = q1, y_old = q2, vx_old = v1, vy_old = v2;
        q1 = x_old * c + y_old * s;
        q2 = -x_old * s + y_old * c;
        v1 = vx_old * c + vy_old * s;
        v2 = -vx_old * s + vy_old * c;
    } else {
        q2 = particle_check_angle(q2 - frame_angle);
    }
    A.r[n] = q1;
    A.phi[n] = q2;
    A.r_dot[n] = v1;
    A.phi_dot[n] = v2;
    A.stokes[n] = stokes;
    X.timestep[n] = h;
    X.facold[n] = facold;
    X.r_ddot[n] = a1_out; // (the loop ends on an accepted substep)
    X.phi_ddot[n] = a2_out;
    X.accepted[n] = accepted;
    X.rejected[n] = rejected;
}

// init_particle_timestep (:248-374): Hairer's starting step with rsmooth = 0.05, facold = 1e-4
template <bool CART> __global__ void __launch_bounds__(PARTICLES_EXPLICIT_BLOCK)
    k_particles_timestep_init(const Dev P, const ParticleArgs A, const ParticleAdaptive X)
{
    const int n = blockIdx.x * PARTICLES_EXPLICIT_BLOCK + threadIdx.x;
    if (n >= A.n || !A.alive[n])
        return;
    const double atoli = 1e-12; // (rtoli = 0: every sk is atoli)
    const double q1 = A.r[n], q2 = A.phi[n], v1 = A.r_dot[n], v2 = A.phi_dot[n];
    const double epsilon_sq = 0.05 * 0.05;
    double k1_v1, k1_v2;
    particle_accel<CART>(P, A, q1, q2, v1, v2, epsilon_sq, k1_v1, k1_v2);
    const double k1_q1 = v1, k1_q2 = v2;
    double dnf = 0.0, dny = 0.0, sqr;
    sqr = k1_q1 / atoli;
    dnf += sqr * sqr;
    sqr = q1 / atoli;
    dny += sqr * sqr;
    sqr = k1_q2 / atoli;
    dnf += sqr * sqr;
    sqr = q2 / atoli;
    dny += sqr * sqr;
    sqr = k1_v1 / atoli;
    dnf += sqr * sqr;
    sqr = v1 / atoli;
    dny += sqr * sqr;
    sqr = k1_v2 / atoli;
    dnf += sqr * sqr;
    sqr = v2 / atoli;
    dny += sqr * sqr;
    double h;
    if ((dnf <= 1.0E-10) || (dny <= 1.0E-10))
        h = 1.0E-6;
    else
        h = sqrt(dny / dnf) * 0.01;
    // an explicit Euler step
    const double t_q1 = q1 + h * k1_q1, t_q2 = q2 + h * k1_q2, t_v1 = v1 + h * k1_v1, t_v2 = v2 + h * k1_v2;
    double k2_v1, k2_v2;
    particle_accel<CART>(P, A, t_q1, t_q2, t_v1, t_v2, epsilon_sq, k2_v1, k2_v2);
    double der2 = 0.0;
    sqr = (t_v1 - k1_q1) / atoli;
    der2 += sqr * sqr;
    sqr = (t_v2 - k1_q2) / atoli;
    der2 += sqr * sqr;
    sqr = (k2_v1 - k1_v1) / atoli;
    der2 += sqr * sqr;
    sqr = (k2_v2 - k1_v2) / atoli;
    der2 += sqr * sqr;
    der2 = sqrt(der2) / h;
    const double der12 = fmax(fabs(der2), sqrt(dnf));
    double h1;
    if (der12 <= 1.0E-15)
        h1 = fmax(1.0E-6, fabs(h) * 1.0E-3);
    else
        h1 = pow(0.01 / der12, 1.0 / 5.0);
    X.timestep[n] = fmin(100.0 * h, h1);
    X.facold[n] = 1.0e-4;
}

// ---------------------------------------------------------------------------------------------------------------------
// Particles on several slabs (fcpt_particles_slabs): particles::move()'s hand-over to the radial neighbours
// (particles/particles.cpp:2033-2161).  Every slab holds every slot, so a record carries its slot index and the receiver
// searches nothing.  A message is M.inner / M.outer: word 0 the record count as a double, then M.rec doubles per record.
//
// Emigration.  The leavers of a side are served in the order of their slots: a leaver's place in the message is the number of leavers of
// that side in the slots below its own.  A leaver whose place is beyond the capacity stays, alive, for the next call, so
// with more leavers than places the lowest slots go: which ones go depends on the particles alone, never on the order in
// which wavefronts run, and two runs of one state send the same records in the same places.  Three launches:
//   k_particles_emigrate_count   workgroup b takes the M.chunk slots from b * M.chunk on (a multiple of 256, so every lane
//                                makes every pass and reaches every ballot) and stores its leavers per side, M.cnt[s][b]
//   k_particles_emigrate_finish  one workgroup: M.cnt[s][0 .. groups] becomes the running sum in front of each workgroup
//                                (the last entry the side's total); the clipped counts into word 0, the totals
//   k_particles_emigrate         a leaver's place: the sum in front of its workgroup, the leavers of the workgroup's earlier
//                                passes and of the wavefronts below in this pass, the lanes below it in the ballot (mbcnt).
//                                A workgroup without leavers returns at once, without a read of the particles.
// side of slot n: 0 leaves inwards (d^2 < lo_sq), 1 outwards (d^2 > hi_sq), -1 stays, is dead or is no slot
// (particles.cpp:2067, :2126; on an edge it stays)
__device__ __forceinline__ int particle_leaves(const ParticleArgs &A, const ParticleMigrate &M, int n)
{
    if (n >= A.n || !A.alive[n])
        return -1;
    const double q1 = A.r[n];
    double d2 = q1 * q1;
    if (M.cartesian) {
        const double q2 = A.phi[n];
        d2 = q1 * q1 + q2 * q2;
    }
    if (M.has_inner && d2 < M.lo_sq)
        return 0;
    if (M.has_outer && d2 > M.hi_sq)
        return 1;
    return -1;
}

__device__ __forceinline__ void particle_record_write(double *rec, int n, const ParticleArgs &A, const ParticleAdaptive &X, int nrec)
{
    rec[0] = (double)n;
    rec[1] = A.r[n];
    rec[2] = A.phi[n];
    rec[3] = A.r_dot[n];
    rec[4] = A.phi_dot[n];
    rec[5] = A.stokes[n];
    if (nrec == PARTICLE_RECORD_MAX) {
        rec[6] = X.timestep[n];
        rec[7] = X.facold[n];
        rec[8] = X.r_ddot[n];
        rec[9] = X.phi_ddot[n];
    }
}

__global__ void __launch_bounds__(256) k_particles_emigrate_count(const ParticleArgs A, const ParticleMigrate M)
{
    __shared__ unsigned wave_found[2][4];
    const int first = blockIdx.x * M.chunk;
    unsigned found[2] = {0u, 0u}; // (wave-uniform)
    for (int i = threadIdx.x; i < M.chunk; i += 256) {
        const int side = particle_leaves(A, M, first + i);
        found[0] += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(side == 0));
        found[1] += (unsigned)__popcll(__builtin_amdgcn_ballot_w64(side == 1));
    }
    if ((threadIdx.x & 63) == 0) {
        wave_found[0][threadIdx.x >> 6] = found[0];
        wave_found[1][threadIdx.x >> 6] = found[1];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const unsigned *w = wave_found[threadIdx.x];
        M.cnt[threadIdx.x * (PARTICLE_MIGRATE_GROUPS + 1) + blockIdx.x] = w[0] + w[1] + w[2] + w[3];
    }
}

// one workgroup of 256 lanes, behind k_particles_emigrate_count: lane t sums its stretch of the M.groups counts, takes the
// stretches below it from the LDS and writes the running sums back
__global__ void __launch_bounds__(256) k_particles_emigrate_finish(const ParticleMigrate M)
{
    __shared__ unsigned stretch[256];
    const int per = (M.groups + 255) / 256;
    const int lo = min((int)threadIdx.x * per, M.groups), hi = min(lo + per, M.groups);
    for (int s = 0; s < 2; ++s) {
        unsigned *cnt = M.cnt + s * (PARTICLE_MIGRATE_GROUPS + 1);
        unsigned sum = 0;
        for (int k = lo; k < hi; ++k)
            sum += cnt[k];
        stretch[threadIdx.x] = sum;
        __syncthreads();
        unsigned run = 0;
        for (unsigned k = 0; k < threadIdx.x; ++k)
            run += stretch[k];
        for (int k = lo; k < hi; ++k) {
            const unsigned here = cnt[k];
            cnt[k] = run;
            run += here;
        }
        if (threadIdx.x == 255) { // (its stretch is the last one: `run` is the side's total)
            cnt[M.groups] = run;
            double *msg = s == 0 ? M.inner : M.outer;
            const unsigned found = run;
            const unsigned sent = !msg ? 0u : (found < (unsigned)M.capacity ? found : (unsigned)M.capacity);
            if (msg)
                msg[0] = (double)sent;
            M.tot[s] += sent;
            M.tot[3] += found - sent;
        }
        __syncthreads(); // `stretch` is written again for the other side
    }
}

__global__ void __launch_bounds__(256) k_particles_emigrate(const ParticleArgs A, const ParticleAdaptive X, const ParticleMigrate M)
{
    __shared__ unsigned wave_found[2][4];
    const unsigned *front[2] = {M.cnt, M.cnt + PARTICLE_MIGRATE_GROUPS + 1};
    unsigned run[2] = {front[0][blockIdx.x], front[1][blockIdx.x]}; // leavers in front of this pass (workgroup-uniform)
    if (run[0] == front[0][blockIdx.x + 1] && run[1] == front[1][blockIdx.x + 1])
        return;
    const int first = blockIdx.x * M.chunk, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < M.chunk; i += 256) {
        const int n = first + i;
        const int side = particle_leaves(A, M, n);
        const unsigned long long leavers[2] = {__builtin_amdgcn_ballot_w64(side == 0), __builtin_amdgcn_ballot_w64(side == 1)};
        if ((threadIdx.x & 63) == 0) {
            wave_found[0][wave] = (unsigned)__popcll(leavers[0]);
            wave_found[1][wave] = (unsigned)__popcll(leavers[1]);
        }
        __syncthreads();
        unsigned waves_below[2] = {0u, 0u}, pass[2] = {0u, 0u};
        for (int s = 0; s < 2; ++s)
            for (int k = 0; k < 4; ++k) {
                waves_below[s] += k < wave ? wave_found[s][k] : 0u;
                pass[s] += wave_found[s][k];
            }
        if (side >= 0) {
            double *msg = side == 0 ? M.inner : M.outer;
            const unsigned long long mine = side == 0 ? leavers[0] : leavers[1];
            const unsigned below = __builtin_amdgcn_mbcnt_hi((unsigned)(mine >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mine, 0u));
            const unsigned place = (side == 0 ? run[0] + waves_below[0] : run[1] + waves_below[1]) + below;
            if (msg && place < (unsigned)M.capacity) {
                particle_record_write(msg + 1 + (size_t)place * M.rec, n, A, X, M.rec);
                A.alive[n] = 0;
            }
        }
        run[0] += pass[0];
        run[1] += pass[1];
        __syncthreads(); // wave_found is written again in the next pass
    }
}

// k_particles_immigrate: blockIdx.y is the side; the count comes from word 0 on the device.  Lane t < count scatters record
// t into its slot and sets alive.  A count that is no whole number in 0 .. capacity, or a slot index that is none in
// 0 .. n-1, writes nothing of that message / record and goes to the status word (PARTICLE_GUARD_MESSAGE).
__global__ void __launch_bounds__(256) k_particles_immigrate(const ParticleArgs A, const ParticleAdaptive X, const ParticleMigrate M)
{
    const double *msg = blockIdx.y == 0 ? M.inner : M.outer;
    if (!msg)
        return;
    const unsigned t = blockIdx.x * 256 + threadIdx.x;
    const double cnt = msg[0];
    if (!(cnt >= 0.0 && cnt <= (double)M.capacity && cnt == floor(cnt))) { // (a NaN compares false)
        if (t == 0)
            *A.status = (unsigned long long)PARTICLE_GUARD_MESSAGE | ((unsigned long long)0xffffffffu << 8);
        return;
    }
    const unsigned count = (unsigned)cnt;
    if (t == 0 && count)
        atomicAdd(&M.tot[2], (unsigned long long)count);
    if (t >= count)
        return;
    const double *rec = msg + 1 + (size_t)t * M.rec;
    const double slot = rec[0];
    if (!(slot >= 0.0 && slot < (double)A.n && slot == floor(slot))) {
        *A.status = (unsigned long long)PARTICLE_GUARD_MESSAGE | ((unsigned long long)0xffffffffu << 8);
        return;
    }
    const int n = (int)slot;
    A.r[n] = rec[1];
    A.phi[n] = rec[2];
    A.r_dot[n] = rec[3];
    A.phi_dot[n] = rec[4];
    A.stokes[n] = rec[5];
    if (M.rec == PARTICLE_RECORD_MAX) {
        X.timestep[n] = rec[6];
        X.facold[n] = rec[7];
        X.r_ddot[n] = rec[8];
        X.phi_ddot[n] = rec[9];
    }
    A.alive[n] = 1;
}
