// k_particles_step_explicit (PARTICLES_DEV false: dt and frame_angle are kernel arguments) and
// k_particles_step_explicit_clock (true: they come from the device clock), see particles.h, which includes this file once
// for each with PARTICLES_KERNEL, PARTICLES_DEV and PARTICLES_SLAB defined (k_particles_step_explicit_slab: one of several
// slabs, see particle_rinf_id and particle_off_slab; k_particles_step_explicit_slab_clock: that, reading the device clock).
template <bool ADI, bool DRAG, bool CART>
__global__ void __launch_bounds__(PARTICLES_EXPLICIT_BLOCK)
    PARTICLES_KERNEL(const Dev P, const ParticleArgs A, const ParticleAdaptive X)
{
    const int n = blockIdx.x * PARTICLES_EXPLICIT_BLOCK + threadIdx.x;
    if (n >= A.n || !A.alive[n])
        return;
    const double dt = particle_dt<PARTICLES_DEV>(P, A);
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
            const ParticleGasAt g = particle_interpolate<ADI, PARTICLES_SLAB>(P, A, r, phi);
            const bool off_slab = particle_off_slab<PARTICLES_SLAB>(P, g.ib_raw, 0, nr - 3);
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
            guard = particle_guard<PARTICLES_SLAB>(off_slab, guard);
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
    bool off_substep = false; // guard 11 (PARTICLES_SLAB): a substep's cell beyond the slab's rings; leaves with guard 9's branch
    while (!last) {
        // guard 9: an integer comparison, which no NaN in h, err or the state can defeat
        if (accepted + rejected >= cap || (PARTICLES_SLAB && off_substep)) {
            *A.status = (unsigned long long)particle_guard<PARTICLES_SLAB>(off_substep, PARTICLE_GUARD_ATTEMPTS) | ((unsigned long long)n << 8);
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
            const int ia = particle_rinf_id<PARTICLES_SLAB>(Rinf, nr, A, r);
            int is = r >= Rmed[ia] ? ia : ia - 1; // get_rmed_id with the release build's clamp
            off_substep = off_substep || particle_off_slab<PARTICLES_SLAB>(P, is, 0, nr - 3);
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

    if (PARTICLES_SLAB && off_substep) { // (the last substep's cell)
        *A.status = (unsigned long long)PARTICLE_GUARD_OFF_SLAB | ((unsigned long long)n << 8);
        return;
    }
    // ---- move(): escaped particles leave; rotate(): the frame's turn over the step -----------------------------------
    const double rsq = CART ? q1 * q1 + q2 * q2 : q1 * q1;
    if (rsq > A.escape_max_sq || rsq < A.escape_min_sq)
        A.alive[n] = 0;
    const double frame_angle = particle_frame_angle<PARTICLES_DEV>(P, A, dt);
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
