// fargocpt_hip -- the bodies of the setup: the star at the origin and the planets, either on their initial circular
// orbits seen in the frame rotating with OmegaFrame, or (--bodies free) as a system of their own (fcpt_nbody_*) that
// moves under its own gravity and, with DiskFeedback, under the disk's.
#include "driver.h"

#include <algorithm>
#include <cmath>

void BodySystem::init(const Config &c)
{
    const fcpt_desc &d = dr->desc;
    // (HydroFrameCenter: all with a single body is the same centre)
    const std::string frame_center = lower(c.str("HydroFrameCenter", "primary"));
    indirect = frame_center == "primary" || (frame_center == "all" && c.nbody.size() == 1);
    torque_acc.assign(bodies.size(), 0.0);
    indirect_acc.assign(bodies.size(), 0.0);
    if (free) {
        CHECK(fcpt_nbody_create(d.G, &nb));
        for (const Body &b : bodies)
            CHECK(fcpt_nbody_add(nb, b.m, b.a, b.ecc, b.pericenter, b.true_anomaly));
        CHECK(fcpt_nbody_shift_to_centre(nb, 1)); // HydroFrameCenter: primary
    }
    no_star_smoothing = c.flag("CompatibilityNoStarSmoothing", false);
    smoothing_planetloc = c.flag("CompatibilitySmoothingPlanetLoc", false);
}

double BodySystem::omega_kepler(const Body &b) const
{
    const fcpt_desc &d = dr->desc;
    return b.a > 0 ? std::sqrt(d.G * (d.hydro_center_mass + b.m) / (b.a * b.a * b.a)) : 0.0;
}
// get_rampup_mass (planet.cpp:166-179): m, or the body's mass ramped up over its first "ramp-up time" orbits
double BodySystem::rampup_mass(const Body &b, double t, double m) const
{
    const double om = omega_kepler(b);
    if (b.rampup > 0 && om > 0) {
        const double period = 2 * M_PI / om;
        if (t < b.rampup * period) {
            const double cs = std::cos(t * M_PI_2 / (b.rampup * period));
            return b.m * (1.0 - cs * cs);
        }
    }
    return m;
}
// dimensionless Roche radius ~ (q/3)^(1/3) (Theo.cpp:251-277 converges to it for small q)
double BodySystem::roche_smoothing(const Body &b) const
{
    return b.a * std::cbrt(b.m / (3.0 * dr->desc.hydro_center_mass)) * b.rsm_factor;
}

// Bodies at time t for the potential of a step of length dt (CalculateNbodyPotential, Pframeforce.cpp:21-94):
// positions on the circular orbits, masses ramped up, and the indirect term of the star-centred frame without the
// disk (refframe::IndirectTermPlanets): minus the acceleration of the star, which the reference takes as the velocity
// change of the hydro centre over the step divided by dt (ComputeIndirectTermNbody, frame_of_reference.cpp:138-160)
// -- for circular orbits the time average of G m r_p / a^3 over [t, t + dt], in closed form.
void BodySystem::set_circular(double t, double dt)
{
    const fcpt_desc &d = dr->desc;
    double x[FCPT_MAX_BODIES], y[FCPT_MAX_BODIES], m[FCPT_MAX_BODIES], rsm[FCPT_MAX_BODIES];
    const int n = (int)std::min<size_t>(bodies.size(), FCPT_MAX_BODIES);
    itx = ity = 0.0;
    for (int k = 0; k < n; ++k) {
        const Body &b = bodies[k];
        const double om = omega_kepler(b);
        const double ang = b.phase + (om - d.omega_frame) * t;
        x[k] = b.a * std::cos(ang);
        y[k] = b.a * std::sin(ang);
        m[k] = rampup_mass(b, t, b.m);
        rsm[k] = roche_smoothing(b);
        if (indirect && k > 0 && b.a > 0 && dt > 0) {
            const double g = d.G * b.m / (b.a * b.a), w = om * dt;
            itx -= g * (std::sin(ang + w) - std::sin(ang)) / w;
            ity -= g * (std::cos(ang) - std::cos(ang + w)) / w;
        }
    }
    CHECK(fcpt_set_bodies(dr->ctx, n, x, y, m, rsm, itx, ity));
}

// arguments of the disk's force on every body at the current positions (compute_smoothing, Force.cpp:145-159)
void BodySystem::queue_disk_force()
{
    const fcpt_desc &d = dr->desc;
    double state[FCPT_MAX_BODIES * FCPT_NBODY_STATE];
    double x[FCPT_MAX_BODIES], y[FCPT_MAX_BODIES], r[FCPT_MAX_BODIES], sm[FCPT_MAX_BODIES], rsm[FCPT_MAX_BODIES];
    CHECK(fcpt_nbody_get_state(nb, state));
    for (int k = 0; k < count(); ++k) {
        const double *q = state + FCPT_NBODY_STATE * k;
        x[k] = q[0];
        y[k] = q[1];
        r[k] = std::sqrt(q[0] * q[0] + q[1] * q[1]);
        sm[k] = -1.0; // ThicknessSmoothing x H of each cell
        if (no_star_smoothing && k == 0)
            sm[k] = 0.0;
        else if (smoothing_planetloc)
            sm[k] = d.thickness_smoothing * d.aspect_ratio * std::pow(r[k], 1.0 + d.flaring_index);
        rsm[k] = roche_smoothing(bodies[k]);
    }
    CHECK(fcpt_disk_on_bodies_begin(dr->ctx, count(), x, y, r, sm, rsm));
}

// inner + outer sums of all slabs: the disk's specific force on body k in (ax[k], ay[k])
void BodySystem::collect_disk_force(double *ax, double *ay)
{
    double f[4 * FCPT_MAX_BODIES];
    CHECK(fcpt_disk_on_bodies_end(dr->ctx, f));
    if (dr->slab.multi())
        CHECK(fcpt_allreduce_sum(dr->ctx, 4 * count(), f));
    for (int k = 0; k < count(); ++k) {
        ax[k] = f[4 * k] + f[4 * k + 2];
        ay[k] = f[4 * k + 1] + f[4 * k + 3];
    }
}

// step_Euler up to the potential (simulation.cpp:155-175) for a step of length dt from the force (ax, ay) on the state
// at its start: disk kick, both indirect terms, bodies to the context, indirect term on the bodies.  dt = 0: only the
// bodies go to the context.
void BodySystem::set_free(double t, double dt, const double *ax, const double *ay)
{
    const int n = count();
    double state[FCPT_MAX_BODIES * FCPT_NBODY_STATE];
    itx = ity = 0.0;
    if (dt > 0.0 && disk_feedback) {
        CHECK(fcpt_nbody_get_state(nb, state));
        for (int k = 0; k < n; ++k) {
            const double *q = state + FCPT_NBODY_STATE * k;
            torque_acc[k] += q[4] * (q[0] * ay[k] - q[1] * ax[k]) * dt;
            indirect_acc[k] += q[4] * (q[1] * ax[0] - q[0] * ay[0]) * dt;
        }
        CHECK(fcpt_nbody_kick(nb, ax, ay, dt)); // UpdatePlanetVelocitiesWithDiskForce
        itx -= ax[0];                            // ComputeIndirectTermDisk: one centre body
        ity -= ay[0];
    }
    if (dt > 0.0 && n > 1) { // ComputeIndirectTermNbody, IndirectTermMode 0
        double dv[2];
        CHECK(fcpt_nbody_centre_delta_v(nb, 1, dt, dv));
        itx -= dv[0] / dt;
        ity -= dv[1] / dt;
    }
    double x[FCPT_MAX_BODIES], y[FCPT_MAX_BODIES], m[FCPT_MAX_BODIES], rsm[FCPT_MAX_BODIES];
    CHECK(fcpt_nbody_get_state(nb, state));
    for (int k = 0; k < n; ++k) {
        const double *q = state + FCPT_NBODY_STATE * k;
        x[k] = q[0];
        y[k] = q[1];
        m[k] = rampup_mass(bodies[k], t, q[4]);
        rsm[k] = roche_smoothing(bodies[k]);
    }
    CHECK(fcpt_set_bodies(dr->ctx, n, x, y, m, rsm, itx, ity));
    if (dt > 0.0) { // apply_indirect_term_on_Nbody
        double kx[FCPT_MAX_BODIES], ky[FCPT_MAX_BODIES];
        for (int k = 0; k < n; ++k) {
            kx[k] = itx;
            ky[k] = ity;
        }
        CHECK(fcpt_nbody_kick(nb, kx, ky, dt));
    }
}

// the rest of the step for the bodies (simulation.cpp:222-224) and the frame's rotation
void BodySystem::advance(double dt)
{
    CHECK(fcpt_nbody_advance(nb, dt));
    CHECK(fcpt_nbody_shift_to_centre(nb, 1));
    if (dr->desc.omega_frame != 0.0)
        CHECK(fcpt_nbody_rotate(nb, -dr->desc.omega_frame * dt));
}

// correct_velocity_for_disk_accel (main.cpp:123-126, planetary_system.cpp:895-939)
void BodySystem::correct_velocity_for_disk()
{
    const int n = count();
    double ax[FCPT_MAX_BODIES], ay[FCPT_MAX_BODIES], state[FCPT_MAX_BODIES * FCPT_NBODY_STATE];
    queue_disk_force();
    collect_disk_force(ax, ay);
    CHECK(fcpt_nbody_get_state(nb, state));
    for (int k = 0; k < n; ++k) {
        double *q = state + FCPT_NBODY_STATE * k;
        const double v2 = q[2] * q[2] + q[3] * q[3], ar = ax[k] * q[0] + ay[k] * q[1]; // v_new^2 / r = v_old^2 / r - a_r
        if (v2 == 0.0 || ar > v2)
            continue;
        const double scale = std::sqrt(v2 - ar) / std::sqrt(v2);
        q[2] *= scale;
        q[3] *= scale;
    }
    CHECK(fcpt_nbody_set_state(nb, n, state));
}

// monitor/nbody<k>.dat (t_planet::write, nbody/planet.cpp:283-374): the reference's columns; those this driver has no
// source for (circumplanetary mass, anomalies, accretion) are written as 0.  The accumulators start again.
void BodySystem::write_rows(unsigned nsnap, unsigned nmon, double t, bool create)
{
    if (!dr->slab.master())
        return;
    const fcpt_desc &d = dr->desc;
    double state[FCPT_MAX_BODIES * FCPT_NBODY_STATE];
    CHECK(fcpt_nbody_get_state(nb, state));
    for (int k = 0; k < count(); ++k) {
        FILE *f = open_or_die(dr->outdir + "monitor/nbody" + std::to_string(k) + ".dat", create ? "w" : "a");
        if (create) {
            const char *cols[] = {"snapshot number | 1", "monitor number | 1", "x | length", "y | length", "vx | velocity",
                                  "vy | velocity", "mass | mass", "time | time", "omega frame | frequency",
                                  "mdcp | mass", "eccentricity | 1", "angular momentum | angular momentum",
                                  "semi-major axis | length", "omega kepler | frequency", "mean anomaly | 1",
                                  "eccentric anomaly | 1", "true anomaly | 1", "pericenter angle | 1", "torque | torque",
                                  "accreted torque | torque", "indirect torque | torque", "accretion rate | mass accretion rate"};
            fprintf(f, "#FargoCPT planet file for planet: %d\n#version: 2\n", k);
            for (int c = 0; c < 22; ++c)
                fprintf(f, "#variable: %d | %s\n", c, cols[c]);
        }
        const double *q = state + FCPT_NBODY_STATE * k, *q0 = state;
        double ecc = 0.0, sma = 0.0, omk = 0.0;
        const double rx = q[0] - q0[0], ry = q[1] - q0[1], vx = q[2] - q0[2], vy = q[3] - q0[3];
        const double h = rx * vy - ry * vx, mu = d.G * (q0[4] + q[4]), r = std::sqrt(rx * rx + ry * ry);
        if (k > 0 && r > 0.0 && mu > 0.0) {
            sma = 1.0 / (2.0 / r - (vx * vx + vy * vy) / mu);
            const double e2 = 1.0 - h * h / (mu * sma);
            ecc = e2 > 0.0 ? std::sqrt(e2) : 0.0;
            omk = sma > 0.0 ? std::sqrt(mu / (sma * sma * sma)) : 0.0;
        }
        fprintf(f, "%u\t%u\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g"
                   "\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\t%#.18g\n",
                nsnap, nmon, q[0], q[1], q[2], q[3], q[4], t, d.omega_frame, 0.0, ecc, q[4] * (q[0] * q[3] - q[1] * q[2]), sma,
                omk, 0.0, 0.0, 0.0, 0.0, torque_acc[k] / d.monitor_timestep, 0.0, indirect_acc[k] / d.monitor_timestep, 0.0);
        fclose(f);
    }
    std::fill(torque_acc.begin(), torque_acc.end(), 0.0);
    std::fill(indirect_acc.begin(), indirect_acc.end(), 0.0);
}

// nbody.bin: uint32 version (1), uint32 n, n x FCPT_NBODY_STATE doubles (fcpt_nbody_get_state)
void BodySystem::save(const std::string &dir) const
{
    const size_t n = (size_t)count() * FCPT_NBODY_STATE;
    const uint32_t head[2] = {1u, (uint32_t)count()};
    double state[FCPT_MAX_BODIES * FCPT_NBODY_STATE];
    CHECK(fcpt_nbody_get_state(nb, state));
    FILE *f = open_or_die(dir + "nbody.bin", "wb");
    if (fwrite(head, sizeof(head), 1, f) != 1 || fwrite(state, sizeof(double), n, f) != n)
        die_cannot("write", dir + "nbody.bin");
    fclose(f);
}
void BodySystem::load(const std::string &dir)
{
    const size_t n = (size_t)count() * FCPT_NBODY_STATE;
    uint32_t head[2] = {0, 0};
    double state[FCPT_MAX_BODIES * FCPT_NBODY_STATE];
    FILE *f = fopen((dir + "nbody.bin").c_str(), "rb");
    if (!f || fread(head, sizeof(head), 1, f) != 1 || head[0] != 1u || head[1] != (uint32_t)count() ||
        fread(state, sizeof(double), n, f) != n) {
        fprintf(stderr, "fargocpt_hip: cannot read the state of %d bodies from %snbody.bin (written by --bodies free)\n",
                count(), dir.c_str());
        exit(1);
    }
    fclose(f);
    CHECK(fcpt_nbody_set_state(nb, count(), state));
}
