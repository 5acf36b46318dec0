// fcpt_nbody_*: the point masses of the planetary system as a host-side state of their own (needs no GPU).
// What the reference keeps in t_planetary_system (src/nbody/planetary_system.cpp) and advances with its bundled
// REBOUND: here positions, velocities and masses of <= FCPT_MAX_BODIES bodies in the plane and an integrator written
// from the literature -- Gragg's modified midpoint rule extrapolated to zero step length (Bulirsch & Stoer 1966;
// Hairer, Norsett & Wanner, Solving ODEs I, section II.9): sub-step counts 2, 4, ..., 16, eight columns of the
// Aitken-Neville tableau in h^2, i.e. order 16.  Everything is fixed-order arithmetic on the host: the same state and
// the same dt give the same bits, which is what lets every slab integrate its own copy of the bodies.
#include "fcpt_internal.h"

#include <cmath>
#include <cstring>
#include <new>

struct fcpt_nbody {
    double G;
    int n;
    double x[FCPT_MAX_BODIES], y[FCPT_MAX_BODIES], vx[FCPT_MAX_BODIES], vy[FCPT_MAX_BODIES], m[FCPT_MAX_BODIES];
    // what the additions of advance() have rounded away from x, y, vx, vy so far (compensated summation: a step's
    // rounding error then scales with the step's change, not with the state, and many short steps cost no accuracy)
    double carry[4][FCPT_MAX_BODIES];
};

namespace fcpt {
namespace {

constexpr int NB = FCPT_MAX_BODIES;
constexpr int NV = 4 * NB; // x, y, vx, vy of every body
constexpr int BS_COLUMNS = 8;

struct Vec {
    double q[NV];
};

// d/dt (x, y, vx, vy) under mutual Newtonian gravity; every pair is evaluated once and applied to both partners
void derivative(const fcpt_nbody &s, const Vec &z, Vec &f)
{
    const int n = s.n;
    for (int i = 0; i < n; ++i) {
        f.q[i] = z.q[2 * NB + i];
        f.q[NB + i] = z.q[3 * NB + i];
        f.q[2 * NB + i] = 0.0;
        f.q[3 * NB + i] = 0.0;
    }
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double dx = z.q[j] - z.q[i], dy = z.q[NB + j] - z.q[NB + i];
            const double r2 = dx * dx + dy * dy;
            const double w = s.G / (r2 * std::sqrt(r2));
            f.q[2 * NB + i] += s.m[j] * w * dx;
            f.q[3 * NB + i] += s.m[j] * w * dy;
            f.q[2 * NB + j] -= s.m[i] * w * dx;
            f.q[3 * NB + j] -= s.m[i] * w * dy;
        }
}

// Gragg: z1 = z0 + h f(z0), z_{k+1} = z_{k-1} + 2h f(z_k), result (z_n + z_{n-1} + h f(z_n)) / 2 -- carried as the
// increments z - y0, so that the tableau's rounding errors scale with the step's change and not with the state
void modified_midpoint(const fcpt_nbody &s, const Vec &y0, const Vec &f0, double H, int nsub, Vec &out)
{
    const int n = s.n;
    const double h = H / nsub;
    Vec a, b, z, f;
    std::memset(&a, 0, sizeof(a));
    z = y0;
    for (int c = 0; c < 4; ++c)
        for (int i = 0; i < n; ++i) {
            b.q[c * NB + i] = h * f0.q[c * NB + i];
            z.q[c * NB + i] = y0.q[c * NB + i] + b.q[c * NB + i];
        }
    for (int k = 1; k < nsub; ++k) {
        derivative(s, z, f);
        for (int c = 0; c < 4; ++c)
            for (int i = 0; i < n; ++i) {
                const int e = c * NB + i;
                const double next = a.q[e] + 2.0 * h * f.q[e];
                a.q[e] = b.q[e];
                b.q[e] = next;
                z.q[e] = y0.q[e] + next;
            }
    }
    derivative(s, z, f);
    for (int c = 0; c < 4; ++c)
        for (int i = 0; i < n; ++i)
            out.q[c * NB + i] = 0.5 * (a.q[c * NB + i] + b.q[c * NB + i] + h * f.q[c * NB + i]);
}

// One extrapolated step of length H (the tableau holds increments; so does `out`).  Returns the size of the
// last correction relative to the state's scale: the caller halves H when it is not at rounding level.
double extrapolated_step(const fcpt_nbody &s, const Vec &y0, double H, Vec &out)
{
    const int n = s.n;
    Vec f0, T[BS_COLUMNS];
    derivative(s, y0, f0);
    double err = 0.0;
    for (int k = 0; k < BS_COLUMNS; ++k) {
        Vec row;
        modified_midpoint(s, y0, f0, H, 2 * (k + 1), row);
        // Aitken-Neville in h^2: T[j] holds the entry of column j of the previous row until it is overwritten
        Vec prev = row;
        for (int j = 1; j <= k; ++j) {
            const double ratio = (double)(k + 1) / (double)(k + 1 - j);
            const double den = ratio * ratio - 1.0;
            Vec next;
            for (int c = 0; c < 4; ++c)
                for (int i = 0; i < n; ++i) {
                    const int e = c * NB + i;
                    next.q[e] = prev.q[e] + (prev.q[e] - T[j - 1].q[e]) / den;
                }
            T[j - 1] = prev;
            prev = next;
        }
        if (k == BS_COLUMNS - 1) {
            double scale_x = 0.0, scale_v = 0.0, dx = 0.0, dv = 0.0;
            for (int c = 0; c < 4; ++c)
                for (int i = 0; i < n; ++i) {
                    const int e = c * NB + i;
                    const double diff = std::fabs(prev.q[e] - T[k - 1].q[e]), mag = std::fabs(y0.q[e]);
                    if (c < 2) {
                        dx = diff > dx ? diff : dx;
                        scale_x = mag > scale_x ? mag : scale_x;
                    } else {
                        dv = diff > dv ? diff : dv;
                        scale_v = mag > scale_v ? mag : scale_v;
                    }
                }
            err = 0.0;
            if (scale_x > 0.0)
                err = dx / scale_x;
            if (scale_v > 0.0 && dv / scale_v > err)
                err = dv / scale_v;
        }
        T[k] = prev;
    }
    out = T[BS_COLUMNS - 1];
    return err;
}

// the internal sub-step bound: a tenth of the shortest two-body time sqrt(r^3 / (G (m_i + m_j))) of the state
double substep_bound(const fcpt_nbody &s, const Vec &z)
{
    double tmin = HUGE_VAL;
    for (int i = 0; i < s.n; ++i)
        for (int j = i + 1; j < s.n; ++j) {
            const double mu = s.G * (s.m[i] + s.m[j]);
            if (!(mu > 0.0))
                continue;
            const double dx = z.q[j] - z.q[i], dy = z.q[NB + j] - z.q[NB + i];
            const double r2 = dx * dx + dy * dy;
            const double t = std::sqrt(r2 * std::sqrt(r2) / mu);
            tmin = t < tmin ? t : tmin;
        }
    return 0.1 * tmin;
}

void load(const fcpt_nbody &s, Vec &z, Vec &carry)
{
    std::memset(&z, 0, sizeof(z));
    std::memset(&carry, 0, sizeof(carry));
    for (int i = 0; i < s.n; ++i) {
        for (int c = 0; c < 4; ++c)
            carry.q[c * NB + i] = s.carry[c][i];
        z.q[i] = s.x[i];
        z.q[NB + i] = s.y[i];
        z.q[2 * NB + i] = s.vx[i];
        z.q[3 * NB + i] = s.vy[i];
    }
}
void store(fcpt_nbody &s, const Vec &z, const Vec &carry)
{
    for (int i = 0; i < s.n; ++i) {
        for (int c = 0; c < 4; ++c)
            s.carry[c][i] = carry.q[c * NB + i];
        s.x[i] = z.q[i];
        s.y[i] = z.q[NB + i];
        s.vx[i] = z.q[2 * NB + i];
        s.vy[i] = z.q[3 * NB + i];
    }
}

// advances z over dt: sub-steps no longer than the bound, each halved (at most 12 times) while the last column of the
// tableau still moves the result by more than 16 ulp of the state
void advance_vec(const fcpt_nbody &s, Vec &z, Vec &carry, double dt)
{
    if (dt == 0.0 || s.n == 0)
        return;
    const double tol = 16.0 * 2.220446049250313e-16;
    double done = 0.0;
    const double sign = dt < 0.0 ? -1.0 : 1.0, total = std::fabs(dt);
    while (done < total) {
        double h = total - done;
        const double bound = substep_bound(s, z);
        if (h > bound) { // equal parts of what is left, not a short remainder at the end
            const double parts = std::ceil(h / bound);
            h = h / parts;
        }
        Vec out;
        for (int halvings = 0;; ++halvings) {
            const double err = extrapolated_step(s, z, sign * h, out);
            if (err <= tol || halvings >= 12)
                break;
            h *= 0.5;
        }
        for (int c = 0; c < 4; ++c)
            for (int i = 0; i < s.n; ++i) { // Kahan: z += increment, the part that does not fit is carried on
                const int e = c * NB + i;
                const double add = out.q[e] + carry.q[e];
                const double sum = z.q[e] + add;
                carry.q[e] = add - (sum - z.q[e]);
                z.q[e] = sum;
            }
        done = (total - done) - h <= 1e-14 * total ? total : done + h;
    }
}

void centre_of(const fcpt_nbody &s, const Vec &z, int nc, double out[4])
{
    double msum = 0.0;
    out[0] = out[1] = out[2] = out[3] = 0.0;
    for (int i = 0; i < nc; ++i) {
        msum += s.m[i];
        for (int c = 0; c < 4; ++c)
            out[c] += s.m[i] * z.q[c * NB + i];
    }
    if (msum > 0.0) {
        for (int c = 0; c < 4; ++c)
            out[c] /= msum;
    } else if (nc > 0) { // massless centre bodies: the first one
        for (int c = 0; c < 4; ++c)
            out[c] = z.q[c * NB];
    }
}

} // namespace
} // namespace fcpt

using namespace fcpt;

extern "C" {

int fcpt_nbody_create(double G, fcpt_nbody **out)
{
    if (!out || !(G > 0.0)) {
        set_error("fcpt_nbody_create: null argument or G <= 0");
        return FCPT_EINVAL;
    }
    fcpt_nbody *s = new (std::nothrow) fcpt_nbody();
    if (!s)
        return FCPT_ENOMEM;
    std::memset(s, 0, sizeof(*s));
    s->G = G;
    *out = s;
    return FCPT_OK;
}

int fcpt_nbody_destroy(fcpt_nbody *s)
{
    delete s;
    return FCPT_OK;
}

int fcpt_nbody_count(const fcpt_nbody *s, int32_t *n)
{
    if (!s || !n)
        return FCPT_EINVAL;
    *n = s->n;
    return FCPT_OK;
}

// t_planetary_system::init_planet's placement (planetary_system.cpp:483-575)
int fcpt_nbody_add(fcpt_nbody *s, double mass, double semi_major_axis, double eccentricity, double argument_of_pericenter,
                   double true_anomaly)
{
    if (!s || s->n >= FCPT_MAX_BODIES || !(mass >= 0.0) || !(semi_major_axis >= 0.0) || !(eccentricity >= 0.0) ||
        !(eccentricity < 1.0)) {
        set_error("fcpt_nbody_add: more than %d bodies, or mass < 0, semi-major axis < 0, eccentricity outside [0, 1)",
                  FCPT_MAX_BODIES);
        return FCPT_EINVAL;
    }
    const int k = s->n;
    s->m[k] = mass;
    if (k == 0) { // the first body rests at the origin
        s->x[0] = s->y[0] = s->vx[0] = s->vy[0] = 0.0;
        s->n = 1;
        return FCPT_OK;
    }
    // Jacobi elements: the orbit is about the centre of mass of the bodies already there, with their total mass
    double inner_mass = 0.0, cx = 0.0, cy = 0.0;
    for (int i = 0; i < k; ++i) {
        inner_mass += s->m[i];
        cx += s->m[i] * s->x[i];
        cy += s->m[i] * s->y[i];
    }
    if (inner_mass > 0.0) {
        cx /= inner_mass;
        cy /= inner_mass;
    }
    double omega = argument_of_pericenter;
    if (k == 1 && mass > s->m[0])
        omega += M_PI; // the heavier partner of the first pair starts nearest the origin
    const double p = semi_major_axis * (1.0 - eccentricity * eccentricity);
    const double r = p / (1.0 + eccentricity * std::cos(true_anomaly));
    const double v = semi_major_axis > 0.0 ? std::sqrt(s->G * (inner_mass + mass) / p) : 0.0;
    double px = cx + r * std::cos(omega + true_anomaly);
    double py = cy + r * std::sin(omega + true_anomaly);
    double pvx = v * (-std::cos(omega) * std::sin(true_anomaly) - std::sin(omega) * (eccentricity + std::cos(true_anomaly)));
    double pvy = v * (-std::sin(omega) * std::sin(true_anomaly) + std::cos(omega) * (eccentricity + std::cos(true_anomaly)));
    if (k == 1) {
        // elements of a single body mean nothing: the first two are placed together, about their barycentre
        const double mt = s->m[0] + mass;
        const double w0 = mt > 0.0 ? mass / mt : 0.0, w1 = mt > 0.0 ? s->m[0] / mt : 1.0;
        s->x[0] = -w0 * px;
        s->y[0] = -w0 * py;
        s->vx[0] = -w0 * pvx;
        s->vy[0] = -w0 * pvy;
        px *= w1;
        py *= w1;
        pvx *= w1;
        pvy *= w1;
    }
    s->x[k] = px;
    s->y[k] = py;
    s->vx[k] = pvx;
    s->vy[k] = pvy;
    s->n = k + 1;
    return FCPT_OK;
}

int fcpt_nbody_kick(fcpt_nbody *s, const double *ax, const double *ay, double dt)
{
    if (!s || !ax || !ay)
        return FCPT_EINVAL;
    for (int i = 0; i < s->n; ++i) {
        s->vx[i] += ax[i] * dt;
        s->vy[i] += ay[i] * dt;
    }
    return FCPT_OK;
}

int fcpt_nbody_advance(fcpt_nbody *s, double dt)
{
    if (!s || !std::isfinite(dt)) {
        set_error("fcpt_nbody_advance: null argument or dt not finite");
        return FCPT_EINVAL;
    }
    Vec z, carry;
    load(*s, z, carry);
    advance_vec(*s, z, carry, dt);
    store(*s, z, carry);
    return FCPT_OK;
}

// ComputeIndirectTermNbody (frame_of_reference.cpp:135-165) divides this by dt
int fcpt_nbody_centre_delta_v(const fcpt_nbody *s, int32_t n_centre, double dt, double out[2])
{
    if (!s || !out || n_centre < 1 || n_centre > s->n || !std::isfinite(dt)) {
        set_error("fcpt_nbody_centre_delta_v: bad argument (n_centre %d of %d bodies)", (int)n_centre, s ? s->n : 0);
        return FCPT_EINVAL;
    }
    Vec z, carry;
    double before[4], after[4];
    load(*s, z, carry);
    centre_of(*s, z, n_centre, before);
    advance_vec(*s, z, carry, dt);
    centre_of(*s, z, n_centre, after);
    out[0] = after[2] - before[2];
    out[1] = after[3] - before[3];
    return FCPT_OK;
}

int fcpt_nbody_shift_to_centre(fcpt_nbody *s, int32_t n_centre)
{
    if (!s || n_centre < 1 || n_centre > s->n) {
        set_error("fcpt_nbody_shift_to_centre: bad argument (n_centre %d of %d bodies)", (int)n_centre, s ? s->n : 0);
        return FCPT_EINVAL;
    }
    Vec z, carry;
    double c[4];
    load(*s, z, carry);
    centre_of(*s, z, n_centre, c);
    for (int i = 0; i < s->n; ++i) {
        s->x[i] -= c[0];
        s->y[i] -= c[1];
        s->vx[i] -= c[2];
        s->vy[i] -= c[3];
    }
    return FCPT_OK;
}

int fcpt_nbody_rotate(fcpt_nbody *s, double angle)
{
    if (!s)
        return FCPT_EINVAL;
    const double cs = std::cos(angle), sn = std::sin(angle);
    for (int i = 0; i < s->n; ++i) {
        const double x = s->x[i], y = s->y[i], vx = s->vx[i], vy = s->vy[i];
        s->x[i] = x * cs - y * sn;
        s->y[i] = x * sn + y * cs;
        s->vx[i] = vx * cs - vy * sn;
        s->vy[i] = vx * sn + vy * cs;
        for (int c = 0; c < 4; c += 2) { // the carried parts are vectors too
            const double u = s->carry[c][i], w = s->carry[c + 1][i];
            s->carry[c][i] = u * cs - w * sn;
            s->carry[c + 1][i] = u * sn + w * cs;
        }
    }
    return FCPT_OK;
}

int fcpt_nbody_get_state(const fcpt_nbody *s, double *state)
{
    if (!s || !state)
        return FCPT_EINVAL;
    for (int i = 0; i < s->n; ++i) {
        double *q = state + FCPT_NBODY_STATE * i;
        q[0] = s->x[i];
        q[1] = s->y[i];
        q[2] = s->vx[i];
        q[3] = s->vy[i];
        q[4] = s->m[i];
        for (int c = 0; c < 4; ++c)
            q[5 + c] = s->carry[c][i];
    }
    return FCPT_OK;
}

int fcpt_nbody_set_state(fcpt_nbody *s, int32_t n, const double *state)
{
    if (!s || n < 0 || n > FCPT_MAX_BODIES || (n > 0 && !state)) {
        set_error("fcpt_nbody_set_state: n = %d outside 0 .. %d", (int)n, FCPT_MAX_BODIES);
        return FCPT_EINVAL;
    }
    s->n = n;
    for (int i = 0; i < n; ++i) {
        const double *q = state + FCPT_NBODY_STATE * i;
        s->x[i] = q[0];
        s->y[i] = q[1];
        s->vx[i] = q[2];
        s->vy[i] = q[3];
        s->m[i] = q[4];
        for (int c = 0; c < 4; ++c)
            s->carry[c][i] = q[5 + c];
    }
    return FCPT_OK;
}

} // extern "C"
