// The host-only stages of fcpt_selfgravity (no HIP header): what it refuses, the transform plans, the kernel tables of
// compute_FFT_kernel and the per-ring weights.  fcpt_selftest_selfgravity_kernel and fcpt_selftest_fft_radices run them on
// any machine.
#include "fcpt_selfgravity.h"

#include <cmath>

namespace fcpt {

int sg_validate(const fcpt_desc &d, const fcpt_selfgravity_params &p, FftPlan *plan_phi, FftPlan *plan_rad)
{
    if (p.mode != FCPT_SG_BASIC && p.mode != FCPT_SG_SYMMETRIC) {
        set_error("fcpt_selfgravity: unknown mode %d (FCPT_SG_BASIC = 1, FCPT_SG_SYMMETRIC = 2; the Bessel kernel is not built)",
                  p.mode);
        return FCPT_EINVAL;
    }
    if (d.radial_spacing != FCPT_SPACING_LOGARITHMIC) { // selfgravity.cpp:222
        set_error("fcpt_selfgravity: a logarithmic grid is needed to compute self-gravity with the polar method (RadialSpacing)");
        return FCPT_EINVAL;
    }
    if (d.nranks != 1) {
        set_error("fcpt_selfgravity: the context is one of %d slabs; self-gravity runs on one slab only", d.nranks);
        return FCPT_EINVAL;
    }
    if (!(p.aspect_ratio > 0.0)) {
        set_error("fcpt_selfgravity: aspect_ratio must be positive (got %g)", p.aspect_ratio);
        return FCPT_EINVAL;
    }
    FftPlan a, b;
    const long long lengths[2] = {(long long)d.nphi, 2ll * d.nr_global};
    FftPlan *plans[2] = {&a, &b};
    for (int k = 0; k < 2; ++k)
        if (lengths[k] > FFT_MAX_N || !fft_plan((int)lengths[k], plans[k])) {
            set_error("fcpt_selfgravity: transform length %lld (%s) is refused: a length must be at most %d and have no prime "
                      "factor above 5",
                      lengths[k], k == 0 ? "Nphi" : "2 Nrad", FFT_MAX_N);
            return FCPT_EINVAL;
        }
    if (plan_phi)
        *plan_phi = a;
    if (plan_rad)
        *plan_rad = b;
    return FCPT_OK;
}

void sg_kernel_tables(const fcpt_desc &d, const double *Radii, const fcpt_selfgravity_params &p, double *K_radial,
                      double *K_azimuthal)
{
    const int N = d.nr_global, nphi = d.nphi;
    const double aspect_ratio = p.aspect_ratio;
    // update_sg_constants (selfgravity.cpp:171-179)
    double lambda_sq = 0.0, chi_sq = 0.0, epsilon = 0.0;
    if (p.mode == FCPT_SG_SYMMETRIC) {
        lambda_sq = std::pow(0.4571 * aspect_ratio + 0.6737 * std::sqrt(aspect_ratio), 2);
        chi_sq = std::pow((-0.7543 * aspect_ratio + 0.6472) * aspect_ratio, 2);
    } else {
        epsilon = p.thickness_smoothing_sg * aspect_ratio;
    }
    const double dphi = 2.0 * M_PI / (double)nphi;
    for (int i = 0; i < 2 * N; ++i) {
        double u; // :423-430
        if (i < N)
            u = std::log(Radii[i] / Radii[0]);
        else
            u = -std::log(Radii[2 * N - i] / Radii[0]);
        for (int j = 0; j < nphi; ++j) {
            const size_t l = (size_t)i * nphi + j;
            const double theta = dphi * (double)j;
            if (p.mode == FCPT_SG_BASIC) { // :436-443
                const double denominator =
                    std::pow(epsilon * epsilon * std::exp(u) + 2.0 * (std::cosh(u) - std::cos(theta)), -1.5);
                K_radial[l] = 1.0 + epsilon * epsilon - std::cos(theta) * std::exp(-u);
                K_radial[l] *= denominator;
                K_azimuthal[l] = std::sin(theta);
                K_azimuthal[l] *= denominator;
            } else { // :503-511
                const double denominator = std::pow(
                    2 * (std::cosh(u) - std::cos(theta)) + lambda_sq * (std::exp(u) + std::exp(-u) - 2) + chi_sq, -1.5);
                K_radial[l] = 1.0 - std::cos(theta) * std::exp(-u);
                K_radial[l] *= denominator;
                K_azimuthal[l] = std::sin(theta);
                K_azimuthal[l] *= denominator;
            }
        }
    }
}

void sg_ring_weights(const fcpt_desc &d, const double *Radii, const HostGeometry &g, int nr, SgRingWeights &w)
{
    const int N = d.nr_global;
    // selfgravity.cpp:246-247
    const double r_step = std::log(Radii[N] / Radii[0]) / (double)N;
    const double t_step = 2.0 * M_PI / (double)d.nphi;
    w.sqrt_ratio.resize(nr), w.norm_r.resize(nr), w.norm_t.resize(nr);
    for (int i = 0; i < nr; ++i) {
        w.sqrt_ratio[i] = std::sqrt(g.Rmed[i] / g.Rmed[0]);
        // :678-683
        double normaccr = r_step * t_step / ((double)(2 * N) * (double)d.nphi);
        double normacct = normaccr;
        normaccr /= std::sqrt(g.Rmed[i] / g.Rmed[0]);
        normacct /= (g.Rmed[i] / g.Rmed[0] * std::sqrt(g.Rmed[i] / g.Rmed[0]));
        w.norm_r[i] = normaccr, w.norm_t[i] = normacct;
    }
}

} // namespace fcpt

using namespace fcpt;

extern "C" int fcpt_selftest_selfgravity_kernel(const fcpt_desc *d, const double *radii, const fcpt_selfgravity_params *p,
                                                double *k_radial, double *k_azimuthal, int64_t capacity)
{
    if (!p || !k_radial || !k_azimuthal) {
        set_error("null argument");
        return FCPT_EINVAL;
    }
    if (int rc = validate_create(d, radii))
        return rc;
    if (int rc = sg_validate(*d, *p, nullptr, nullptr))
        return rc;
    const int64_t need = 2ll * d->nr_global * d->nphi;
    if (capacity < need) {
        set_error("fcpt_selftest_selfgravity_kernel: each table holds 2 Nrad x Nphi = %lld doubles, capacity is %lld",
                  (long long)need, (long long)capacity);
        return FCPT_EINVAL;
    }
    sg_kernel_tables(*d, radii, *p, k_radial, k_azimuthal);
    return FCPT_OK;
}

extern "C" int fcpt_selftest_fft_radices(int32_t n, int32_t *radices, int32_t capacity, int32_t *count)
{
    if (!count || capacity < 0 || (capacity > 0 && !radices)) {
        set_error("null argument");
        return FCPT_EINVAL;
    }
    FftPlan plan;
    if (!fft_plan(n, &plan)) {
        set_error("transform length %d is refused: a length must be in 1 .. %d and have no prime factor above 5", n, FFT_MAX_N);
        return FCPT_EINVAL;
    }
    *count = plan.nstages;
    if (capacity > 0 && capacity < plan.nstages) {
        set_error("fcpt_selftest_fft_radices: %d stages, capacity is %d", plan.nstages, capacity);
        return FCPT_EINVAL;
    }
    for (int k = 0; k < plan.nstages && k < capacity; ++k)
        radices[k] = plan.radix[k];
    return FCPT_OK;
}
