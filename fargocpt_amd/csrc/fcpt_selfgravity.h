// Self-gravity of the gas (selfgravity.cpp): what the host unit fcpt_selfgravity_tables.cpp builds for the device unit
// fcpt_selfgravity.hip, and the device-side state of a context that has it switched on.
#ifndef FCPT_SELFGRAVITY_H
#define FCPT_SELFGRAVITY_H

#include "fcpt_internal.h"
#include "kernels/fft.h"

namespace fcpt {

// what fcpt_selfgravity refuses, before it looks at the device; fills the two plans (lengths nphi and 2 nr_global)
int sg_validate(const fcpt_desc &d, const fcpt_selfgravity_params &p, FftPlan *plan_phi, FftPlan *plan_rad);

// K_radial and K_azimuthal of compute_FFT_kernel (selfgravity.cpp:418-518), 2 nr_global x nphi each, row-major, with
// update_sg_constants' epsilon, lambda_sq and chi_sq (:171-179): libm, the reference's expressions in its order
void sg_kernel_tables(const fcpt_desc &d, const double *radii, const fcpt_selfgravity_params &p, double *k_radial,
                      double *k_azimuthal);

// per ring (one slab: the local rings are the global ones): the weights of compute_FFT_density (:356-358) and the
// normalisation of compute_acceleration (:673-689)
struct SgRingWeights {
    std::vector<double> sqrt_ratio; // sqrt(Rmed[i] / Rmed[0])
    std::vector<double> norm_r, norm_t;
};
void sg_ring_weights(const fcpt_desc &d, const double *radii, const HostGeometry &g, int nr, SgRingWeights &w);

// the device side of one context: null / zero while self-gravity is off
struct SgDev {
    int nr, nphi; // the hydro grid; the transforms have lengths nphi and 2 nr
    FftPlan plan_phi, plan_rad;
    double *A;    // nr x nphi complex: phi-spectrum of the packed density, later the radial inverse's lower half
    double *B;    // nphi x nr complex: A transposed
    double *C;    // nphi x 2 nr complex: the spectrum of S_r + i S_t, multiplied in place
    double *KC;   // nphi x 2 nr complex: the spectrum of K_radial + i K_azimuthal
    const double *sqrt_ratio, *norm_r, *norm_t; // nr each
    double rmed0;
    double minus_G;
};

} // namespace fcpt
#endif
