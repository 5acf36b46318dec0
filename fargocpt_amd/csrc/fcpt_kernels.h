// Launch functions of fcpt_kernels.hip (all asynchronous on the given stream).
#ifndef FCPT_KERNELS_H
#define FCPT_KERNELS_H

#include <vector>
#include <hip/hip_runtime.h>

#include "fcpt_internal.h"
#include "fcpt_schedule.h"
#include "fcpt_plan.h"

namespace fcpt {

// One id per __global__ function family; kKernelNames[id] is the function's name as rocprofv3 prints it (without
// namespace and template arguments), so that fcpt_profile_stop's table can be matched to profiles/*.csv by name.
// KID_CLOCK stands for the single-thread k_clock_* kernels (set_dt, scale_dt, advance, policy, policy_ptr, export_cfl).
enum KernelId {
    KID_POTENTIAL, KID_ADI_CS_H, KID_ISO_CS_H, KID_VISCOSITY, KID_PRESSURE, KID_TEMPERATURE,
    KID_SUBSTEP3, KID_BOUNDARY, KID_DAMPING, KID_TRANSPORT_RADIAL,
    KID_RING_MEAN, KID_THETA1, KID_THETA2, KID_VELOCITIES, KID_CFL_INIT, KID_CFL_CELLS, KID_CLOCK,
    KID_SRC_FUSED, KID_AV_FUSED, KID_VISC_FUSED, KID_SOURCE_MARCH, KID_THETA_MARCH,
    KID_TRANSPORT_FUSED, KID_MASSFLOW, KID_CFL_RINGS, KID_THETA_GATED_BOUNDARY, KID_EXCHANGE_COPY,
    KID_DISK_ON_BODY, KID_VISC_FACTORS, KID_SOURCE_MARCH_ADI, KID_SOURCE_MARCH_ADI_WIDE,
    KID_ACCEL_ON_GAS, KID_SOURCE_MARCH_ADI_ACC, KID_TRANSPORT_RADIAL_MEANS, KID_CFL_RINGS_BC,
    KID_DISK_ON_BODIES, KID_PARTICLES, KID_PARTICLES_EXPLICIT, KID_PARTICLES_EMIGRATE, KID_PARTICLES_EMIGRATE_FINISH,
    KID_PARTICLES_IMMIGRATE, KID_PARTICLES_EMIGRATE_COUNT,
    KID_SG_FFT_ROWS, KID_SG_TRANSPOSE, KID_SG_MULTIPLY, KID_SG_KICK, KID_COUNT
};
static_assert(KID_COUNT <= 64, "fcpt_profile_start selects kernels with a 64-bit mask");
extern const char *const kKernelNames[KID_COUNT];

// HIP-event stopwatch around selected kernel launches (on the launch stream).
struct Profiler {
    unsigned long long mask = 0;
    std::vector<hipEvent_t> events;
    std::vector<int> ids;
    int used = 0;
    int open_id = -1;
    int stride = 1, seen = 0; // every stride-th launch of the selected kernels carries the event pair (option profile_stride)
    void begin(int id, hipStream_t st);
    void end(int id, hipStream_t st);
};
extern thread_local Profiler *g_prof;

void launch_potential(const Dev &P, hipStream_t st);
void launch_accel_on_gas(const Dev &P, hipStream_t st);
void launch_body_force(const Dev &P, hipStream_t st); // the potential, or the accelerations (simulation.cpp:167-175)
void launch_recalculate_viscosity(const Dev &P, hipStream_t st);
void launch_viscosity_field(const Dev &P, hipStream_t st);
void launch_iso_cs_h(const Dev &P, const double *cs_ring, hipStream_t st);
void launch_visc_factors(const Dev &P, hipStream_t st);
void launch_boundary(const Dev &P, hipStream_t st);
void launch_selftest_half_limiter(int type, long long n, const double *a, const double *b, double *out, hipStream_t st);
void launch_exchange_copy(const Dev &P, double *inner, double *outer, int unpack, hipStream_t st);
void launch_damping(const Dev &P, double *q, double *q0, const double *radius, const DampRange &r,
                    int is_density, hipStream_t st);
// Where Transport() left the new state: the marching kernels cannot work in place (neighbouring
// wavefronts still read the old rings), so they write Sigma / e to the A scratch grids and the
// velocities to whichever of vrad|vrad_b, vazi|vazi_b was not the input; the caller swaps the
// context's pointers accordingly.
struct TransportResult {
    int marched;  // > 0: a marching kernel ran (new state complete, clock advanced)
    double *sigma, *energy, *vrad, *vazi;
    int split;    // only a part of the chunks was marched
    int gated_pending; // launch_transport(defer_gated): the gated azimuthal launch of the fallback is still to be queued (launch_gated_theta)
};
// the arguments of that launch, kept by the caller until the final boundary call of the step
struct GatedTheta {
    Dev P, Wm;
};
void launch_gated_theta(const GatedTheta &g, const Dev *boundary_view, hipStream_t st); // boundary_view != null: + the boundary call, one launch
enum { TRANSPORT_ALL = 0, TRANSPORT_EDGES = 1, TRANSPORT_INTERIOR = 2 };
TransportResult launch_transport(const Dev &P, const Dev &W, hipStream_t st, int part = TRANSPORT_ALL, GatedTheta *defer_gated = nullptr);
int device_cus(); // compute units of the current device: the argument n_cu of the chunk planner (fcpt_schedule.h)
void launch_shift_means(const Dev &P, hipStream_t st);
void launch_massflow(const Dev &P, hipStream_t st);
void launch_substep3_cooling_only(const Dev &P, hipStream_t st);
void launch_disk_on_body(const Dev &P, double x, double y, double r_object, double smoothing_fixed, double r_sm, double *out,
                         hipStream_t st);
// the objects of k_disk_on_bodies, by value in the kernel's arguments (entries past n are not read)
struct DiskBodies {
    double x[FCPT_MAX_BODIES], y[FCPT_MAX_BODIES], r_object[FCPT_MAX_BODIES], smoothing_fixed[FCPT_MAX_BODIES], r_sm[FCPT_MAX_BODIES];
};
size_t disk_on_bodies_blocks(const Dev &P); // blocks of the first stage: `part` holds 4 * n * blocks doubles, `out` 4 * n
void launch_disk_on_bodies(const Dev &P, int n, const DiskBodies &B, double *part, double *out, hipStream_t st);
void launch_particles(const Dev &P, const ParticleArgs &A, hipStream_t st, bool slab = false);
void launch_particles_explicit(const Dev &P, const ParticleArgs &A, const ParticleAdaptive &X, bool cartesian, hipStream_t st,
                               bool slab = false);
void launch_particles_emigrate(const ParticleArgs &A, const ParticleAdaptive &X, const ParticleMigrate &M, hipStream_t st);
void launch_particles_immigrate(const ParticleArgs &A, const ParticleAdaptive &X, const ParticleMigrate &M, hipStream_t st);
void launch_particles_timestep_init(const Dev &P, const ParticleArgs &A, const ParticleAdaptive &X, bool cartesian, hipStream_t st);
void launch_particles_normals(int n, const unsigned long long *id, unsigned long long seed, unsigned long long step, double *snv,
                              hipStream_t st);
void launch_particles_counter_offset(unsigned long long *offset, unsigned long long counter, const DevClock *clk, hipStream_t st);
void launch_source_fused(const Dev &P, hipStream_t st);
int launch_source_march(const Dev &P, hipStream_t st, bool fold_bc, bool *bc_folded, bool fold_cfl = false);
void launch_cfl_final(const Dev &P, int apply_policy, hipStream_t st);
void launch_viscous_fused(const Dev &P, hipStream_t st);
void launch_derived(const Dev &P, hipStream_t st);
void launch_pressure(const Dev &P, hipStream_t st);
void launch_temperature(const Dev &P, hipStream_t st);
void launch_cfl(const Dev &P, int apply_policy, hipStream_t st, bool interior_done = false);
bool launch_cfl_interior(const Dev &P, hipStream_t st);
void launch_cfl_bc(const Dev &P, int apply_policy, hipStream_t st);
void launch_clock_set_dt(DevClock *clk, double dt, hipStream_t st);
void launch_clock_scale_dt(DevClock *clk, int mode, double dt, double factor, hipStream_t st);
void launch_clock_export_cfl(DevClock *clk, double *out, hipStream_t st);
void launch_clock_policy_ptr(DevClock *clk, double cfl_max_var, const double *cfl_global, hipStream_t st);
void launch_clock_advance(DevClock *clk, hipStream_t st);
void launch_clock_policy(DevClock *clk, double cfl_max_var, int use_device_cfl, double cfl_global,
                         hipStream_t st);

} // namespace fcpt
#endif
