// Shared by the translation units of the device side of the C ABI: the context structure and the helpers that more
// than one of them uses.  fcpt_context.hip: creation (the device stages: uploads, grids, clock -- what it uploads is
// built by the host unit fcpt_tables.cpp, declared in fcpt_internal.h), options, transfers, initial physics, profiling;
// fcpt_step.hip: CFL, the step, the final boundary call, the run loop (+ hipGraph replay) -- it enqueues what the host
// unit fcpt_plan.cpp decides (fcpt_plan.h) from the Dev view and the LaunchState below;
// fcpt_exchange.hip: ghost exchange and the RCCL entry points; fcpt_particles.hip: dust particles.
#ifndef FCPT_CTX_H
#define FCPT_CTX_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "fcpt_comm.h"
#include "fcpt_kernels.h"
#include "fcpt_selfgravity.h"

using namespace fcpt; // private header of four translation units of namespace-fcpt code around one C struct

#define HIPCHK(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) {                                                             \
            set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return FCPT_EHIP;                                                               \
        }                                                                                   \
    } while (0)

// The particle launch fcpt_run_steps queues in every iteration (fcpt_particles_follow_run_steps), without its per-step
// scalars, which the kernel takes from the device clock: filled by particles_loop_launch(), launched by
// enqueue_particles_loop(), and kept beside a captured graph to tell whether the graph still holds that launch.
// (fcpt_particles_step fills one the same way, with its scalars in A and A.step_offset null, and launches it at once.)
struct ParticleLaunch {
    int on; // follow is switched on and there are particles; 0: everything below is zero
    int explicit_adaptive, cartesian, adapt_set;
    ParticleArgs A;
    ParticleAdaptive X;
};

// The host-side state that decides launches and outlives a call of the ABI, beside the Dev view: what is current on the
// device, what is still owed to it.  One plain struct, zero-filled at fcpt_create the way Dev is: the hipGraph replay
// compares it as a whole and the rollback of a failed capture assigns it as a whole.  What one function of an
// iteration tells the next (StepPlan, KickResult, PendingGated) is passed by value and never stored here.
struct LaunchState {
    bool potential_valid; // the potential grid holds the potential of the current bodies (and scale height)
    bool pressure_valid;  // the pressure grid (ideal EOS: every derived grid) is that of the current state
    bool stepped;         // fcpt_step ran since the last fcpt_post
    bool cfl_interior;    // fcpt_cfl_begin evaluated the interior rings of the current state
    bool ghosts_unknown;  // a state grid was uploaded since the last boundary call
    bool qdiff_valid;     // Dev::qdiff holds Q+ - Q- of the grids (written by the last kick's march)
    // fcpt_run_steps (single slab): the final boundary call of the step just taken has not been launched yet -- the next
    // iteration's CFL launch carries it (k_cfl_rings_bc), or flush_deferred_boundary() does.  Never set when the function returns.
    bool bc_deferred;
    bool has_mid;         // leapfrog: fcpt_set_bodies_midstep gave the bodies at the mid-step time
    bool join_pending;    // fcpt_step_device_begin forked the interior transport to `side`: join_side() is owed
    bool march_source;    // the option of this name after apply_options()
    bool selfgravity;     // fcpt_selfgravity {in_step = 1}: every kick begins with the self-gravity kick
};

// the gated azimuthal launch of the fallback transport that enqueue_step left to the final boundary call of the step
// (fcpt_run_steps on one slab, StepPlan::gated_with_boundary): from enqueue_step to enqueue_post, inside one iteration
struct PendingGated {
    bool pending = false;
    GatedTheta launch;
};

struct fcpt_ctx {
    fcpt_desc d;
    fcpt_split s;
    HostGeometry geo;
    std::vector<double> radii;
    Dev P;
    LaunchState ls; // (zero-filled by fcpt_create)
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    double *d_cs_ring = nullptr;
    double *grid[FCPT_F_COUNT] = {};
    DampRange damp[4][2]; // [vrad, vaz, sigma, energy][inner, outer]
    DevClock *h_clk = nullptr; // pinned staging copy
    Profiler prof;
    bool profiling = false;
    // the dt of the next step is the CFL policy's (set by calculate_timestep*, consumed by the step):
    // with CFL <= 0.8 that keeps it inside the FARGO shear limit
    bool policy_dt_dev = false;
    double policy_dt_host = -1.0;
    bool damp_any = false;     // this slab holds rings of a damping zone
    std::vector<int> ring_ref_damped; // per ring: 1 if the folded damping loads reference values there (costlier rings of the transport)
    int *sm_sched_dev = nullptr;      // storage of Dev::sm_sched
    size_t sm_sched_cap = 0;          // ... in ints
    std::vector<int> sm_sched_host;
    std::vector<int> sm_lengths;      // explicit chunk lengths from row 0 upward (fcpt_set_source_chunks); empty: built-in
    int *tf_sched_dev = nullptr;      // storage of Dev::tf_sched
    size_t tf_sched_cap = 0;          // ... in ints
    std::vector<int> tf_lengths;      // explicit chunk lengths in dispatch order (fcpt_set_transport_chunks; FCPT_TF_SCHEDULE at fcpt_create); empty: built-in
    std::vector<int> tf_sched_host;   // what Dev::tf_sched holds
    bool damp_foldable = false; // ... and its damping can be folded into the transport (no "mean" target, Euler)
    // fcpt_step_device_begin: the interior chunks of the transport run on `side` while the caller's stream
    // marches the chunks with the neighbours' ghost rings, packs and sends them
    hipStream_t side = nullptr;
    hipEvent_t e_fork = nullptr, e_join = nullptr;
    // fcpt_disk_on_bodies_begin / _end: first-stage sums [body][block][4] followed by the 4 * FCPT_MAX_BODIES results
    // (allocated by the first call), their pinned host copy, the event behind the copy, the n of the pending call
    double *dob_part = nullptr, *dob_host = nullptr;
    hipEvent_t e_dob = nullptr;
    int dob_pending = 0;
    // leapfrog: bodies at the mid-step time (simulation.cpp:359-366; LaunchState::has_mid)
    double mx[FCPT_MAX_BODIES], my[FCPT_MAX_BODIES], mm[FCPT_MAX_BODIES], mrsm[FCPT_MAX_BODIES];
    // radial slabs over RCCL (fcpt_comm_init): communicator, packed ghost-ring buffers [send inner, send outer,
    // recv inner, recv outer], the device scalar of the MIN all-reduce, a stream for transfers that overlap the CFL
    Comm *comm = nullptr;
    double *xbuf[4] = {};
    double *d_cfl = nullptr;
    int peer_inner = -1, peer_outer = -1;
    hipStream_t comm_stream = nullptr;
    hipEvent_t e_packed = nullptr, e_received = nullptr;
    int device = 0; // HIP device the context was created on
    // dust particles (fcpt_particles.hip): device arrays and parameters of k_particles_step (part.n = 0: none), the ids
    // by slot, the one device block behind all of them
    ParticleArgs part = {};
    fcpt_particle_diffusion part_diff = {1, 0, 0, 0}; // outlives fcpt_particles_set; step counts fcpt_particles_step calls
    unsigned long long *part_id = nullptr;
    void *part_block = nullptr;
    // ParticleIntegrator (outlives fcpt_particles_set) and the explicit integrator's arrays: a block of their own, made
    // by fcpt_particles_timestep_init / _adaptive_set; part_adapt_set: the step size of every slot has been set since the
    // last fcpt_particles_set
    fcpt_particle_integrator part_integ = {0, 0, 0, 0};
    ParticleAdaptive part_adapt = {};
    void *part_adapt_block = nullptr;
    bool part_adapt_set = false;
    // fcpt_particles_follow_run_steps (outlives fcpt_particles_set): fcpt_run_steps queues the particle step of every
    // iteration; part_step_offset: the device word behind ParticleArgs::step_offset, made when first switched on
    bool part_follow = false;
    unsigned long long *part_step_offset = nullptr;
    // fcpt_particles_slabs (outlives fcpt_particles_set): the setting (its four totals live on the device: part_mtot), the
    // ownership window, and -- made when first switched on -- the messages [send inner, send outer, recv inner, recv
    // outer] of fcpt_exchange_count doubles each and the per-call counts of the emigration (ParticleMigrate::cnt)
    fcpt_particle_slabs part_slabs = {0, 0, 0, 0, 0, 0};
    double part_window[2] = {0.0, 0.0};
    double *part_mbuf[4] = {};
    unsigned int *part_mcnt = nullptr;
    unsigned long long *part_mtot = nullptr;
    // fcpt_run_steps on launch-bound grids: a captured hipGraph of `graph_cycle` consecutive steps (the out-of-place
    // transport swaps grid pointers, so the launch arguments repeat with period 2), replayed while the host-side state
    // that decided the launches (the whole Dev view, the whole LaunchState) is what it was at capture
    hipGraphExec_t graph_exec = nullptr;
    hipGraph_t graph = nullptr;
    hipStream_t capture_stream = nullptr;
    int graph_cycle = 0;
    long long graph_replays = 0; // hipGraphLaunch calls issued so far (read-only option "graph_replays")
    bool graph_failed = false;
    Dev graph_P;
    LaunchState graph_ls;
    ParticleLaunch graph_part = {}; // ... and the particle launch inside the cycle
    // self-gravity of the gas (fcpt_selfgravity.hip): the parameters (mode 0: off, everything below null), the device
    // side, and the allocations behind it -- made by fcpt_selfgravity, which drops a captured graph
    fcpt_selfgravity_params sg_params = {0, 0, 0.0, 0.0};
    SgDev sg = {};
    std::vector<void *> sg_allocs;
};


#define DOB_ROWS_HOST 8 /* = DOB_ROWS of k_disk_on_body */

namespace fcpt {

// routes this thread's launches to the context's profiler while it is recording
struct ProfScope {
    Profiler *outer;
    explicit ProfScope(fcpt_ctx *c) : outer(g_prof) { g_prof = c->profiling ? &c->prof : nullptr; }
    ~ProfScope() { g_prof = outer; }
};

template <class T> int dev_alloc(fcpt_ctx *c, T **p, size_t n)
{
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess) {
        set_error("hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
        return FCPT_ENOMEM;
    }
    e = hipMemset(q, 0, (n ? n : 1) * sizeof(T));
    if (e != hipSuccess) {
        set_error("hipMemset failed: %s", hipGetErrorString(e));
        return FCPT_EHIP;
    }
    c->allocs.push_back(q);
    *p = (T *)q;
    return FCPT_OK;
}

template <class T, class D> int dev_upload_raw(fcpt_ctx *c, D **dst, const std::vector<T> &src) // D: T or const T
{
    T *p = nullptr;
    if (int e = dev_alloc(c, &p, src.size()))
        return e;
    if (hipMemcpy(p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("hipMemcpy of a per-ring table failed");
        return FCPT_EHIP;
    }
    *dst = p;
    return FCPT_OK;
}

// fcpt_context.hip
void drop_graph(fcpt_ctx *c);
void join_side(fcpt_ctx *c);
int read_clock(fcpt_ctx *c, DevClock *out);
// fcpt_step.hip
void apply_boundary_view(fcpt_ctx *c, const Dev &P, bool final, bool damping_done = false);
void apply_boundary(fcpt_ctx *c, bool final);
void ensure_pressure(fcpt_ctx *c);
void enqueue_cfl(fcpt_ctx *c, int apply_policy);
void refresh_derived(fcpt_ctx *c);
void enqueue_step(fcpt_ctx *c, bool dt_dev, double dt, bool shear_safe, bool split = false, const StepPlan &plan = StepPlan(),
                  PendingGated *gated = nullptr);
void enqueue_post(fcpt_ctx *c, bool may_defer_boundary = false, const PendingGated *gated = nullptr);
void flush_deferred_boundary(fcpt_ctx *c);
// fcpt_particles.hip
void particles_free(fcpt_ctx *c);
int particles_loop_check(const fcpt_ctx *c);
void particles_loop_launch(const fcpt_ctx *c, ParticleLaunch *L);
void enqueue_particles_loop(fcpt_ctx *c);
bool particles_loop_migrates(const fcpt_ctx *c);
int enqueue_particles_migrate(fcpt_ctx *c);
// fcpt_selfgravity.hip
void selfgravity_free(fcpt_ctx *c);
void enqueue_selfgravity_compute(fcpt_ctx *c, const Dev &P);
void enqueue_selfgravity_kick(fcpt_ctx *c, const Dev &P, bool dt_from_clock, double dt); // compute + update_velocities
// fcpt_exchange.hip
int enqueue_exchange(fcpt_ctx *c);
int enqueue_cfl_allreduce(fcpt_ctx *c);

} // namespace fcpt
#endif
