// Launch decisions of the step loop: which form of the CFL reduction runs, what rides in which launch, what the final
// boundary call of a step consists of.  Host arithmetic only (fcpt_plan.cpp includes no HIP header): fcpt_step.hip
// plans, then enqueues what the plan says; tests/step_plan_sweep.cpp holds the plans on a CPU.
#ifndef FCPT_PLAN_H
#define FCPT_PLAN_H

#include "fcpt_schedule.h"

// Shared by the kernels (kernels/cfl.h) and the planner.
#define CFL_MAXP 8 /* pairs of cells per thread of k_cfl_rings (Nphi <= 4096); 16 for rings up to 8192 cells */
#define CFL_FOLD_BELOW_CELLS (1ll << 22) /* built-in: the CFL fold inside the marching source kernel below this many cells ... */
#define BC_IN_CFL_FROM_CELLS (1ll << 22) /* ... the final boundary call inside the next CFL launch from this many up */

namespace fcpt {

// the one-block-per-ring kernel of the CFL reduction (k_cfl_rings) applies
bool cfl_by_rings(const Dev &P);
// ... and its form that carries the final boundary call of the step before (k_cfl_rings_bc) may run
bool cfl_bc_mergeable(const Dev &P);

// What the context knows besides the Dev view and its options.  The wave damping comes in two meanings:
//   damping_configured: the descriptor asks for it (fcpt_desc::damping) -- apply_boundary_view() goes through the damping
//                       launches when it is set, whether this slab holds damped rings or not.  Read by `pure_bc` and by
//                       the merge of the gated launch with the boundary call: they ask "is the call ONE launch".
//   slab_damped:        this slab holds rings of a damping zone (fcpt_ctx::damp_any).  Read by the rule that lets the
//                       boundary call ride in the next CFL launch (bc_rides_in_cfl), as by fcpt_cfl_begin: they ask
//                       "is the state final".
// (Without damped rings the damping launches are empty, so the first is only the stricter of the two.)
struct StepFacts {
    bool leapfrog;
    bool damping_configured, slab_damped;
    bool march_source;               // LaunchState's: the option after apply_options()
    bool particles;                  // fcpt_particles_follow_run_steps with particles: their launch stands behind the CFL launch
    bool selfgravity = false;        // fcpt_selfgravity {in_step = 1}: the kick begins with launches that read the step length
};

// One iteration of the device-resident loop (fcpt_run_steps without neighbours).  The first three are plan_device_step()'s;
// skip_q_store is the loop's own.  An ABI call steps with the defaults.
struct StepPlan {
    int cfl_policy = 1;               // argument of the CFL launch: 1: fold + time-step policy behind it, 2: the marching
                                      // source kernel queued next folds in its prologue (or enqueue_kick launches k_cfl_final)
    bool gated_with_boundary = false; // the transport leaves the gated launch of its fallback to the final boundary call
    bool bc_rides_in_cfl = false;     // that call may ride in the next iteration's CFL launch
    bool skip_q_store = false;        // not the call's last step: Dev::q_skip for its kick (Q+ / Q- are outputs only)
};
StepPlan plan_device_step(const Dev &P, const StepFacts &F);

// The final boundary call of a step and what follows it.
struct PostPlan {
    bool damping_done;    // the step's transport applied the wave damping (Dev::damp_in_step)
    bool pure_bc;         // the call is nothing but the ghost-ring kernel: no damping launches, no derived grids behind it
    bool deferred;        // it rides in the next CFL launch (fcpt_ctx::bc_deferred)
    bool with_gated;      // it and the pending gated launch are one launch
    bool refresh_derived; // the derived grids are recomputed behind it (ideal EOS without the marching source step)
};
// stepped: fcpt_step ran since the last fcpt_post; may_defer: the caller's next launch is a CFL reduction
PostPlan plan_post(const Dev &P, const StepFacts &F, bool stepped, bool may_defer, bool gated_pending);

// THE rule for the ride of the final boundary call in the next CFL launch (both plans call it)
bool bc_rides_in_cfl(const Dev &P, const StepFacts &F, bool allowed, bool damping_done);

} // namespace fcpt
#endif
