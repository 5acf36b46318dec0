// Launch decisions of the step loop (fcpt_plan.h).  No HIP header, no allocation: the plans are a few comparisons, made
// once per step on grids whose steps are as short as the host's launch calls.
#include "fcpt_plan.h"

namespace fcpt {

bool cfl_by_rings(const Dev &P)
{
    // one block per ring: mean and cells in one pass (even Nphi up to 1024 * CFL_MAXP = 8192; the isothermal
    // viscosity and sound speed per ring, or the lazily derived ones of the ideal EOS)
    return (P.nphi & 1) == 0 && P.nphi >= 128 && P.nphi <= 1024 * CFL_MAXP && (!P.adiabatic || P.lazy_derived) &&
           P.stabilize != 2 && P.opt.cfl_rings != 0;
}

// (worth it only where the ring launch is several rounds of workgroups long -- measured, three / two A/B pairs each,
//  profiles/r03_ab_bc_in_cfl.txt: 2048 x 4096 isothermal 0.3311 against 0.3343 ms per step, ideal EOS 0.511 against
//  0.514; on a grid whose workgroups are all resident at once the four waiting ones start with the rest and spin:
//  512 x 1536 0.0755 against 0.0725, 1024 x 3072 ideal 0.223 against 0.222)
bool cfl_bc_mergeable(const Dev &P)
{
    return cfl_by_rings(P) && P.nr >= 8 && ((long long)P.nr * P.nphi >= BC_IN_CFL_FROM_CELLS || P.opt.bc_in_cfl == 2); // (2: tests)
}

// recalculate_derived_disk_quantities behind the boundary call launches kernels where the derived grids are not lazy
static bool derived_behind(const Dev &P) { return P.adiabatic && !P.lazy_derived; }

// when the call is nothing but the ghost-ring kernel on a final state (no damped rings left to damp, no derived grids to
// refresh behind it) and the next launch of the stream is the one-block-per-ring CFL kernel, that launch carries it
bool bc_rides_in_cfl(const Dev &P, const StepFacts &F, bool allowed, bool damping_done)
{
    return allowed && (damping_done || !F.slab_damped) && !derived_behind(P) && cfl_bc_mergeable(P);
}

StepPlan plan_device_step(const Dev &P, const StepFacts &F)
{
    StepPlan plan;
    // the fold of the CFL reduction inside the marching source kernel: Euler steps whose first launch behind the CFL
    // reduction -- but for k_potential, which reads no step length -- is that kernel; ring kernel of the reduction in use
    // (built-in: grids below 4 M cells -- measured, profiles/r03_ab_cfl_fold_in_source.txt: 512 x 1536 -2.4 %, 1024 x 3072
    //  ideal EOS -1.2 %; at 2048 x 4096 the 1 400 workgroups folding 48 KB each cost the kernel what the launch saved)
    // (particles: their launch stands between the CFL reduction and the gas step and reads the step length, which the
    //  fold would leave only in the source kernel's prologue: the policy launch)
    // (self-gravity: likewise -- its kick stands ahead of the source kernel and needs the final step length)
    const int want = P.opt.cfl_fold_in_source;
    const bool fold = (want < 0 ? (long long)P.nr * P.nphi < CFL_FOLD_BELOW_CELLS : want != 0) && !F.leapfrog && F.march_source && source_march_applies(P) && cfl_by_rings(P) && !F.particles && !F.selfgravity;
    plan.cfl_policy = fold ? 2 : 1;
    // the gated launch of the fallback transport together with the final boundary call, where that call will be
    // nothing but the ghost-ring kernel and does not ride in the next CFL launch (grids below 4 M cells)
    const bool damping_done = P.damp_in_step != 0; // (the step about to be queued sets `stepped`)
    const bool pure_bc = (damping_done || !F.damping_configured) && !derived_behind(P);
    plan.bc_rides_in_cfl = bc_rides_in_cfl(P, F, P.opt.bc_in_cfl != 0, damping_done);
    plan.gated_with_boundary = P.opt.gate_in_boundary != 0 && !F.leapfrog && pure_bc && !plan.bc_rides_in_cfl;
    return plan;
}

PostPlan plan_post(const Dev &P, const StepFacts &F, bool stepped, bool may_defer, bool gated_pending)
{
    PostPlan plan;
    // the damping of the final boundary call was applied by k_velocities when damp_in_step
    plan.damping_done = P.damp_in_step != 0 && stepped;
    plan.refresh_derived = derived_behind(P);
    const bool one_launch = plan.damping_done || !F.damping_configured;
    plan.pure_bc = one_launch && !plan.refresh_derived;
    plan.deferred = bc_rides_in_cfl(P, F, may_defer, plan.damping_done);
    // (a gated launch is only ever pending where plan_device_step found pure_bc, so `one_launch` decides as pure_bc would)
    plan.with_gated = gated_pending && !plan.deferred && one_launch;
    return plan;
}

} // namespace fcpt
