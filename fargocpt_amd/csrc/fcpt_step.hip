// The hot path of the C ABI (include/fargocpt_hip.h): CFL reduction, the gas step, the final boundary call and the
// run loop, with its hipGraph replay for launch-bound grids.
#include "fcpt_ctx.h"

using namespace fcpt;

namespace fcpt {

// boundary_conditions.cpp:65-114
void apply_boundary_view(fcpt_ctx *c, const Dev &P, bool final, bool damping_done)
{
    if (final && c->d.damping && !damping_done) {
        // damping.cpp:754-774, order of damping_vector: vrad, vaz, sigma, energy
        for (int o = 0; o < 2; ++o)
            launch_damping(P, P.vrad, P.vrad0, P.Rinf.p, c->damp[0][o], 0, c->stream);
        for (int o = 0; o < 2; ++o)
            launch_damping(P, P.vazi, P.vazi0, P.Rmed.p, c->damp[1][o], 0, c->stream);
        for (int o = 0; o < 2; ++o)
            launch_damping(P, P.sigma, P.sigma0, P.Rmed.p, c->damp[2][o], 1, c->stream);
        if (P.adiabatic)
            for (int o = 0; o < 2; ++o)
                launch_damping(P, P.energy, P.energy0, P.Rmed.p, c->damp[3][o], 0, c->stream);
    }
    launch_boundary(P, c->stream);
}
void apply_boundary(fcpt_ctx *c, bool final) { apply_boundary_view(c, c->P, final); }

// isothermal pressure is Sigma c_s^2 with c_s fixed per ring: the marching source kernel forms
// it in registers, so the grid is only materialised for callers that ask for it
// (ideal EOS with the marching source step: the same holds for T, c_s, H and nu)
static void ensure_pressure_view(fcpt_ctx *c, const Dev &P)
{
    if (!c->ls.pressure_valid) {
        if (P.adiabatic)
            launch_derived(P, c->stream);
        else
            launch_pressure(P, c->stream);
        c->ls.pressure_valid = true;
    }
}
void ensure_pressure(fcpt_ctx *c) { ensure_pressure_view(c, c->P); }

// recalculate_derived_disk_quantities: the derived grids now where kernels read them from the grids, else on request
void refresh_derived(fcpt_ctx *c)
{
    if (c->P.adiabatic && !c->P.lazy_derived) {
        launch_derived(c->P, c->stream);
        c->ls.pressure_valid = true;
    } else {
        c->ls.pressure_valid = false; // P only (ideal EOS: c_s, H, nu, T too), evaluated lazily
    }
}

} // namespace fcpt

namespace {

StepFacts step_facts(const fcpt_ctx *c)
{
    StepFacts F;
    F.leapfrog = c->d.integrator == FCPT_INTEGRATOR_LEAPFROG;
    F.damping_configured = c->d.damping != 0;
    F.slab_damped = c->damp_any;
    F.march_source = c->ls.march_source;
    F.particles = c->part_follow && c->part.n > 0;
    F.selfgravity = c->ls.selfgravity;
    return F;
}

// the four state grids as the ABI hands them out: wherever the out-of-place transport (or a rollback) left Dev's pointers
void sync_state_grids(fcpt_ctx *c)
{
    c->grid[FCPT_F_SIGMA] = c->P.sigma;
    c->grid[FCPT_F_VRAD] = c->P.vrad;
    c->grid[FCPT_F_VAZI] = c->P.vazi;
    c->grid[FCPT_F_ENERGY] = c->P.energy;
}

// where a kick left its result: the velocities always in (vrad_b, vazi_b)
struct KickResult {
    bool energy_in_b; // the energy in energy_b (marching source step, ideal EOS)
    int ring_parts;   // segments of ring sums of v_phi left by k_source_march (0: none)
    bool bc_folded;   // the kick applied the boundary conditions that follow it
};

// one gas "kick" (source terms, artificial viscosity, viscosity, SubStep3) with the step length currently in the device
// clock, launched with the view P.  fold_bc: and the boundary call that follows the first kick of a step;
// plan.cfl_policy == 2: the CFL fold + time-step policy of this step has not been launched yet; plan.skip_q_store
KickResult enqueue_kick(fcpt_ctx *c, const Dev &P, bool fold_bc, const StepPlan &plan)
{
    hipStream_t st = c->stream;
    KickResult r = {false, 0, false};
    const bool fold_pending = plan.cfl_policy == 2;
    // update_with_sourceterms begins with selfgravity::compute(data, dt, true) (SourceEuler.cpp:435-441): v += dt g in place,
    // launches of their own ahead of everything else (plan_device_step leaves no CFL fold pending with self-gravity)
    if (c->ls.selfgravity)
        enqueue_selfgravity_kick(c, P, true, 0.0);
    // one pass: (v[, e]) -> (v_b[, e_b])
    const bool fold_cfl = fold_pending && c->ls.march_source && source_march_applies(P);
    if (fold_pending && !fold_cfl)
        launch_cfl_final(P, 1, st);
    int segs = 0;
    if (c->ls.march_source && plan.skip_q_store && P.adiabatic && cfl_by_rings(P)) {
        Dev Q = P; // (Q+ and Q- themselves are read by nothing on the device in this configuration: the ring kernel of the CFL reduction takes their difference)
        Q.q_skip = 1;
        segs = launch_source_march(Q, st, fold_bc, &r.bc_folded, fold_cfl);
    } else if (c->ls.march_source) {
        segs = launch_source_march(P, st, fold_bc, &r.bc_folded, fold_cfl);
    }
    r.ring_parts = segs > 0 ? segs : 0;
    r.energy_in_b = segs != 0 && P.adiabatic;
    c->ls.qdiff_valid = segs != 0 && P.adiabatic; // the march wrote Q+ - Q- beside Q+ and Q-; the three fused kernels do not
    if (!segs) {
        ensure_pressure_view(c, P);
        launch_source_fused(P, st);          // (v) -> (v_b) -> (v)
        launch_recalculate_viscosity(P, st);
        launch_visc_factors(P, st);          // StabilizeViscosity: from nu and Sigma, for k_visc_fused (1) and the CFL reduction (2)
        launch_viscous_fused(P, st);         // (v) -> (v_b); ideal EOS: + viscous heating + SubStep3
    }
    return r;
}

// the bodies at the mid-step time (fcpt_set_bodies_midstep) into a view
void set_mid_bodies(const fcpt_ctx *c, Dev &M)
{
    for (int k = 0; k < M.nbodies; ++k) {
        M.bx[k] = c->mx[k];
        M.by[k] = c->my[k];
        M.bm[k] = c->mm[k];
        M.brsm[k] = c->mrsm[k];
    }
}

void enqueue_potential(fcpt_ctx *c, bool midstep)
{
    Dev &P = c->P;
    // the mid-step potential of step_LeapFrog sees the scale height of the first kick (left in the
    // grid by k_source_march_adi), not one derived from the transported state
    const bool kick_height = midstep && P.adiabatic && P.lazy_derived;
    if (kick_height || (midstep && c->ls.has_mid)) {
        Dev M = P;
        if (kick_height)
            M.lazy_derived = 0;
        if (c->ls.has_mid)
            set_mid_bodies(c, M);
        launch_body_force(M, c->stream);
        c->ls.potential_valid = false; // the grid now holds the mid-step potential
        return;
    }
    if (P.inline_potential) { // k_source_march_adi evaluates it ring by ring; the grid is only filled on request
        c->ls.potential_valid = false;
        return;
    }
    if (P.adiabatic || !c->ls.potential_valid) {
        launch_body_force(P, c->stream); // CalculateNbodyPotential | CalculateAccelOnGas; static when H and the bodies are
        c->ls.potential_valid = true;
    }
}

} // namespace

namespace fcpt {

// the gas part of step_Euler up to Transport (simulation.cpp:167-217), or of step_LeapFrog
// (simulation.cpp:316-393): kick 1/2 (dt/2), drift (dt), kick 2/2 (dt/2).  `dt_dev`: the step length is in the device
// clock.  plan: what fcpt_run_steps asks of this step (an ABI call: the defaults); gated: where the transport may leave
// the gated launch of its fallback (plan.gated_with_boundary)
void enqueue_step(fcpt_ctx *c, bool dt_dev, double dt, bool shear_safe, bool split, const StepPlan &plan, PendingGated *gated)
{
    join_side(c);
    c->ls.cfl_interior = false;
    const Dev &P = c->P;
    hipStream_t st = c->stream;
    const bool frog = c->d.integrator == FCPT_INTEGRATOR_LEAPFROG;
    if (frog)
        launch_clock_scale_dt(P.clk, dt_dev ? 1 : 0, dt, 0.5, st); // dt <- step/2, keeps step in cfl_dt
    else if (!dt_dev)
        launch_clock_set_dt(P.clk, dt, st);
    enqueue_potential(c, false);
    // (after an upload of a state grid the ghost rings may not satisfy the boundary conditions yet: the folded form
    //  rewrites Sigma's ghost ring while neighbouring wavefronts may still read it -- harmless only when the values
    //  are the ones already there, so that one step takes the separate launch)
    //  likewise a second fcpt_step without fcpt_post in between: the ghost rings are the transport's, not a boundary call's)
    const KickResult k1 = enqueue_kick(c, P, !c->ls.ghosts_unknown && !c->ls.stepped, plan);
    c->ls.ghosts_unknown = false;
    Dev Q = P; // view with the post-kick velocities
    Q.vrad = P.vrad_b;
    Q.vazi = P.vazi_b;
    if (k1.energy_in_b)
        Q.energy = P.energy_b;
    Q.src_ring_nparts = k1.ring_parts; // ring sums of v_phi left by k_source_march
    if (!k1.bc_folded) // (else the source march applied it on its edge chunks)
        apply_boundary_view(c, Q, false);
    if (frog)
        launch_clock_scale_dt(P.clk, 2, 0.0, 1.0, st); // dt <- step (saved in cfl_dt)
    launch_massflow(Q, st); // WriteMassFlow: what this Transport() carries through the interfaces
    TransportResult tr;
    if (split && !frog && transport_can_split(Q, device_cus(), shear_safe) && c->side) {
        launch_shift_means(Q, st);
        (void)hipEventRecord(c->e_fork, st);
        (void)hipStreamWaitEvent(c->side, c->e_fork, 0);
        (void)launch_transport(Q, P, c->side, TRANSPORT_INTERIOR);
        (void)hipEventRecord(c->e_join, c->side);
        tr = launch_transport(Q, P, st, TRANSPORT_EDGES);
        c->ls.join_pending = true;
    } else {
        const bool leave_gated = gated && plan.gated_with_boundary && !frog;
        tr = launch_transport(Q, P, st, TRANSPORT_ALL, leave_gated ? &gated->launch : nullptr);
        if (gated)
            gated->pending = tr.gated_pending != 0;
    }
    if (!tr.marched)
        launch_clock_advance(P.clk, st);
    // the marching transport is out of place: the new state may sit in the scratch twins
    if (tr.sigma != c->P.sigma)
        std::swap(c->P.sigma, c->P.sigA);
    if (tr.energy != c->P.energy)
        std::swap(c->P.energy, c->P.eA);
    if (tr.vrad != c->P.vrad)
        std::swap(c->P.vrad, c->P.vrad_b);
    if (tr.vazi != c->P.vazi)
        std::swap(c->P.vazi, c->P.vazi_b);
    sync_state_grids(c);
    if (frog) {
        launch_clock_scale_dt(P.clk, 2, 0.0, 0.5, st); // dt <- step/2
        enqueue_potential(c, true);
        c->ls.pressure_valid = false; // compute_pressure(data), simulation.cpp:378
        if (P.adiabatic && !P.lazy_derived)
            ensure_pressure(c);
        Dev K = P;
        K.kick_time_shift = 1; // SubStep3 of the second kick runs at midstep_time (simulation.cpp:388)
        const KickResult k2 = enqueue_kick(c, K, false, StepPlan());
        // the result is in the *_b buffers: bring it home
        const size_t ns = (size_t)P.nr * P.nphi * sizeof(double), nv = (size_t)(P.nr + 1) * P.nphi * sizeof(double);
        (void)hipMemcpyAsync(P.vrad, P.vrad_b, nv, hipMemcpyDeviceToDevice, st);
        (void)hipMemcpyAsync(P.vazi, P.vazi_b, ns, hipMemcpyDeviceToDevice, st);
        if (k2.energy_in_b)
            (void)hipMemcpyAsync(P.energy, P.energy_b, ns, hipMemcpyDeviceToDevice, st);
        launch_clock_scale_dt(P.clk, 2, 0.0, 1.0, st); // dt <- step, for the damping of the final boundary call
    }
    c->ls.stepped = true;
}

void flush_deferred_boundary(fcpt_ctx *c)
{
    if (c->ls.bc_deferred) {
        c->ls.bc_deferred = false;
        launch_boundary(c->P, c->stream);
    }
}

void enqueue_post(fcpt_ctx *c, bool may_defer_boundary, const PendingGated *gated)
{
    join_side(c);
    const bool gated_pending = gated && gated->pending; // (enqueue_device_step asked the transport to leave its gated fallback launch to this call)
    const PostPlan plan = plan_post(c->P, step_facts(c), c->ls.stepped, may_defer_boundary, gated_pending);
    if (gated_pending)
        launch_gated_theta(gated->launch, plan.with_gated ? &c->P : nullptr, c->stream); // with_gated: one launch for both
    if (plan.deferred)
        c->ls.bc_deferred = true;
    else if (!plan.with_gated)
        apply_boundary_view(c, c->P, true, plan.damping_done);
    c->ls.stepped = false;
    refresh_derived(c);
}

void enqueue_cfl(fcpt_ctx *c, int apply_policy)
{
    join_side(c);
    c->P.qdiff_on = c->ls.qdiff_valid ? 1 : 0;
    if (c->ls.bc_deferred && !c->ls.cfl_interior && cfl_bc_mergeable(c->P)) {
        c->ls.bc_deferred = false;
        launch_cfl_bc(c->P, apply_policy, c->stream); // + the final boundary call of the step before
    } else {
        flush_deferred_boundary(c);
        launch_cfl(c->P, apply_policy, c->stream, c->ls.cfl_interior);
    }
    c->ls.cfl_interior = false;
}

} // namespace fcpt

extern "C" {

// condition_cfl for the rings that neither the ghost exchange nor the boundary kernels touch, to be queued between
// fcpt_exchange_pack and the wait for the neighbours' rings: it runs while they are on the wire.  The next
// fcpt_cfl / fcpt_cfl_device evaluates the remaining rings and reduces.  A no-op (the whole CFL runs later)
// whenever that split would not see the final state: damping outside the step kernels, narrow rings, ...
int fcpt_cfl_begin(fcpt_ctx *c)
{
    if (!c)
        return FCPT_EINVAL;
    join_side(c);
    c->ls.cfl_interior = false;
    const bool state_final = c->ls.stepped && (!c->damp_any || c->P.damp_in_step != 0); // fcpt_post will not damp
    if (!state_final)
        return FCPT_OK;
    if (c->P.opt.cfl_split == 0)
        return FCPT_OK;
    ProfScope prof_scope(c);
    c->P.qdiff_on = c->ls.qdiff_valid ? 1 : 0;
    c->ls.cfl_interior = launch_cfl_interior(c->P, c->stream);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_cfl(fcpt_ctx *c, double *dt_local)
{
    if (!c || !dt_local)
        return FCPT_EINVAL;
    ProfScope prof_scope(c);
    enqueue_cfl(c, 0);
    HIPCHK(hipGetLastError());
    DevClock k;
    if (int rc = read_clock(c, &k))
        return rc;
    double v;
    std::memcpy(&v, &k.cfl_bits, sizeof(v));
    *dt_local = v;
    return FCPT_OK;
}

int fcpt_cfl_device(fcpt_ctx *c, double *d_dt_local)
{
    if (!c || !d_dt_local)
        return FCPT_EINVAL;
    ProfScope prof_scope(c);
    enqueue_cfl(c, 0);
    launch_clock_export_cfl(c->P.clk, d_dt_local, c->stream);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_calculate_timestep_device(fcpt_ctx *c, const double *d_cfl_global)
{
    if (c && !d_cfl_global)
        d_cfl_global = c->d_cfl; // what fcpt_cfl_allreduce left
    if (!c || !d_cfl_global)
        return FCPT_EINVAL;
    ProfScope prof_scope(c);
    launch_clock_policy_ptr(c->P.clk, c->d.cfl_max_var, d_cfl_global, c->stream);
    c->policy_dt_dev = true;
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_step_device(fcpt_ctx *c)
{
    if (!c)
        return FCPT_EINVAL;
    ProfScope prof_scope(c);
    enqueue_step(c, true, 0.0, c->policy_dt_dev && c->d.cfl <= 0.8);
    c->policy_dt_dev = false;
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

// fcpt_step_device for slabs with neighbours: the chunks of the transport that hold the rings the neighbours are
// waiting for (rows [7,14), [nr-14,nr-7)) are marched on the caller's stream, all others on an internal stream,
// so that fcpt_exchange_pack and the transfers queued next run under the interior chunks.  Until
// fcpt_step_device_end only fcpt_exchange_pack may be called.
int fcpt_step_device_begin(fcpt_ctx *c)
{
    if (!c)
        return FCPT_EINVAL;
    if (!c->side) {
        HIPCHK(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->e_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->e_join, hipEventDisableTiming));
    }
    ProfScope prof_scope(c);
    enqueue_step(c, true, 0.0, c->policy_dt_dev && c->d.cfl <= 0.8, true);
    c->policy_dt_dev = false;
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_step_device_end(fcpt_ctx *c)
{
    if (!c)
        return FCPT_EINVAL;
    join_side(c);
    return FCPT_OK;
}

int fcpt_post_device(fcpt_ctx *c)
{
    if (!c)
        return FCPT_EINVAL;
    join_side(c);
    ProfScope prof_scope(c);
    enqueue_post(c);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_calculate_timestep(fcpt_ctx *c, double cfl_dt_global, double *dt)
{
    if (!c || !dt)
        return FCPT_EINVAL;
    launch_clock_policy(c->P.clk, c->d.cfl_max_var, 0, cfl_dt_global, c->stream);
    DevClock k;
    if (int rc = read_clock(c, &k))
        return rc;
    *dt = k.last_dt;
    c->policy_dt_host = k.last_dt;
    return FCPT_OK;
}

int fcpt_snap_to_monitor(const fcpt_ctx *cc, double cfl_dt, double *step_dt)
{
    fcpt_ctx *c = const_cast<fcpt_ctx *>(cc);
    if (!c || !step_dt)
        return FCPT_EINVAL;
    DevClock k;
    if (int rc = read_clock(c, &k))
        return rc;
    // simulation.cpp:528-540
    const double time_next_monitor = (k.n_monitor + 1) * c->d.monitor_timestep;
    const double time_left_till_write = time_next_monitor - k.time;
    const bool overshoot = cfl_dt > time_left_till_write;
    const double dt_stretch_factor = 0.05;
    const bool almost_there = time_left_till_write < cfl_dt * (1 + dt_stretch_factor);
    *step_dt = (overshoot || almost_there) ? time_left_till_write : cfl_dt;
    return FCPT_OK;
}

int fcpt_step(fcpt_ctx *c, double dt)
{
    if (!c)
        return FCPT_EINVAL;
    ProfScope prof_scope(c);
    enqueue_step(c, false, dt, c->policy_dt_host > 0.0 && dt <= c->policy_dt_host * (1.0 + 1e-12) && c->d.cfl <= 0.8);
    c->policy_dt_host = -1.0;
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_post(fcpt_ctx *c, double dt)
{
    if (!c)
        return FCPT_EINVAL;
    ProfScope prof_scope(c);
    launch_clock_set_dt(c->P.clk, dt, c->stream);
    enqueue_post(c);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_apply_boundary(fcpt_ctx *c, double dt, int32_t final)
{
    if (!c)
        return FCPT_EINVAL;
    join_side(c);
    ProfScope prof_scope(c);
    launch_clock_set_dt(c->P.clk, dt, c->stream);
    apply_boundary(c, final != 0);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

} // extern "C"
namespace {
bool graph_wanted(const fcpt_ctx *c)
{
    if (c->profiling || c->graph_failed || c->comm)
        return false;
    if (c->P.opt.graph_steps >= 0)
        return c->P.opt.graph_steps != 0;
    // launch-bound grids: the kernels of a step are shorter than the host's launch calls
    return (long long)c->P.nr * c->P.nphi <= 131072;
}
// one iteration of the device-resident loop: CFL reduction -> policy kernel -> step -> post, as plan_device_step() has it
void enqueue_device_step(fcpt_ctx *c, bool skip_q_store = false)
{
    const StepFacts F = step_facts(c);
    StepPlan plan = plan_device_step(c->P, F);
    plan.skip_q_store = skip_q_store;
    enqueue_cfl(c, plan.cfl_policy);
    // the particle step where the reference has it (simulation.cpp:177-180): the step length is in force, the final
    // boundary call of the step before has run (inside the CFL launch or ahead of it), the gas is that of the start of
    // the step
    if (F.particles)
        enqueue_particles_loop(c);
    PendingGated gated;
    enqueue_step(c, true, 0.0, c->d.cfl <= 0.8, false, plan, &gated);
    enqueue_post(c, c->P.opt.bc_in_cfl != 0, &gated); // (the boundary call may ride in the next iteration's CFL launch)
}
// capture `cycle` steps; true if the host-side state is back where it started (the graph can be replayed)
bool capture_graph(fcpt_ctx *c, int cycle)
{
    if (!c->capture_stream && hipStreamCreateWithFlags(&c->capture_stream, hipStreamNonBlocking) != hipSuccess)
        return false;
    const Dev P0 = c->P;
    const LaunchState ls0 = c->ls;
    hipStream_t user = c->stream;
    c->stream = c->capture_stream;
    bool ok = hipStreamBeginCapture(c->capture_stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        for (int n = 0; n < cycle; ++n)
            enqueue_device_step(c);
        hipGraph_t g = nullptr;
        ok = hipStreamEndCapture(c->capture_stream, &g) == hipSuccess && g != nullptr;
        c->graph = g;
    }
    c->stream = user;
    (void)hipGetLastError();
    const bool periodic = std::memcmp(&P0, &c->P, sizeof(Dev)) == 0 && std::memcmp(&ls0, &c->ls, sizeof(LaunchState)) == 0;
    if (ok && periodic)
        ok = hipGraphInstantiate(&c->graph_exec, c->graph, nullptr, nullptr, 0) == hipSuccess;
    if (!ok || !periodic) {
        // nothing was executed during the capture: put the host-side view back and step without a graph
        c->P = P0;
        c->ls = ls0;
        sync_state_grids(c);
        drop_graph(c);
        return false;
    }
    c->graph_cycle = cycle;
    c->graph_P = c->P;
    c->graph_ls = ls0;
    particles_loop_launch(c, &c->graph_part);
    return true;
}
} // namespace
extern "C" {

// sim::run's loop (simulation.cpp:515-553) for a single slab.
int fcpt_run_steps(fcpt_ctx *c, int64_t nsteps, int32_t snap, int64_t *done)
{
    if (!c)
        return FCPT_EINVAL;
    ProfScope prof_scope(c);
    int64_t n = 0;
    if (int rc = particles_loop_check(c)) { // fcpt_particles_follow_run_steps: refused before anything is queued
        if (done)
            *done = 0;
        return rc;
    }
    const bool slabs = c->comm && (c->peer_inner >= 0 || c->peer_outer >= 0); // this slab has neighbours
    // fcpt_particles_follow_run_steps: the device loop counts the particle steps itself (the kernels add the clock's
    // iteration count to an offset left here, once, outside any graph), and the host's counter follows when the steps are
    // queued; the host-stepped branch calls fcpt_particles_step, which counts; without particles the counter still advances
    const bool follow = c->part_follow, follow_dev = follow && !slabs && !snap && c->part.n > 0;
    // ... on several slabs (particles_loop_check: a communicator and fcpt_particles_slabs): the step and the migration
    const bool follow_slabs = slabs && particles_loop_migrates(c);
    // set by the branches that call fcpt_particles_step, which counts every call, also one without particles
    bool counted_by_particles_step = false;
    if ((follow_dev || (follow_slabs && !snap && c->part.n > 0)) && nsteps > 0)
        launch_particles_counter_offset(c->part_step_offset, c->part_diff.step, c->P.clk, c->stream);
    if (slabs && !snap) {
        // several slabs, dt never leaves the device: CFL -> MIN over the slabs (cfl.cpp:379) -> policy kernel
        // [-> particle step -> migration] -> step -> ghost exchange (simulation.cpp:236) -> post, all on one stream
        for (; n < nsteps; ++n) {
            if (int rc = enqueue_cfl_allreduce(c))
                return rc;
            launch_clock_policy_ptr(c->P.clk, c->d.cfl_max_var, c->d_cfl, c->stream);
            if (follow_slabs) {
                // the particle step where the reference has it (simulation.cpp:177-180), in its clock-reading slab form
                // (none without particles), then particles::move's hand-over; every slab issues the collective in every
                // iteration, with or without particles.
                // The migration's neighbour exchange is queued on the context's stream, like the all-reduce above.  With
                // comm_overlap the ghost exchange runs on the communication stream, and still no two calls of this
                // communicator can overlap: the context's stream has waited for the previous ghost exchange (e_received,
                // enqueue_exchange) before anything of this iteration, and the next ghost exchange waits for e_packed,
                // which enqueue_exchange records on the context's stream behind this migration.
                enqueue_particles_loop(c);
                if (int rc = enqueue_particles_migrate(c))
                    return rc;
            }
            StepPlan plan;
            plan.skip_q_store = c->d.integrator != FCPT_INTEGRATOR_LEAPFROG && n + 1 < nsteps; // Q+ / Q- (outputs) by the last step only
            enqueue_step(c, true, 0.0, c->d.cfl <= 0.8, false, plan);
            if (int rc = enqueue_exchange(c))
                return rc;
            enqueue_post(c);
        }
        HIPCHK(hipGetLastError());
    } else if (!snap) {
        // dt never leaves the device: CFL reduction -> policy kernel -> step -> post
        if (graph_wanted(c) && nsteps >= 8) {
            join_side(c);
            // A captured cycle is replayed while the host-side state that decided its launches (the whole Dev view, the
            // whole LaunchState) is what it was at capture: bodies, options, uploads change it for good; the parity
            // of the transport's ping-pong and the boundary call that rides in the next CFL launch (deferred inside
            // this function only) are put back by one or two plain steps -- the same two that let the lazily evaluated
            // grids settle before the first capture.
            // The particle launch of the cycle (fcpt_particles_follow_run_steps) is compared as a whole too: the flag, the
            // arrays and parameters of fcpt_particles_set, the drag, diffusion and integrator settings, the adaptive block.
            ParticleLaunch part_now;
            particles_loop_launch(c, &part_now);
            auto valid = [&] {
                return c->graph_exec && std::memcmp(&c->graph_P, &c->P, sizeof(Dev)) == 0 &&
                       std::memcmp(&c->graph_ls, &c->ls, sizeof(LaunchState)) == 0 &&
                       std::memcmp(&c->graph_part, &part_now, sizeof(ParticleLaunch)) == 0;
            };
            for (int lead = 0; lead < 2 && !valid(); ++lead, ++n)
                enqueue_device_step(c);
            if (!valid()) {
                drop_graph(c);
                if (!capture_graph(c, 2) && !capture_graph(c, 4))
                    c->graph_failed = true;
            }
            if (c->graph_exec) {
                for (; n + c->graph_cycle <= nsteps; n += c->graph_cycle) {
                    HIPCHK(hipGraphLaunch(c->graph_exec, c->stream));
                    ++c->graph_replays;
                }
            }
        }
        const bool frog_loop = c->d.integrator == FCPT_INTEGRATOR_LEAPFROG;
        for (; n < nsteps; ++n)
            enqueue_device_step(c, !frog_loop && n + 1 < nsteps); // Q+ / Q- (outputs) by the last step only
        flush_deferred_boundary(c); // the last step's boundary call has no CFL launch to ride in
        HIPCHK(hipGetLastError());
    } else {
        // monitor-time snapping: the (reduced) dt comes to the host, as in sim::run.  Several slabs: MIN over the slabs,
        // particles::move behind the particle step, the ghost exchange between the step and its final boundary call
        const bool particles = slabs ? follow_slabs : follow;
        const double t_final = (double)c->d.nsnapshots * c->d.nmonitor * c->d.monitor_timestep;
        for (; n < nsteps; ++n) {
            DevClock k;
            if (int rc = read_clock(c, &k))
                return rc;
            if (t_final > 0 && !(k.time < t_final))
                break;
            double cfl_dt, dt, step_dt;
            if (int rc = slabs ? fcpt_cfl_allreduce(c, &cfl_dt) : fcpt_cfl(c, &cfl_dt))
                return rc;
            if (int rc = fcpt_calculate_timestep(c, cfl_dt, &dt))
                return rc;
            if (int rc = fcpt_snap_to_monitor(c, dt, &step_dt))
                return rc;
            const double time_next_monitor = (k.n_monitor + 1) * c->d.monitor_timestep;
            if (particles) { // simulation.cpp:177-180, with the indirect term of the last fcpt_set_bodies
                counted_by_particles_step = true;
                if (int rc = fcpt_particles_step(c, step_dt, c->P.indirect_x, c->P.indirect_y, c->d.omega_frame * step_dt))
                    return rc;
                if (slabs)
                    if (int rc = fcpt_particles_migrate(c))
                        return rc;
            }
            if (int rc = fcpt_step(c, step_dt))
                return rc;
            if (slabs)
                if (int rc = fcpt_exchange(c))
                    return rc;
            if (int rc = fcpt_post(c, step_dt))
                return rc;
            if (int rc = read_clock(c, &k))
                return rc;
            if (std::fabs(time_next_monitor - k.time) < 1e-6 * dt) {
                fcpt_clock hc = {k.time, k.last_dt, k.n_hydro_iter, k.n_monitor + 1, 0};
                hc.n_snapshot = hc.n_monitor / (uint32_t)(c->d.nmonitor > 0 ? c->d.nmonitor : 1);
                if (int rc = fcpt_set_clock(c, &hc))
                    return rc;
            }
        }
    }
    if (follow && !counted_by_particles_step) // the loops that queue the step themselves, or none: one count per iteration
        c->part_diff.step += (unsigned long long)n;
    if (done)
        *done = n;
    return FCPT_OK;
}

} // extern "C"
