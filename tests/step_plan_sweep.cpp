// Stand-alone sweep of the step planner (fargocpt_amd/csrc/fcpt_plan.cpp, linked with fcpt_schedule.cpp alone): the plans of
// an iteration of the device loop and of the post stage over grids, physics and options, held to properties that are stated
// here without looking at how the planner arrives at them.  Built and run by tests/test_step_plan_sweep.py with the address
// and undefined-behaviour sanitizers.  Exit status 0 and nothing on stderr: all plans passed.
#include <cstdio>
#include <cstring>

#include "../fargocpt_amd/csrc/fcpt_plan.h"

using namespace fcpt;

static int failures = 0;
static char what[320];
static void fail(const char *msg)
{
    if (++failures <= 20)
        std::fprintf(stderr, "%s: %s\n", what, msg);
}
#define CHECK(cond, msg) \
    do {                 \
        if (!(cond))     \
            fail(msg);   \
    } while (0)

enum Damping { DAMP_OFF, DAMP_FOLDABLE, DAMP_MEAN_TARGET, DAMP_UNFUSED, DAMP_OTHER_SLABS, DAMP_MODES };
// (DAMP_OTHER_SLABS: the descriptor asks for damping, this slab holds none of the damped rings)

struct Case {
    int nr, nphi, adiabatic, lazy_wanted, leapfrog, damping, stabilize, particles;
    int cfl_rings, fold, bc_in_cfl, gate;
};

// the context's switches as fcpt_create / fcpt_set_option derive them (apply_options, build_ring_tables)
static void make(const Case &k, Dev &P, StepFacts &F)
{
    std::memset(&P, 0, sizeof(P));
    std::memset(&P.opt, 0xff, sizeof(P.opt)); // every switch -1: the built-in choice
    P.nr = k.nr, P.nphi = k.nphi, P.adiabatic = k.adiabatic, P.stabilize = k.stabilize, P.leapfrog = k.leapfrog;
    P.opt.march_source_adi = k.lazy_wanted;
    P.opt.cfl_rings = k.cfl_rings, P.opt.cfl_fold_in_source = k.fold, P.opt.bc_in_cfl = k.bc_in_cfl, P.opt.gate_in_boundary = k.gate;
    const bool march_runs = k.nphi >= 128 && (!k.adiabatic || k.lazy_wanted);
    P.lazy_derived = k.adiabatic && march_runs;
    const bool foldable = k.damping == DAMP_FOLDABLE && !k.leapfrog;
    P.damp_in_step = foldable;
    F.leapfrog = k.leapfrog != 0;
    F.damping_configured = k.damping != DAMP_OFF;
    F.slab_damped = k.damping != DAMP_OFF && k.damping != DAMP_OTHER_SLABS;
    F.march_source = true; // the option of this name, at its default
    F.particles = k.particles != 0;
}

static void check(const Case &k)
{
    Dev P;
    StepFacts F;
    make(k, P, F);
    std::snprintf(what, sizeof(what), "%d x %d, ideal %d (lazy %d), leapfrog %d, damping %d, stabilize %d, particles %d, cfl_rings %d, fold %d, bc_in_cfl %d, gate %d",
                  k.nr, k.nphi, k.adiabatic, P.lazy_derived, k.leapfrog, k.damping, k.stabilize, k.particles, k.cfl_rings, k.fold, k.bc_in_cfl, k.gate);
    const long long cells = (long long)k.nr * k.nphi, four_m = 1ll << 22;
    // what the kernels can do, restated from their own limits
    const bool ring_kernel = k.nphi % 2 == 0 && k.nphi >= 128 && k.nphi <= 8192 && (!k.adiabatic || P.lazy_derived) && k.stabilize != 2 && k.cfl_rings != 0;
    const bool march = F.march_source && k.nphi >= 128 && (!k.adiabatic || k.lazy_wanted);
    const bool merged_kernel = ring_kernel && k.nr >= 8 && (cells >= four_m || k.bc_in_cfl == 2);
    const bool derived_behind = k.adiabatic && !P.lazy_derived;
    const bool damping_launches = F.slab_damped && !P.damp_in_step; // k_damping launches are due in the boundary call
    const bool damping_calls = F.damping_configured && !P.damp_in_step; // ... or at least gone through

    CHECK(cfl_by_rings(P) == ring_kernel, "cfl_by_rings");
    CHECK(cfl_bc_mergeable(P) == merged_kernel, "cfl_bc_mergeable");
    CHECK(source_march_applies(P) == (k.nphi >= 128 && (!k.adiabatic || k.lazy_wanted)), "source_march_applies");

    const StepPlan s = plan_device_step(P, F);
    CHECK(s.cfl_policy == 1 || s.cfl_policy == 2, "the CFL policy argument is 1 or 2");
    CHECK(!s.skip_q_store, "skip_q_store is the loop's");
    const bool fold = s.cfl_policy == 2, fold_possible = !k.leapfrog && march && ring_kernel && !k.particles;
    CHECK(!fold || fold_possible, "a fold in the source march without Euler, the march, the ring kernel, or with particles");
    if (k.fold < 0)
        CHECK(fold == (fold_possible && cells < four_m), "built-in fold: exactly below 4 M cells");
    else
        CHECK(fold == (fold_possible && k.fold != 0), "fold as the option says");

    CHECK(!(s.gated_with_boundary && s.bc_rides_in_cfl), "the gated launch merged with a boundary call that rides in the CFL launch");
    if (derived_behind || damping_launches)
        CHECK(!s.gated_with_boundary && !s.bc_rides_in_cfl, "a merge although derived grids or damping launches stand behind the boundary call");
    CHECK(!s.bc_rides_in_cfl || merged_kernel, "a ride without k_cfl_rings_bc");
    CHECK(!s.bc_rides_in_cfl || k.bc_in_cfl != 0, "a ride with bc_in_cfl 0");
    CHECK(!(s.bc_rides_in_cfl && k.bc_in_cfl == 1) || cells >= four_m, "bc_in_cfl 1: a ride below 4 M cells");
    CHECK(s.bc_rides_in_cfl == (k.bc_in_cfl != 0 && merged_kernel && !derived_behind && !damping_launches), "the ride, exactly");
    CHECK(s.gated_with_boundary == (k.gate != 0 && !k.leapfrog && !derived_behind && !damping_calls && !s.bc_rides_in_cfl), "the gated merge, exactly");

    // the post stage of that iteration (stepped, the loop may defer) agrees with the plan of the iteration
    for (int stepped = 0; stepped < 2; ++stepped)
        for (int may_defer = 0; may_defer < 2; ++may_defer)
            for (int pending = 0; pending < 2; ++pending) {
                const PostPlan p = plan_post(P, F, stepped != 0, may_defer != 0, pending != 0);
                CHECK(p.damping_done == (P.damp_in_step && stepped), "damping_done");
                CHECK(p.refresh_derived == derived_behind, "refresh_derived");
                CHECK(p.pure_bc == (!derived_behind && (p.damping_done || !F.damping_configured)), "pure_bc");
                CHECK(!p.deferred || may_defer, "deferred unasked");
                CHECK(!p.deferred || (merged_kernel && !derived_behind && (p.damping_done || !F.slab_damped)), "deferred with work behind the call");
                CHECK(!(p.deferred && p.with_gated), "deferred and merged with the gated launch");
                CHECK(!p.with_gated || pending, "with_gated without a pending launch");
                if (stepped && may_defer == (k.bc_in_cfl != 0)) {
                    CHECK(p.deferred == s.bc_rides_in_cfl, "the post stage and the iteration disagree on the ride");
                    if (pending && s.gated_with_boundary)
                        CHECK(p.with_gated, "the gated launch the iteration left to the boundary call is not merged with it");
                }
            }
}

// the two headline grids of the benchmark: planet_disk, isothermal, Euler, reference damping folded into the transport
static void check_headline(int nr, int nphi, int policy, bool rides, bool gated)
{
    const Case k = {nr, nphi, 0, 1, 0, DAMP_FOLDABLE, 0, 0, 1, -1, 1, 1};
    Dev P;
    StepFacts F;
    make(k, P, F);
    std::snprintf(what, sizeof(what), "headline %d x %d", nr, nphi);
    const StepPlan s = plan_device_step(P, F);
    CHECK(s.cfl_policy == policy, "CFL policy");
    CHECK(s.bc_rides_in_cfl == rides, "ride in the CFL launch");
    CHECK(s.gated_with_boundary == gated, "gated launch with the boundary call");
    const PostPlan p = plan_post(P, F, true, true, gated);
    CHECK(p.deferred == rides && p.with_gated == gated && p.pure_bc && !p.refresh_derived && p.damping_done, "post stage");
}

int main()
{
    const int NR[] = {8, 20, 32, 2048};
    const int NPHI[] = {64, 126, 128, 256, 4096, 8192, 8194};
    long plans = 0;
    for (int nr : NR)
        for (int nphi : NPHI)
            for (int eos = 0; eos < 3; ++eos) // isothermal; ideal with lazy derived grids; ideal without
                for (int leapfrog = 0; leapfrog < 2; ++leapfrog)
                    for (int damping = 0; damping < DAMP_MODES; ++damping)
                        for (int stabilize = 0; stabilize < 3; ++stabilize)
                            for (int particles = 0; particles < 2; ++particles)
                                for (int cfl_rings = 0; cfl_rings < 2; ++cfl_rings)
                                    for (int fold = -1; fold < 2; ++fold)
                                        for (int bc_in_cfl = 0; bc_in_cfl < 3; ++bc_in_cfl)
                                            for (int gate = 0; gate < 2; ++gate) {
                                                check(Case{nr, nphi, eos != 0, eos != 2, leapfrog, damping, stabilize, particles, cfl_rings, fold, bc_in_cfl, gate});
                                                ++plans;
                                            }
    check_headline(2048, 4096, 1, true, false); // no fold; the boundary call rides; the gated launch is not left to it
    check_headline(512, 1536, 2, false, true);  // fold; gated launch + boundary call are one launch; nothing rides
    std::printf("%ld plans, %d failures\n", plans, failures);
    return failures ? 1 : 0;
}
