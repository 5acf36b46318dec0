// Dust particles of the C ABI: device state, the launch of k_particles_step (kernels/particles.h), the switches of
// drag and diffusion and the blocking reads.  Replaces particles::integrate with ParticleIntegrator: midpoint (particles/particles.cpp:1525-1557,1579-1672)
// and ParticleIntegrator: explicit (:1677-2014, k_particles_step_explicit)
// -- either kernel one template, its host-argument or device-clock form and its slab form chosen by template arguments; one
// statement of the launch (fill_launch, enqueue_launch) for fcpt_particles_step and for fcpt_run_steps --
// for one radial slab, and -- fcpt_particles_slabs -- for a slab among several: ownership by window, and particles::move()'s
// hand-over to the radial neighbours (:2016-2161) as records in messages of the ghost rings' length; see
// include/fargocpt_hip.h for what is and is not covered.
#include "fcpt_ctx.h"

#include <algorithm>
#include <cfloat>

namespace fcpt {

void particles_free(fcpt_ctx *c)
{
    if (c->part_block)
        (void)hipFree(c->part_block);
    c->part_block = nullptr;
    c->part_id = nullptr;
    c->part = ParticleArgs{};
    if (c->part_adapt_block)
        (void)hipFree(c->part_adapt_block);
    c->part_adapt_block = nullptr;
    c->part_adapt = ParticleAdaptive{};
    c->part_adapt_set = false;
}

} // namespace fcpt

namespace {

const char *const kGuardNames[11] = {"",
                                     "Ma < 1e-20",
                                     "Ma > 1e20",
                                     "CdE < 1e-20",
                                     "CdE > 1e20",
                                     "CdS < 1e-30",
                                     "CdS > 1e30",
                                     "Cd < 1e-20",
                                     "Cd > 1e20",
                                     "the explicit integrator reached max_attempts substeps",
                                     "t_stop < 10 dt: the drag is too stiff for the explicit kick"};
const int kDefaultMaxAttempts = 10000;

// waits for the queued steps; reports (once) a guard tripped since the last call
int particles_wait(fcpt_ctx *c, const char *who)
{
    unsigned long long status = 0;
    HIPCHK(hipMemcpyAsync(&status, c->part.status, sizeof(status), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (!status)
        return FCPT_OK;
    HIPCHK(hipMemsetAsync(c->part.status, 0, sizeof(status), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int guard = (int)(status & 0xffull);
    const size_t slot = (size_t)(status >> 8);
    unsigned long long id = 0;
    if (slot < (size_t)c->part.n)
        HIPCHK(hipMemcpy(&id, c->part_id + slot, sizeof(id), hipMemcpyDeviceToHost));
    if (guard == 12)
        set_error("%s: guard 12: a migration message held a record count beyond the capacity or a slot index outside 0 .. %d; "
                  "nothing of it was written",
                  who, c->part.n - 1);
    else if (guard == 11)
        set_error("%s: particle id %llu tripped guard 11 (the step needs a gas row beyond the rings of slab %d on a side that "
                  "has a neighbour: it moved more than the overlap in one step, or its migration was deferred too long) and was "
                  "left unchanged",
                  who, id, c->d.rank);
    else if (guard >= 9 && guard <= 10)
        set_error("%s: particle id %llu tripped guard %d (%s) and was left unchanged", who, id, guard, kGuardNames[guard]);
    else
        set_error("%s: particle id %llu tripped guard %d of calc_tstop (%s) and was left unchanged", who, id, guard,
                  guard >= 1 && guard <= 8 ? kGuardNames[guard] : "?");
    return FCPT_EINVAL;
}

// the explicit integrator's block, made when first needed: four double arrays and two counters per slot, zeroed
int adaptive_alloc(fcpt_ctx *c)
{
    if (c->part_adapt_block)
        return FCPT_OK;
    const size_t nn = (size_t)c->part.n;
    const size_t bytes = nn * 8 * 4 + nn * 4 * 2;
    void *block = nullptr;
    if (hipMalloc(&block, bytes) != hipSuccess) {
        set_error("hipMalloc(%zu bytes) for the adaptive step sizes failed", bytes);
        return FCPT_ENOMEM;
    }
    if (hipMemsetAsync(block, 0, bytes, c->stream) != hipSuccess) {
        (void)hipFree(block);
        set_error("hipMemsetAsync of the adaptive step sizes failed");
        return FCPT_EHIP;
    }
    c->part_adapt_block = block;
    double *arr = (double *)block;
    ParticleAdaptive &X = c->part_adapt;
    X.timestep = arr;
    X.facold = arr + nn;
    X.r_ddot = arr + 2 * nn;
    X.phi_ddot = arr + 3 * nn;
    X.accepted = (unsigned int *)(arr + 4 * nn);
    X.rejected = X.accepted + nn;
    return FCPT_OK;
}

// the bodies of the last fcpt_set_bodies in polar coordinates (t_planet::get_r / get_phi)
void polar_bodies(const Dev &P, ParticleArgs &A)
{
    for (int k = 0; k < P.nbodies; ++k) {
        A.br[k] = std::sqrt(P.bx[k] * P.bx[k] + P.by[k] * P.by[k]);
        A.bphi[k] = std::atan2(P.by[k], P.bx[k]);
    }
}

// the Philox counter holds the id: two particles with one id would receive the same kicks
bool ids_distinct(const unsigned long long *id, size_t n)
{
    std::vector<unsigned long long> v(id, id + n);
    std::sort(v.begin(), v.end());
    return std::adjacent_find(v.begin(), v.end()) == v.end();
}

// ---- fcpt_particles_slabs -------------------------------------------------------------------------------------------
// the context takes particles as one of several slabs: the slab kernels, ownership and migration apply
bool on_slab(const fcpt_ctx *c)
{
    return c->part_slabs.on != 0 && c->d.nranks > 1;
}
size_t message_doubles(const fcpt_ctx *c)
{
    uint64_t cnt = 0;
    (void)fcpt_exchange_count(c, &cnt);
    return (size_t)cnt;
}
int record_doubles(const fcpt_ctx *c)
{
    return c->part_adapt_block ? PARTICLE_RECORD_MAX : PARTICLE_RECORD_MIN;
}
// records per side and call: the caller's, or what a message holds, whichever is smaller
int migrate_capacity(const fcpt_ctx *c)
{
    const int fit = (int)((message_doubles(c) - 1) / (size_t)record_doubles(c));
    const int asked = c->part_slabs.migrate_capacity;
    return asked > 0 && asked < fit ? asked : fit;
}
// squared edges of the ownership window; a side without a neighbour has none
void window_sq(const fcpt_ctx *c, double *lo_sq, double *hi_sq)
{
    *lo_sq = c->s.is_first ? -HUGE_VAL : c->part_window[0] * c->part_window[0];
    *hi_sq = c->s.is_last ? HUGE_VAL : c->part_window[1] * c->part_window[1];
}
void migrate_args(const fcpt_ctx *c, double *inner, double *outer, ParticleMigrate *M)
{
    window_sq(c, &M->lo_sq, &M->hi_sq);
    M->has_inner = !c->s.is_first;
    M->has_outer = !c->s.is_last;
    M->cartesian = c->part_integ.kind == 1 && c->part_integ.cartesian != 0;
    M->capacity = migrate_capacity(c);
    M->rec = record_doubles(c);
    M->inner = M->has_inner ? inner : nullptr;
    M->outer = M->has_outer ? outer : nullptr;
    M->cnt = c->part_mcnt;
    M->tot = c->part_mtot;
    M->chunk = M->groups = 0; // (launch_particles_emigrate's)
}
bool buffer_on_device(const void *p)
{
    if (!p)
        return true;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError(); // plain host memory: not an error here
        return false;
    }
    return a.type == hipMemoryTypeDevice;
}
// ---- the launch of a step ---------------------------------------------------------------------------------------------
// the per-step scalars fcpt_particles_step passes by value; fcpt_run_steps has none (the kernels read the device clock)
struct StepScalars {
    double dt, indirect_x, indirect_y, frame_angle;
    unsigned long long step;
};
// the explicit integrator may not step: no step sizes since the last fcpt_particles_set (each caller has its own text)
bool lacks_step_sizes(const fcpt_ctx *c)
{
    return c->part.n > 0 && c->part_integ.kind == 1 && !c->part_adapt_set;
}
// The launch of a step from the context as it is.  `host`: its scalars and indirect term (step_offset stays null); null: the
// device-sourced form of fcpt_run_steps -- dt, frame_angle and the counter stay zero and step_offset is set
// (kernels/particles.h: particle_dt and its neighbours), the indirect term is the one of the last fcpt_set_bodies.
// Zero-filled first and copied bytewise: fcpt_run_steps compares two of these with memcmp, padding included.
void fill_launch(const fcpt_ctx *c, const StepScalars *host, ParticleLaunch *L)
{
    std::memset((void *)L, 0, sizeof(*L));
    L->on = 1;
    L->explicit_adaptive = c->part_integ.kind == 1;
    L->cartesian = c->part_integ.cartesian != 0;
    L->adapt_set = c->part_adapt_set;
    ParticleArgs &A = L->A;
    std::memcpy((void *)&A, &c->part, sizeof(A));
    polar_bodies(c->P, A);
    A.dt = host ? host->dt : 0.0;
    A.frame_angle = host ? host->frame_angle : 0.0;
    A.step = host ? host->step : 0;
    A.indirect_x = host ? host->indirect_x : c->P.indirect_x;
    A.indirect_y = host ? host->indirect_y : c->P.indirect_y;
    A.gas_drag = c->part_diff.gas_drag;
    A.diffusion = c->part_diff.diffusion;
    A.id = c->part_id;
    A.seed = c->part_diff.seed;
    A.step_offset = host ? nullptr : c->part_step_offset;
    if (L->explicit_adaptive) {
        std::memcpy((void *)&L->X, &c->part_adapt, sizeof(L->X));
        L->X.max_attempts = c->part_integ.max_attempts > 0 ? c->part_integ.max_attempts : kDefaultMaxAttempts;
        L->X.rmin = c->d.rmin;
        L->X.rmax = c->d.rmax;
    }
}
// one launch on the context's stream: the explicit or the midpoint kernel, in the slab form where the context is a slab
void enqueue_launch(fcpt_ctx *c, const ParticleLaunch &L)
{
    if (L.explicit_adaptive)
        launch_particles_explicit(c->P, L.A, L.X, L.cartesian != 0, c->stream, on_slab(c));
    else
        launch_particles(c->P, L.A, c->stream, on_slab(c));
}

// ---- the blocking reads: live slots only, in ascending slot order -----------------------------------------------------
// The alive bytes of every slot on the host and their count in *m (also when refusing); refuses the caller whose arrays
// have room for fewer.  on_stream: read behind what the context's stream holds and wait for it; otherwise a blocking copy.
int live_slots(fcpt_ctx *c, const char *who, int64_t capacity, bool on_stream, std::vector<unsigned char> &alive, int64_t *m)
{
    alive.resize((size_t)c->part.n);
    if (on_stream) {
        HIPCHK(hipMemcpyAsync(alive.data(), c->part.alive, alive.size(), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    } else {
        HIPCHK(hipMemcpy(alive.data(), c->part.alive, alive.size(), hipMemcpyDeviceToHost));
    }
    *m = 0;
    for (unsigned char a : alive)
        *m += a != 0;
    if (*m > capacity) {
        set_error("%s: %lld live particles, room for %lld", who, (long long)*m, (long long)capacity);
        return FCPT_EINVAL;
    }
    return FCPT_OK;
}
// compaction on download: out[k] = in[slot] over the live slots (null out: that array was not asked for)
template <class T, class U> void compact(const std::vector<unsigned char> &alive, const T *in, U *out)
{
    if (!out)
        return;
    size_t k = 0;
    for (size_t s = 0; s < alive.size(); ++s)
        if (alive[s])
            out[k++] = in[s];
}

int migrate_check(const fcpt_ctx *c, const char *who)
{
    if (!c) {
        set_error("%s: null context", who);
        return FCPT_EINVAL;
    }
    if (!on_slab(c)) {
        set_error("%s needs fcpt_particles_slabs with on = 1 on a context that is one of several slabs", who);
        return FCPT_EINVAL;
    }
    return FCPT_OK;
}
// k_particles_emigrate into `inner` / `outer` (device, or host: through the context's own messages)
int migrate_pack(fcpt_ctx *c, double *send_inner, double *send_outer)
{
    if (c->part.n <= 0) { // nobody to send: empty messages
        const double zero = 0.0;
        for (double *m : {send_inner, send_outer})
            if (m)
                HIPCHK(hipMemcpyAsync(m, &zero, sizeof(zero), hipMemcpyDefault, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream)); // `zero` leaves scope
        return FCPT_OK;
    }
    join_side(c);
    const bool dev_in = buffer_on_device(send_inner), dev_out = buffer_on_device(send_outer);
    ParticleMigrate M;
    migrate_args(c, !send_inner ? nullptr : (dev_in ? send_inner : c->part_mbuf[0]),
                 !send_outer ? nullptr : (dev_out ? send_outer : c->part_mbuf[1]), &M);
    launch_particles_emigrate(c->part, c->part_adapt, M, c->stream);
    HIPCHK(hipGetLastError());
    const size_t bytes = message_doubles(c) * sizeof(double);
    if (M.inner && !dev_in)
        HIPCHK(hipMemcpyAsync(send_inner, c->part_mbuf[0], bytes, hipMemcpyDeviceToHost, c->stream));
    if (M.outer && !dev_out)
        HIPCHK(hipMemcpyAsync(send_outer, c->part_mbuf[1], bytes, hipMemcpyDeviceToHost, c->stream));
    if ((M.inner && !dev_in) || (M.outer && !dev_out))
        HIPCHK(hipStreamSynchronize(c->stream)); // the host buffers are complete when the call returns
    return FCPT_OK;
}
int migrate_unpack(fcpt_ctx *c, const double *recv_inner, const double *recv_outer)
{
    if (c->part.n <= 0)
        return FCPT_OK;
    join_side(c);
    const bool dev_in = buffer_on_device(recv_inner), dev_out = buffer_on_device(recv_outer);
    const size_t bytes = message_doubles(c) * sizeof(double);
    if (recv_inner && !dev_in)
        HIPCHK(hipMemcpyAsync(c->part_mbuf[2], recv_inner, bytes, hipMemcpyHostToDevice, c->stream));
    if (recv_outer && !dev_out)
        HIPCHK(hipMemcpyAsync(c->part_mbuf[3], recv_outer, bytes, hipMemcpyHostToDevice, c->stream));
    ParticleMigrate M;
    migrate_args(c, !recv_inner ? nullptr : (dev_in ? const_cast<double *>(recv_inner) : c->part_mbuf[2]),
                 !recv_outer ? nullptr : (dev_out ? const_cast<double *>(recv_outer) : c->part_mbuf[3]), &M);
    launch_particles_immigrate(c->part, c->part_adapt, M, c->stream);
    HIPCHK(hipGetLastError());
    if ((recv_inner && !dev_in) || (recv_outer && !dev_out))
        HIPCHK(hipStreamSynchronize(c->stream)); // the caller's host buffers are free again
    return FCPT_OK;
}
// pack, the neighbour exchange of the ghost rings' communicator with the messages in its place, unpack: one stream.
// `count`: the doubles that travel per message, word 0 and the records the capacity allows at the least
int migrate_collective(fcpt_ctx *c, size_t count)
{
    double *s_in = c->peer_inner >= 0 ? c->part_mbuf[0] : nullptr, *s_out = c->peer_outer >= 0 ? c->part_mbuf[1] : nullptr;
    double *r_in = c->peer_inner >= 0 ? c->part_mbuf[2] : nullptr, *r_out = c->peer_outer >= 0 ? c->part_mbuf[3] : nullptr;
    if (c->part.n <= 0) { // the neighbours still wait for this slab's messages: empty ones
        for (double *m : {s_in, s_out})
            if (m)
                HIPCHK(hipMemsetAsync(m, 0, sizeof(double), c->stream));
    } else if (int rc = migrate_pack(c, s_in, s_out)) {
        return rc;
    }
    const int rc = comm_neighbour_exchange(c->comm, c->peer_inner, s_in, r_in, c->peer_outer, s_out, r_out, count, c->stream);
    if (rc)
        return rc == FCPT_EHIP ? FCPT_ECOMM : rc;
    return migrate_unpack(c, r_in, r_out);
}

} // namespace

namespace fcpt {

// what fcpt_run_steps refuses with follow on, before anything is queued
int particles_loop_check(const fcpt_ctx *c)
{
    if (!c->part_follow)
        return FCPT_OK;
    if (c->d.nranks > 1 && (!c->comm || !c->part_slabs.on)) {
        set_error("fcpt_run_steps: fcpt_particles_follow_run_steps is on, and particles inside the multi-slab loop need %s%s%s "
                  "(this context is slab %d of %d)",
                  c->comm ? "" : "a communicator (fcpt_comm_init or fcpt_comm_init_host)",
                  !c->comm && !c->part_slabs.on ? " and " : "", c->part_slabs.on ? "" : "fcpt_particles_slabs with on = 1",
                  c->d.rank, c->d.nranks);
        return FCPT_EINVAL;
    }
    if (c->d.integrator == FCPT_INTEGRATOR_LEAPFROG) {
        set_error("fcpt_run_steps: fcpt_particles_follow_run_steps is on, and the particle step has no place in Integrator: "
                  "Leapfrog (switch it off, or use Integrator: Euler)");
        return FCPT_EINVAL;
    }
    if (lacks_step_sizes(c)) {
        set_error("fcpt_run_steps: fcpt_particles_follow_run_steps is on, and the explicit integrator has no step sizes since "
                  "the last fcpt_particles_set: call fcpt_particles_timestep_init or fcpt_particles_adaptive_set first");
        return FCPT_EINVAL;
    }
    return FCPT_OK;
}

// The launch fcpt_particles_step would make from the context as it is, in its device-sourced form (fill_launch); all zero
// where follow is off or there are no particles
void particles_loop_launch(const fcpt_ctx *c, ParticleLaunch *L)
{
    if (c->part_follow && c->part.n > 0)
        fill_launch(c, nullptr, L);
    else
        std::memset((void *)L, 0, sizeof(*L));
}

// the particle step of one iteration of fcpt_run_steps' device loop, behind the launch that left the step length in the clock
// (one of several slabs: the clock-reading slab kernels)
void enqueue_particles_loop(fcpt_ctx *c)
{
    ParticleLaunch L;
    particles_loop_launch(c, &L);
    if (!L.on)
        return;
    join_side(c);
    enqueue_launch(c, L);
}

// fcpt_run_steps on several slabs hands the step's leavers over with this (follow on, fcpt_particles_slabs on, a
// communicator: particles_loop_check); also with no particles at all, so that every slab makes the same calls
bool particles_loop_migrates(const fcpt_ctx *c)
{
    return c->part_follow && on_slab(c) && c->comm;
}

// The migration of one iteration of the multi-slab device loop, on the context's stream: fcpt_particles_migrate with
// messages cut to what the capacity in force can fill, 1 + capacity * R doubles (equal on all slabs: migrate_capacity and
// the record length are)
int enqueue_particles_migrate(fcpt_ctx *c)
{
    return migrate_collective(c, 1 + (size_t)migrate_capacity(c) * (size_t)record_doubles(c));
}

} // namespace fcpt

extern "C" {

int fcpt_particles_follow_run_steps(fcpt_ctx *c, int32_t on)
{
    if (!c || (on != 0 && on != 1)) {
        set_error("fcpt_particles_follow_run_steps: null context, or on = %d is neither 0 nor 1", (int)on);
        return FCPT_EINVAL;
    }
    if (on && !c->part_step_offset)
        if (int rc = dev_alloc(c, &c->part_step_offset, 1))
            return rc;
    c->part_follow = on != 0;
    return FCPT_OK;
}

int fcpt_particles_follow_run_steps_get(const fcpt_ctx *c, int32_t *on)
{
    if (!c || !on)
        return FCPT_EINVAL;
    *on = c->part_follow ? 1 : 0;
    return FCPT_OK;
}

int fcpt_particles_set(fcpt_ctx *c, const fcpt_particle_params *prm, int64_t n, const uint64_t *id, const double *r,
                       const double *phi, const double *r_dot, const double *phi_dot, const double *radius,
                       const double *stokes)
{
    if (!c || n < 0 || n > 0x7fffffff) {
        set_error("fcpt_particles_set: null context or n outside 0 .. 2^31-1");
        return FCPT_EINVAL;
    }
    if (n > 0 && (!prm || !id || !r || !phi || !r_dot || !phi_dot || !radius || !stokes)) {
        set_error("fcpt_particles_set: null argument");
        return FCPT_EINVAL;
    }
    if (n > 0 && c->d.nranks != 1 && !c->part_slabs.on) {
        set_error("fcpt_particles_set: particles need the whole grid in one slab (this context is slab %d of %d)", c->d.rank,
                  c->d.nranks);
        return FCPT_EINVAL;
    }
    if (n > 0 && (!(prm->escape_radius_min >= c->d.rmin) || !(prm->escape_radius_max <= c->d.rmax) ||
                  !(prm->escape_radius_min < prm->escape_radius_max))) {
        set_error("fcpt_particles_set: escape radii [%g, %g] must be ordered and inside the grid [%g, %g]", prm->escape_radius_min,
                  prm->escape_radius_max, c->d.rmin, c->d.rmax);
        return FCPT_EINVAL;
    }
    if (n > 0 && c->part_diff.diffusion && !ids_distinct((const unsigned long long *)id, (size_t)n)) {
        set_error("fcpt_particles_set: particle ids must be distinct while dust diffusion is on (the id is the random counter)");
        return FCPT_EINVAL;
    }
    HIPCHK(hipStreamSynchronize(c->stream)); // a queued step may still use the arrays
    particles_free(c);
    if (n == 0)
        return FCPT_OK;
    // one block: status word, ids, six double arrays, alive bytes
    const size_t nn = (size_t)n;
    const size_t bytes = 8 + nn * 8 * 7 + nn;
    void *block = nullptr;
    if (hipMalloc(&block, bytes) != hipSuccess) {
        set_error("hipMalloc(%zu bytes) for the particles failed", bytes);
        return FCPT_ENOMEM;
    }
    c->part_block = block;
    char *p = (char *)block;
    ParticleArgs &A = c->part;
    A.status = (unsigned long long *)p;
    c->part_id = (unsigned long long *)(p + 8);
    double *arr = (double *)(p + 8 + nn * 8);
    A.r = arr;
    A.phi = arr + nn;
    A.r_dot = arr + 2 * nn;
    A.phi_dot = arr + 3 * nn;
    A.stokes = arr + 4 * nn;
    A.radius = arr + 5 * nn;
    A.alive = (unsigned char *)(arr + 6 * nn);
    const double *src[6] = {r, phi, r_dot, phi_dot, stokes, radius};
    int rc = FCPT_OK;
    auto chk = [&](hipError_t e) {
        if (e != hipSuccess && rc == FCPT_OK) {
            set_error("fcpt_particles_set: copy to the device failed: %s", hipGetErrorString(e));
            rc = FCPT_EHIP;
        }
    };
    chk(hipMemsetAsync(A.status, 0, 8, c->stream));
    chk(hipMemcpyAsync(c->part_id, id, nn * 8, hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < 6; ++k)
        chk(hipMemcpyAsync(arr + k * nn, src[k], nn * 8, hipMemcpyHostToDevice, c->stream));
    std::vector<unsigned char> owned; // (outlives the copy)
    if (on_slab(c)) {
        // every slab is handed the full list and owns what starts inside its window: r_lo^2 <= d^2 < r_hi^2
        double lo_sq, hi_sq;
        window_sq(c, &lo_sq, &hi_sq);
        const bool cart = c->part_integ.kind == 1 && c->part_integ.cartesian != 0;
        owned.resize(nn);
        for (size_t k = 0; k < nn; ++k) {
            const double d2 = cart ? r[k] * r[k] + phi[k] * phi[k] : r[k] * r[k];
            owned[k] = lo_sq <= d2 && d2 < hi_sq;
        }
        chk(hipMemcpyAsync(A.alive, owned.data(), nn, hipMemcpyHostToDevice, c->stream));
    } else {
        chk(hipMemsetAsync(A.alive, 1, nn, c->stream));
    }
    chk(hipStreamSynchronize(c->stream));
    if (rc) {
        particles_free(c);
        return rc;
    }
    A.n = (int)n;
    A.particle_density = prm->particle_density;
    A.molecule_mass = prm->molecule_mass;
    A.molecule_radius = prm->molecule_radius;
    A.k_B = prm->k_B;
    // parameters.cpp:957-961
    A.escape_max_sq = prm->escape_radius_max * prm->escape_radius_max - DBL_EPSILON;
    A.escape_min_sq = prm->escape_radius_min * prm->escape_radius_min + DBL_EPSILON;
    A.gravity_cartesian = prm->gravity_cartesian != 0;
    A.spacing = c->d.radial_spacing;
    A.cf_rmin = c->d.rmin;
    A.cf_growth = c->geo.cf_growth;
    A.cf_inv_log_growth = c->geo.cf_inv_log_growth;
    A.cf_opt_const = c->geo.cf_opt_const;
    A.row0 = on_slab(c) ? c->s.imin : 0;
    return FCPT_OK;
}

int fcpt_particles_step(fcpt_ctx *c, double dt, double indirect_x, double indirect_y, double frame_angle)
{
    if (!c)
        return FCPT_EINVAL;
    const unsigned long long step = c->part_diff.step++;
    if (c->part.n <= 0)
        return FCPT_OK;
    if (lacks_step_sizes(c)) {
        set_error("fcpt_particles_step: the explicit integrator has no step sizes since the last fcpt_particles_set: call "
                  "fcpt_particles_timestep_init or fcpt_particles_adaptive_set first");
        return FCPT_EINVAL;
    }
    join_side(c);
    ProfScope prof_scope(c);
    const StepScalars host = {dt, indirect_x, indirect_y, frame_angle, step};
    ParticleLaunch L;
    fill_launch(c, &host, &L);
    enqueue_launch(c, L);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_particles_count(fcpt_ctx *c, int64_t *n_alive)
{
    if (!c || !n_alive)
        return FCPT_EINVAL;
    *n_alive = 0;
    if (c->part.n <= 0)
        return FCPT_OK;
    if (int rc = particles_wait(c, "fcpt_particles_count"))
        return rc;
    std::vector<unsigned char> alive;
    return live_slots(c, "fcpt_particles_count", INT64_MAX, false, alive, n_alive);
}

int fcpt_particles_get(fcpt_ctx *c, int64_t capacity, uint64_t *id, double *r, double *phi, double *r_dot, double *phi_dot,
                       double *radius, double *stokes, int64_t *n)
{
    if (!c || !n || capacity < 0)
        return FCPT_EINVAL;
    *n = 0;
    if (c->part.n <= 0)
        return FCPT_OK;
    if (int rc = particles_wait(c, "fcpt_particles_get"))
        return rc;
    const size_t nn = (size_t)c->part.n;
    std::vector<unsigned char> alive;
    std::vector<double> host(6 * nn);
    std::vector<unsigned long long> ids(id ? nn : 0);
    if (id)
        HIPCHK(hipMemcpy(ids.data(), c->part_id, nn * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(host.data(), c->part.r, 6 * nn * sizeof(double), hipMemcpyDeviceToHost)); // r is the first of six arrays
    if (int rc = live_slots(c, "fcpt_particles_get", capacity, false, alive, n))
        return rc;
    double *out[6] = {r, phi, r_dot, phi_dot, stokes, radius}; // the order of the device block
    compact(alive, ids.data(), id);
    for (int q = 0; q < 6; ++q)
        compact(alive, host.data() + q * nn, out[q]);
    return FCPT_OK;
}

int fcpt_particles_diffusion(fcpt_ctx *c, const fcpt_particle_diffusion *p)
{
    if (!c || !p) {
        set_error("fcpt_particles_diffusion: null argument");
        return FCPT_EINVAL;
    }
    if ((p->gas_drag != 0 && p->gas_drag != 1) || (p->diffusion != 0 && p->diffusion != 1)) {
        set_error("fcpt_particles_diffusion: gas_drag = %d and diffusion = %d must be 0 or 1", p->gas_drag, p->diffusion);
        return FCPT_EINVAL;
    }
    if (p->diffusion && c->part_integ.kind == 1) {
        set_error("fcpt_particles_diffusion: dust diffusion is not available with the explicit adaptive integrator "
                  "(fcpt_particles_integrator kind = 1)");
        return FCPT_EINVAL;
    }
    if (p->diffusion && c->part.n > 0) {
        std::vector<unsigned long long> ids((size_t)c->part.n);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(ids.data(), c->part_id, ids.size() * 8, hipMemcpyDeviceToHost));
        if (!ids_distinct(ids.data(), ids.size())) {
            set_error("fcpt_particles_diffusion: particle ids must be distinct while dust diffusion is on (the id is the random counter)");
            return FCPT_EINVAL;
        }
    }
    c->part_diff = *p;
    return FCPT_OK;
}

int fcpt_particles_diffusion_get(fcpt_ctx *c, fcpt_particle_diffusion *out)
{
    if (!c || !out)
        return FCPT_EINVAL;
    *out = c->part_diff;
    return FCPT_OK;
}

int fcpt_particles_integrator(fcpt_ctx *c, const fcpt_particle_integrator *p)
{
    if (!c || !p) {
        set_error("fcpt_particles_integrator: null argument");
        return FCPT_EINVAL;
    }
    if ((p->kind != 0 && p->kind != 1) || (p->cartesian != 0 && p->cartesian != 1)) {
        set_error("fcpt_particles_integrator: kind = %d and cartesian = %d must be 0 or 1", p->kind, p->cartesian);
        return FCPT_EINVAL;
    }
    if (p->max_attempts < 0) {
        set_error("fcpt_particles_integrator: max_attempts = %d must not be negative (0 selects %d)", p->max_attempts,
                  kDefaultMaxAttempts);
        return FCPT_EINVAL;
    }
    if (p->cartesian && p->kind == 0) {
        set_error("fcpt_particles_integrator: cartesian = 1 needs the explicit adaptive integrator (kind = 1); the midpoint "
                  "integrator's Cartesian gravity is fcpt_particle_params.gravity_cartesian");
        return FCPT_EINVAL;
    }
    if (p->kind == 1 && c->part_diff.diffusion) {
        set_error("fcpt_particles_integrator: the explicit adaptive integrator is not available with dust diffusion "
                  "(fcpt_particles_diffusion diffusion = 1)");
        return FCPT_EINVAL;
    }
    c->part_integ = *p;
    c->part_integ._pad0 = 0;
    return FCPT_OK;
}

int fcpt_particles_integrator_get(fcpt_ctx *c, fcpt_particle_integrator *out)
{
    if (!c || !out)
        return FCPT_EINVAL;
    *out = c->part_integ;
    return FCPT_OK;
}

int fcpt_particles_timestep_init(fcpt_ctx *c)
{
    if (!c)
        return FCPT_EINVAL;
    if (c->part_integ.kind != 1) {
        set_error("fcpt_particles_timestep_init: select the explicit adaptive integrator first (fcpt_particles_integrator kind = 1)");
        return FCPT_EINVAL;
    }
    if (c->part.n <= 0)
        return FCPT_OK;
    if (int rc = adaptive_alloc(c))
        return rc;
    join_side(c);
    ParticleArgs A = c->part;
    polar_bodies(c->P, A);
    launch_particles_timestep_init(c->P, A, c->part_adapt, c->part_integ.cartesian != 0, c->stream);
    HIPCHK(hipGetLastError());
    c->part_adapt_set = true;
    return FCPT_OK;
}

int fcpt_particles_adaptive_set(fcpt_ctx *c, int64_t n, const double *timestep, const double *facold)
{
    if (!c || !timestep || !facold) {
        set_error("fcpt_particles_adaptive_set: null argument");
        return FCPT_EINVAL;
    }
    if (n != (int64_t)c->part.n || n <= 0) {
        set_error("fcpt_particles_adaptive_set: n = %lld, the context holds %d particle slots", (long long)n, c->part.n);
        return FCPT_EINVAL;
    }
    if (int rc = adaptive_alloc(c))
        return rc;
    const size_t nn = (size_t)n;
    HIPCHK(hipMemcpyAsync(c->part_adapt.timestep, timestep, nn * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->part_adapt.facold, facold, nn * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream)); // the caller's arrays are free again
    c->part_adapt_set = true;
    return FCPT_OK;
}

int fcpt_particles_adaptive_get(fcpt_ctx *c, int64_t capacity, double *timestep, double *facold, double *r_ddot, double *phi_ddot,
                                uint32_t *accepted, uint32_t *rejected, int64_t *n)
{
    if (!c || !n || capacity < 0)
        return FCPT_EINVAL;
    *n = 0;
    if (c->part.n <= 0)
        return FCPT_OK;
    if (!c->part_adapt_block) {
        set_error("fcpt_particles_adaptive_get: no adaptive state since the last fcpt_particles_set");
        return FCPT_EINVAL;
    }
    if (int rc = particles_wait(c, "fcpt_particles_adaptive_get"))
        return rc;
    const size_t nn = (size_t)c->part.n;
    std::vector<unsigned char> alive;
    std::vector<double> host(4 * nn);
    std::vector<unsigned int> counts(2 * nn);
    HIPCHK(hipMemcpy(host.data(), c->part_adapt.timestep, 4 * nn * sizeof(double), hipMemcpyDeviceToHost)); // the first of four arrays
    HIPCHK(hipMemcpy(counts.data(), c->part_adapt.accepted, 2 * nn * sizeof(unsigned int), hipMemcpyDeviceToHost));
    if (int rc = live_slots(c, "fcpt_particles_adaptive_get", capacity, false, alive, n))
        return rc;
    double *out[4] = {timestep, facold, r_ddot, phi_ddot};
    uint32_t *cnt[2] = {accepted, rejected};
    for (int q = 0; q < 4; ++q)
        compact(alive, host.data() + q * nn, out[q]);
    for (int q = 0; q < 2; ++q)
        compact(alive, counts.data() + q * nn, cnt[q]);
    return FCPT_OK;
}

int fcpt_particles_normals(fcpt_ctx *c, uint64_t step, int64_t capacity, double *snv)
{
    if (!c || capacity < 0 || (capacity > 0 && !snv))
        return FCPT_EINVAL;
    if (c->part.n <= 0)
        return FCPT_OK;
    const size_t nn = (size_t)c->part.n;
    double *d_snv = nullptr;
    if (hipMalloc((void **)&d_snv, nn * sizeof(double)) != hipSuccess) {
        set_error("hipMalloc(%zu bytes) for the deviates failed", nn * sizeof(double));
        return FCPT_ENOMEM;
    }
    launch_particles_normals(c->part.n, c->part_id, c->part_diff.seed, step, d_snv, c->stream);
    std::vector<double> host(nn);
    std::vector<unsigned char> alive;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess)
        e = hipMemcpyAsync(host.data(), d_snv, nn * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    int64_t m = 0;
    // (alive is read on the stream, behind the kernel and the copy, and the wait covers all three)
    const int rc = e == hipSuccess ? live_slots(c, "fcpt_particles_normals", capacity, true, alive, &m) : FCPT_OK;
    (void)hipFree(d_snv);
    HIPCHK(e);
    if (rc)
        return rc;
    compact(alive, host.data(), snv);
    return FCPT_OK;
}

// ---- particles on several slabs: the setting, the messages, the collective -----------------------------------------------

int fcpt_particles_slabs(fcpt_ctx *c, const fcpt_particle_slabs *p)
{
    if (!c || !p) {
        set_error("fcpt_particles_slabs: null argument");
        return FCPT_EINVAL;
    }
    if (p->on != 0 && p->on != 1) {
        set_error("fcpt_particles_slabs: on = %d is neither 0 nor 1", (int)p->on);
        return FCPT_EINVAL;
    }
    const int fit = (int)((message_doubles(c) - 1) / (size_t)PARTICLE_RECORD_MIN);
    if (p->migrate_capacity < 0 || p->migrate_capacity > fit) {
        set_error("fcpt_particles_slabs: migrate_capacity = %d outside 0 .. %d, what a message of %zu doubles holds (0 selects "
                  "the built-in value)",
                  (int)p->migrate_capacity, fit, message_doubles(c));
        return FCPT_EINVAL;
    }
    if (c->part.n > 0 && (p->on != 0) != (c->part_slabs.on != 0) && c->d.nranks > 1) {
        set_error("fcpt_particles_slabs: switch it before fcpt_particles_set (the context holds %d particle slots)", c->part.n);
        return FCPT_EINVAL;
    }
    if (p->on && !c->part_mtot) {
        if (int rc = fcpt_particles_slab_window(&c->d, c->radii.data(), c->part_window))
            return rc;
        for (int k = 0; k < 4; ++k)
            if (int rc = dev_alloc(c, &c->part_mbuf[k], message_doubles(c)))
                return rc;
        if (int rc = dev_alloc(c, &c->part_mcnt, 2 * (PARTICLE_MIGRATE_GROUPS + 1)))
            return rc;
        if (int rc = dev_alloc(c, &c->part_mtot, 4))
            return rc;
    }
    c->part_slabs.on = p->on;
    c->part_slabs.migrate_capacity = p->migrate_capacity;
    return FCPT_OK;
}

int fcpt_particles_slabs_get(fcpt_ctx *c, fcpt_particle_slabs *out)
{
    if (!c || !out)
        return FCPT_EINVAL;
    *out = c->part_slabs;
    if (c->part_mtot) {
        unsigned long long tot[4];
        HIPCHK(hipMemcpyAsync(tot, c->part_mtot, sizeof(tot), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        out->sent_inner = tot[0];
        out->sent_outer = tot[1];
        out->received = tot[2];
        out->deferred = tot[3];
    }
    return FCPT_OK;
}

int fcpt_particles_migrate_count(fcpt_ctx *c, uint64_t *count)
{
    return fcpt_exchange_count(c, count);
}

int fcpt_particles_migrate_pack(fcpt_ctx *c, double *send_inner, double *send_outer)
{
    if (int rc = migrate_check(c, "fcpt_particles_migrate_pack"))
        return rc;
    ProfScope prof_scope(c);
    return migrate_pack(c, send_inner, send_outer);
}

int fcpt_particles_migrate_unpack(fcpt_ctx *c, const double *recv_inner, const double *recv_outer)
{
    if (int rc = migrate_check(c, "fcpt_particles_migrate_unpack"))
        return rc;
    ProfScope prof_scope(c);
    return migrate_unpack(c, recv_inner, recv_outer);
}

// the collective with messages of the documented full length, fcpt_particles_migrate_count
int fcpt_particles_migrate(fcpt_ctx *c)
{
    if (int rc = migrate_check(c, "fcpt_particles_migrate"))
        return rc;
    if (!c->comm) {
        set_error("fcpt_particles_migrate needs fcpt_comm_init or fcpt_comm_init_host");
        return FCPT_EINVAL;
    }
    ProfScope prof_scope(c);
    return migrate_collective(c, message_doubles(c));
}

} // extern "C"
