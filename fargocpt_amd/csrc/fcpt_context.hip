// Context management: creation and destruction, options, host <-> device transfers, bodies, initial physics and the
// per-kernel profiler of the C ABI (include/fargocpt_hip.h).
#include "fcpt_ctx.h"

using namespace fcpt;

namespace fcpt {

void drop_graph(fcpt_ctx *c)
{
    if (c->graph_exec)
        (void)hipGraphExecDestroy(c->graph_exec);
    if (c->graph)
        (void)hipGraphDestroy(c->graph);
    c->graph_exec = nullptr;
    c->graph = nullptr;
    c->graph_cycle = 0;
}

// the caller's stream waits for the interior transport forked by fcpt_step_device_begin
void join_side(fcpt_ctx *c)
{
    if (c->ls.join_pending) {
        (void)hipStreamWaitEvent(c->stream, c->e_join, 0);
        c->ls.join_pending = false;
    }
}

int read_clock(fcpt_ctx *c, DevClock *out)
{
    join_side(c);
    HIPCHK(hipMemcpyAsync(c->h_clk, c->P.clk, sizeof(DevClock), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *out = *c->h_clk;
    if (out->shear_error) {
        set_error("a step exceeded the FARGO shear limit (|Nshift[i]-Nshift[i-1]| > 1) with the option "
                  "transport_fallback = 0, i.e. without the two-kernel transport queued behind the fused one; "
                  "the state is invalid");
        return FCPT_ESHEAR;
    }
    return FCPT_OK;
}

} // namespace fcpt

namespace {

int *option_slot(Options &o, const char *name)
{
#define X(n)                     \
    if (!std::strcmp(name, #n)) \
        return &o.n;
    FCPT_OPTION_NAMES
#undef X
    return nullptr;
}

// defaults of the switches: FCPT_<NAME> in the environment, read here and nowhere else
void options_from_environment(Options &o)
{
    o.transport_fused = o.transport_rows = o.source_rows = o.theta_rows = -1;
    o.transport_graded = 1;
    o.source_graded = -1;
    o.transport_big = o.transport_ladder = o.transport_rank_grade = -1;
    o.transport_fallback = o.transport_split = o.march_source = o.march_source_adi = 1;
    o.theta_march = o.cfl_rings = o.cfl_split = o.source_ring_parts = o.fused_damping = 1;
    o.cfl_wide_blocks = -1;
    o.gate_in_boundary = 1;
    o.cfl_fold_in_source = -1;
    o.inline_potential = 1;
    o.bc_fold = 1;
    o.bc_in_cfl = 1;
    o.comm_overlap = 0;
    o.comm_loopback = 0;
    o.graph_steps = -1;
    o.profile_stride = 1;
#define X(n)                                                           \
    {                                                                  \
        char env[64] = "FCPT_";                                        \
        size_t k = 5;                                                  \
        for (const char *q = #n; *q && k + 1 < sizeof(env); ++q)       \
            env[k++] = (char)((*q >= 'a' && *q <= 'z') ? *q - 32 : *q); \
        env[k] = 0;                                                    \
        if (const char *e = getenv(env))                               \
            if (e[0])                                                  \
                o.n = atoi(e);                                         \
    }
    FCPT_OPTION_NAMES
#undef X
}

int dev_upload(fcpt_ctx *c, const double **dst, const std::vector<double> &src)
{
    double *p = nullptr;
    if (int rc = dev_alloc(c, &p, src.size()))
        return rc;
    hipError_t e = hipMemcpy(p, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("hipMemcpy H2D failed: %s", hipGetErrorString(e));
        return FCPT_EHIP;
    }
    *dst = p;
    return FCPT_OK;
}

// the context's derived switches after its options changed (fcpt_create, fcpt_set_option)
void apply_options(fcpt_ctx *c, bool at_create = true)
{
    const Options &o = c->P.opt;
    c->ls.march_source = o.march_source != 0;
    const bool adi_march = c->P.adiabatic && c->ls.march_source && c->P.nphi >= 128 && o.march_source_adi != 0;
    c->P.lazy_derived = adi_march ? 1 : 0;
    c->P.inline_potential = (adi_march && !c->P.leapfrog && o.inline_potential != 0 && !c->P.accel_force) ? 1 : 0;
    c->P.damp_in_step = (c->damp_foldable && o.fused_damping != 0) ? 1 : 0;
    c->ls.cfl_interior = false;
    c->ls.potential_valid = false;
    c->ls.pressure_valid = false;
    // the wavefront table of the marching source kernels (the caller has synchronised the stream, or nothing has run yet)
    c->P.sm_sched = nullptr;
    c->P.sm_sched_n = 0;
    c->sm_sched_host.clear();
    if (c->sm_sched_dev && c->ls.march_source) {
        // (an explicit list, fcpt_set_source_chunks, stands in for the built-in table whatever source_graded says;
        //  source_rows > 0 selects equal chunks over either)
        const std::vector<int> sched = c->sm_lengths.empty() ? source_schedule(c->P, device_cus())
                                       : o.source_rows > 0   ? std::vector<int>()
                                                             : source_schedule_explicit(c->P, c->sm_lengths, nullptr);
        if (!sched.empty() && sched.size() <= c->sm_sched_cap &&
            hipMemcpy(c->sm_sched_dev, sched.data(), sched.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess) {
            c->P.sm_sched = c->sm_sched_dev;
            c->P.sm_sched_n = (int)(sched.size() / 4);
            c->sm_sched_host = sched;
        }
    }
    // the chunk table of the fused transport
    c->P.tf_sched = nullptr;
    c->P.tf_sched_n = 0;
    if (c->tf_sched_dev) {
        std::vector<int> slow(c->P.nr, 0);
        if (c->P.damp_in_step)
            slow = c->ring_ref_damped;
        const std::vector<int> sched = transport_schedule(c->P, device_cus(), slow, &c->tf_lengths);
        c->tf_sched_host.clear();
        if (!sched.empty() && sched.size() <= c->tf_sched_cap &&
            hipMemcpy(c->tf_sched_dev, sched.data(), sched.size() * sizeof(int), hipMemcpyHostToDevice) == hipSuccess) {
            c->P.tf_sched = c->tf_sched_dev;
            c->P.tf_sched_n = (int)(sched.size() / 4);
            c->tf_sched_host = sched;
        }
    }
    if (!at_create)
        refresh_derived(c); // the kernels that read c_s, H, nu, T from the grids expect them current
}

int copy_initial_values(fcpt_ctx *c)
{
    const Dev &P = c->P;
    const size_t ns = (size_t)P.nr * P.nphi * sizeof(double), nv = (size_t)(P.nr + 1) * P.nphi * sizeof(double);
    HIPCHK(hipMemcpyAsync(P.vrad0, P.vrad, nv, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.vazi0, P.vazi, ns, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.sigma0, P.sigma, ns, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(P.energy0, P.energy, ns, hipMemcpyDeviceToDevice, c->stream));
    return FCPT_OK;
}

// ---- the device stages of fcpt_create (the host ones: fcpt_tables.cpp) ----

// the geometry and the tables of `t` in device memory, Dev's views of them, and what the context keeps of `t`
int upload_tables(fcpt_ctx *c, const RingTables &t)
{
    Dev &P = c->P;
    const HostGeometry &g = c->geo;
    const struct {
        const double **dst;
        const std::vector<double> &src;
    } arrays[] = {{&P.Rmed.p, g.Rmed}, {&P.Rinf.p, g.Rinf}, {&P.Rsup.p, g.Rsup}, {&P.Surf.p, g.Surf}, {&P.InvRmed.p, g.InvRmed},
                  {&P.InvRinf.p, g.InvRinf}, {&P.InvSurf.p, g.InvSurf}, {&P.InvDiffRmed.p, g.InvDiffRmed},
                  {&P.InvDiffRsup.p, g.InvDiffRsup}, {&P.InvDiffRsupRb.p, g.InvDiffRsupRb},
                  {&P.cosphi, t.cosphi}, {&P.sinphi, t.sinphi}, {&P.nu_ring.p, t.nu_ring},
                  {&P.g_dxtheta.p, t.g_dxtheta}, {&P.g_inv_dxtheta.p, t.g_inv_dxtheta}, {&P.g_dr_invsurf.p, t.g_dr_invsurf},
                  {&P.g_r_omega.p, t.g_r_omega}, {&P.g_inv_omk.p, t.g_inv_omk}, {&P.g_omk.p, t.g_omk}, {&P.g_ra3.p, t.g_ra3},
                  {&P.dfac_s.p, t.fs}, {&P.dtau_s.p, t.ts}, {&P.dfac_v.p, t.fv}, {&P.dtau_v.p, t.tv}};
    for (const auto &a : arrays)
        if (int rc = dev_upload(c, a.dst, a.src))
            return rc;
    if (int rc = dev_upload_raw(c, &c->d_cs_ring, t.cs_ring)) // k_iso_cs_h writes through this pointer, the others read
        return rc;
    P.cs_ring.p = c->d_cs_ring;
    CArrI *const dtype[4] = {&P.dtype_vr, &P.dtype_va, &P.dtype_sig, &P.dtype_e};
    for (int q = 0; q < 4; ++q)
        if (int rc = dev_upload_raw(c, &dtype[q]->p, t.dtype[q]))
            return rc;
    if (int rc = dev_upload_raw(c, &P.rad_tab, t.rad))
        return rc;
    if (int rc = dev_upload_raw(c, &P.theta_tab, t.theta))
        return rc;
    if (int rc = dev_upload_raw(c, &P.src_tab, t.src))
        return rc;
    if (int rc = dev_upload_raw(c, &P.damp_tab, t.damp_rows))
        return rc;
    if (int rc = dev_upload_raw(c, &P.tf_tab, t.tf))
        return rc;
    std::memcpy(c->damp, t.damp, sizeof(c->damp));
    c->ring_ref_damped = t.ring_ref_damped;
    c->damp_any = t.damp_any;
    c->damp_foldable = t.damp_foldable;
    return FCPT_OK;
}

// every grid and work array of the slab, zero-filled, and the field table of fcpt_upload / fcpt_download
int alloc_grids(fcpt_ctx *c)
{
    Dev &P = c->P;
    const fcpt_desc &d = c->d;
    const int nr = c->s.nr, nphi = d.nphi;
    const size_t ns = (size_t)nr * nphi, nv = (size_t)(nr + 1) * nphi;
    P.ring_pstride = nphi / 32 + 4;
    const struct {
        double **p;
        size_t n;
    } grids[] = {{&P.sigma, ns}, {&P.vrad, nv}, {&P.vazi, ns}, {&P.energy, ns}, {&P.vrad_b, nv}, {&P.vazi_b, ns}, {&P.energy_b, ns},
                 {&P.pressure, ns}, {&P.soundspeed, ns}, {&P.scale_height, ns}, {&P.viscosity, ns}, {&P.temperature, ns},
                 {&P.potential, ns},
                 {&P.sigma0, ns}, {&P.vrad0, nv}, {&P.vazi0, ns}, {&P.energy0, ns},
                 // (qr .. trp: read and written by no kernel; kept allocated, see Dev and profiles/ab_narrow_source.txt)
                 {&P.qr, ns}, {&P.qphi, ns}, {&P.divv, ns}, {&P.trr, ns}, {&P.tpp, ns}, {&P.trp, nv}, {&P.qplus, ns}, {&P.qminus, ns},
                 {&P.rmpA, ns}, {&P.rmmA, ns}, {&P.lpA, ns}, {&P.lmA, ns}, {&P.sigA, ns}, {&P.eA, ns},
                 {&P.rmpB, ns}, {&P.rmmB, ns}, {&P.lpB, ns}, {&P.lmB, ns}, {&P.sigB, ns}, {&P.eB, ns},
                 {&P.vmean, (size_t)nr + 1}, {&P.vconst, (size_t)nr},
                 {&P.cfl_part, (size_t)(nr + 256) * (size_t)((nphi + 255) / 256 + 1)}, {&P.ring_part, (size_t)nr * P.ring_pstride},
                 // null unless StabilizeViscosity / WriteMassFlow / BodyForceFromPotential: no / the ideal EOS
                 {&P.cfac_phi, d.stabilize_viscosity ? ns : 0}, {&P.cfac_r, d.stabilize_viscosity ? ns : 0},
                 {&P.massflow, d.write_massflow ? nv : 0},
                 // (zero-filled: rows 0 and nr are never written, Pframeforce.cpp:121-123)
                 {&P.accel_r, d.body_force_from_potential ? 0 : nv}, {&P.accel_az, d.body_force_from_potential ? 0 : nv},
                 {&P.qdiff, d.eos == FCPT_EOS_IDEAL ? ns : 0}};
    for (const auto &g : grids)
        if (g.n)
            if (int rc = dev_alloc(c, g.p, g.n))
                return rc;
    if (int rc = dev_alloc(c, &P.nshift, (size_t)nr))
        return rc;
    if (int rc = dev_alloc(c, &P.clk, 1))
        return rc;
    if (int rc = dev_alloc(c, &P.shift_jump, 8))
        return rc;
    if (int rc = dev_alloc(c, &P.shift_tab, (size_t)nr + TF_ROW_GUARD)) // (the guard rows in front of ring 0 stay zero)
        return rc;
    P.shift_tab += TF_ROW_GUARD;
    c->tf_sched_cap = (size_t)4 * 65536; // graded chunks: two to three rounds of a 512-CU device's wavefront slots, and the padding
    if (int rc = dev_alloc(c, &c->tf_sched_dev, c->tf_sched_cap))
        return rc;
    c->sm_sched_cap = (size_t)4 * (8 * 4 * 8 * 64 + 64); // one entry per wavefront slot of a 512-CU device at 8 per SIMD
    if (int rc = dev_alloc(c, &c->sm_sched_dev, c->sm_sched_cap))
        return rc;
    if (hipHostMalloc((void **)&c->h_clk, sizeof(DevClock)) != hipSuccess) {
        set_error("hipHostMalloc failed");
        return FCPT_ENOMEM;
    }
    P.vmean_c.p = P.vmean;
    P.vconst_c.p = P.vconst;
    P.nshift_c.p = P.nshift;
    c->grid[FCPT_F_SIGMA] = P.sigma;
    c->grid[FCPT_F_VRAD] = P.vrad;
    c->grid[FCPT_F_VAZI] = P.vazi;
    c->grid[FCPT_F_ENERGY] = P.energy;
    c->grid[FCPT_F_PRESSURE] = P.pressure;
    c->grid[FCPT_F_SOUNDSPEED] = P.soundspeed;
    c->grid[FCPT_F_SCALE_HEIGHT] = P.scale_height;
    c->grid[FCPT_F_VISCOSITY] = P.viscosity;
    c->grid[FCPT_F_TEMPERATURE] = P.temperature;
    c->grid[FCPT_F_POTENTIAL] = P.potential;
    c->grid[FCPT_F_SIGMA0] = P.sigma0;
    c->grid[FCPT_F_VRAD0] = P.vrad0;
    c->grid[FCPT_F_VAZI0] = P.vazi0;
    c->grid[FCPT_F_ENERGY0] = P.energy0;
    c->grid[FCPT_F_QPLUS] = P.qplus;
    c->grid[FCPT_F_QMINUS] = P.qminus;
    c->grid[FCPT_F_VISC_CFAC_PHI] = P.cfac_phi; // null unless StabilizeViscosity
    c->grid[FCPT_F_VISC_CFAC_R] = P.cfac_r;
    c->grid[FCPT_F_MASSFLOW] = P.massflow; // null unless WriteMassFlow
    c->grid[FCPT_F_ACCEL_RADIAL] = P.accel_r; // null unless BodyForceFromPotential: no
    c->grid[FCPT_F_ACCEL_AZIMUTHAL] = P.accel_az;
    return FCPT_OK;
}

// FCPT_TF_SCHEDULE of tuning runs: "28x56,12x24,6" = 56 chunks of 28 rings, 24 of 12, the rest of 6
std::vector<int> parse_tf_schedule(const char *q, int nr)
{
    std::vector<int> lengths;
    while (*q) {
        char *e = nullptr;
        const long a = strtol(q, &e, 10);
        if (e == q)
            break;
        long n = 1;
        q = e;
        if (*q == 'x' || *q == 'X') {
            n = strtol(q + 1, &e, 10);
            q = e;
        }
        for (long k = 0; k < n && (long)lengths.size() < 4l * nr; ++k)
            lengths.push_back((int)(a < 1 ? 1 : a));
        while (*q == ',' || *q == ' ')
            ++q;
    }
    return lengths;
}

int seed_clock(fcpt_ctx *c)
{
    DevClock clk;
    std::memset(&clk, 0, sizeof(clk));
    clk.last_dt = c->d.first_dt; // Interpret.cpp:86
    clk.dt = c->d.first_dt;
    clk.dt_min = 1.0e300;
    clk.dt_max = 0.0;
    if (hipMemcpy(c->P.clk, &clk, sizeof(clk), hipMemcpyHostToDevice) != hipSuccess) {
        set_error("hipMemcpy of the clock failed");
        return FCPT_EHIP;
    }
    return FCPT_OK;
}

} // namespace

extern "C" {

int fcpt_device_count(int32_t *n)
{
    if (!n)
        return FCPT_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) {
        (void)hipGetLastError();
        ndev = 0;
    }
    *n = ndev;
    return FCPT_OK;
}

int fcpt_set_device(int32_t device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available");
        return FCPT_ENODEV;
    }
    if (device < 0 || device >= ndev) {
        set_error("fcpt_set_device(%d): %d device(s) visible", device, ndev);
        return FCPT_EINVAL;
    }
    HIPCHK(hipSetDevice(device));
    return FCPT_OK;
}

int fcpt_create(const fcpt_desc *d, const double *radii, fcpt_ctx **out)
{
    if (!out) {
        set_error("null argument");
        return FCPT_EINVAL;
    }
    if (int rc = validate_create(d, radii))
        return rc;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available: the HIP path cannot run (there is no CPU fallback)");
        return FCPT_ENODEV;
    }
    fcpt_ctx *c = new (std::nothrow) fcpt_ctx();
    if (!c)
        return FCPT_ENOMEM;
    std::memset(&c->P, 0, sizeof(c->P)); // (padding too: the hipGraph replay compares Dev views with memcmp)
    std::memset(&c->ls, 0, sizeof(c->ls)); // (likewise)
    c->ls.ghosts_unknown = true;
    c->d = *d;
    if (d->eos != FCPT_EOS_IDEAL) // no energy equation: SubStep3 and with it every cooling term is not called
        c->d.cooling_surface = c->d.cooling_beta = 0; // (simulation.cpp:205-207 `if (parameters::Adiabatic)`)
    (void)hipGetDevice(&c->device);
    int rc = split_domain(c->d, c->s);
    if (!rc) {
        c->radii.assign(radii, radii + d->nr_global + FCPT_GEOM_PAD + 1);
        build_geometry(c->d, c->s, radii, c->geo);
        RingTables tables;
        build_ring_tables(c->d, c->s, c->geo, tables);
        rc = upload_tables(c, tables);
    }
    if (!rc)
        rc = alloc_grids(c);
    if (!rc) {
        fill_parameters(c->d, c->s, c->geo, c->P);
        rc = seed_clock(c);
    }
    if (rc) {
        fcpt_destroy(c);
        return rc;
    }
    if (const char *q = getenv("FCPT_TF_SCHEDULE"))
        c->tf_lengths = parse_tf_schedule(q, c->s.nr);
    options_from_environment(c->P.opt);
    apply_options(c);
    *out = c;
    return FCPT_OK;
}

int fcpt_set_option(fcpt_ctx *c, const char *name, int32_t value)
{
    if (!c || !name)
        return FCPT_EINVAL;
    int *slot = option_slot(c->P.opt, name);
    if (!slot) {
        set_error("fcpt_set_option: unknown option '%s'", name);
        return FCPT_EINVAL;
    }
    if (*slot == value)
        return FCPT_OK;
    if (c->ls.stepped) {
        set_error("fcpt_set_option between fcpt_step and fcpt_post");
        return FCPT_EINVAL;
    }
    join_side(c);
    // a switch may change which grids hold the derived quantities: finish what is queued, then start clean
    HIPCHK(hipStreamSynchronize(c->stream));
    *slot = value;
    apply_options(c, false);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_get_option(const fcpt_ctx *c, const char *name, int32_t *value)
{
    if (!c || !name || !value)
        return FCPT_EINVAL;
    // read-only counters of the hipGraph replay in fcpt_run_steps
    if (!std::strcmp(name, "graph_replays")) {
        *value = (int32_t)(c->graph_replays > 0x7fffffffll ? 0x7fffffffll : c->graph_replays);
        return FCPT_OK;
    }
    if (!std::strcmp(name, "transport_fell_back")) { // 1: the last transport met a ring pair beyond the one-lane shift
        fcpt_ctx *m = const_cast<fcpt_ctx *>(c);      //    and took the two-kernel path (blocks: reads the device stamps)
        int stamps[4] = {0, 0, 0, 0};
        join_side(m);
        HIPCHK(hipMemcpyAsync(stamps, c->P.shift_jump, sizeof(stamps), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        *value = (stamps[2] != 0 && stamps[0] == stamps[2]) ? 1 : 0;
        return FCPT_OK;
    }
    if (!std::strcmp(name, "coop_active")) { // always 0: fcpt_run_steps has no one-kernel-per-step path
        *value = 0;
        return FCPT_OK;
    }
    if (!std::strcmp(name, "graph_cycle")) {
        *value = c->graph_exec ? c->graph_cycle : 0;
        return FCPT_OK;
    }
    const int *slot = option_slot(const_cast<Options &>(c->P.opt), name);
    if (!slot) {
        set_error("fcpt_get_option: unknown option '%s'", name);
        return FCPT_EINVAL;
    }
    *value = *slot;
    return FCPT_OK;
}

int fcpt_set_transport_chunks(fcpt_ctx *c, const int32_t *lengths, int32_t n)
{
    if (!c || n < 0 || (n > 0 && !lengths))
        return FCPT_EINVAL;
    if (c->ls.stepped) {
        set_error("fcpt_set_transport_chunks between fcpt_step and fcpt_post");
        return FCPT_EINVAL;
    }
    for (int k = 0; k < n; ++k)
        if (lengths[k] < 1) {
            set_error("fcpt_set_transport_chunks: chunk %d has %d rings", k, (int)lengths[k]);
            return FCPT_EINVAL;
        }
    join_side(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    c->tf_lengths.assign(lengths, lengths + n);
    apply_options(c, false);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_transport_chunks(const fcpt_ctx *c, int32_t *tile_first_last, int32_t capacity, int32_t *n_wavefronts)
{
    if (!c || !n_wavefronts || capacity < 0 || (capacity > 0 && !tile_first_last))
        return FCPT_EINVAL;
    const int n = (int)(c->tf_sched_host.size() / 4);
    *n_wavefronts = n;
    for (int k = 0; k < n && k < capacity; ++k)
        for (int q = 0; q < 3; ++q)
            tile_first_last[3 * k + q] = c->tf_sched_host[4 * k + q];
    return FCPT_OK;
}

int fcpt_set_source_chunks(fcpt_ctx *c, const int32_t *lengths, int32_t n)
{
    if (!c || n < 0 || (n > 0 && !lengths))
        return FCPT_EINVAL;
    if (c->ls.stepped) {
        set_error("fcpt_set_source_chunks between fcpt_step and fcpt_post");
        return FCPT_EINVAL;
    }
    const std::vector<int> list(lengths, lengths + n);
    bool refused = false;
    const std::vector<int> table = source_schedule_explicit(c->P, list, &refused);
    if (refused) { // the launcher folds the boundary call into the edge chunks of a table: three rows each at least
        int k = 0;
        while (k + 1 < n && list[k] >= 3)
            ++k;
        set_error("fcpt_set_source_chunks: chunk %d has %d rings, fewer than 3", k, list[k]);
        return FCPT_EINVAL;
    }
    if (table.size() > c->sm_sched_cap) {
        set_error("fcpt_set_source_chunks: %d wavefronts, the table holds %d", (int)(table.size() / 4), (int)(c->sm_sched_cap / 4));
        return FCPT_EINVAL;
    }
    join_side(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    c->sm_lengths = list;
    apply_options(c, false);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_source_chunks(const fcpt_ctx *c, int32_t *seg_first_last, int32_t capacity, int32_t *n_wavefronts)
{
    if (!c || !n_wavefronts || capacity < 0 || (capacity > 0 && !seg_first_last))
        return FCPT_EINVAL;
    const int n = (int)(c->sm_sched_host.size() / 4);
    *n_wavefronts = n;
    for (int k = 0; k < n && k < capacity; ++k)
        for (int q = 0; q < 3; ++q)
            seg_first_last[3 * k + q] = c->sm_sched_host[4 * k + q];
    return FCPT_OK;
}

int fcpt_destroy(fcpt_ctx *c)
{
    if (!c)
        return FCPT_OK;
    (void)fcpt_comm_destroy(c);
    drop_graph(c);
    if (c->capture_stream)
        (void)hipStreamDestroy(c->capture_stream);
    particles_free(c);
    selfgravity_free(c);
    for (void *p : c->allocs)
        (void)hipFree(p);
    if (c->h_clk)
        (void)hipHostFree(c->h_clk);
    if (c->dob_host)
        (void)hipHostFree(c->dob_host);
    if (c->e_dob)
        (void)hipEventDestroy(c->e_dob);
    for (hipEvent_t e : c->prof.events)
        (void)hipEventDestroy(e);
    if (c->side) {
        (void)hipStreamSynchronize(c->side);
        (void)hipStreamDestroy(c->side);
    }
    if (c->e_fork)
        (void)hipEventDestroy(c->e_fork);
    if (c->e_join)
        (void)hipEventDestroy(c->e_join);
    delete c;
    return FCPT_OK;
}

int fcpt_set_stream(fcpt_ctx *c, void *hip_stream)
{
    if (!c)
        return FCPT_EINVAL;
    join_side(c);
    c->stream = (hipStream_t)hip_stream;
    return FCPT_OK;
}

int fcpt_synchronize(fcpt_ctx *c)
{
    if (!c)
        return FCPT_EINVAL;
    DevClock k;
    return read_clock(c, &k); // synchronises, and reports a step beyond the shear limit
}

int fcpt_get_split(const fcpt_ctx *c, fcpt_split *out)
{
    if (!c || !out)
        return FCPT_EINVAL;
    *out = c->s;
    return FCPT_OK;
}

int fcpt_get_clock(const fcpt_ctx *cc, fcpt_clock *out)
{
    fcpt_ctx *c = const_cast<fcpt_ctx *>(cc);
    if (!c || !out)
        return FCPT_EINVAL;
    DevClock k;
    if (int rc = read_clock(c, &k))
        return rc;
    out->time = k.time;
    out->last_dt = k.last_dt;
    out->n_hydro_iter = k.n_hydro_iter;
    out->n_monitor = k.n_monitor;
    out->n_snapshot = k.n_snapshot;
    return FCPT_OK;
}

// hydro_dt_logger (hydro_dt_logger.h:13-34)
int fcpt_dt_statistics(fcpt_ctx *c, double *dt_min, double *dt_max, int32_t reset)
{
    if (!c)
        return FCPT_EINVAL;
    DevClock k;
    if (int rc = read_clock(c, &k))
        return rc;
    if (dt_min)
        *dt_min = k.dt_min;
    if (dt_max)
        *dt_max = k.dt_max;
    if (reset) {
        k.dt_min = 1.0e300;
        k.dt_max = 0.0;
        *c->h_clk = k;
        HIPCHK(hipMemcpyAsync(c->P.clk, c->h_clk, sizeof(DevClock), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return FCPT_OK;
}

int fcpt_set_clock(fcpt_ctx *c, const fcpt_clock *in)
{
    if (!c || !in)
        return FCPT_EINVAL;
    DevClock k;
    if (int rc = read_clock(c, &k))
        return rc;
    k.time = in->time;
    k.last_dt = in->last_dt;
    k.n_hydro_iter = in->n_hydro_iter;
    k.n_monitor = in->n_monitor;
    k.n_snapshot = in->n_snapshot;
    // (the shift-jump stamps of k_ring_mean are sequence numbers derived from n_hydro_iter: none may survive a clock
    //  that is set back)
    HIPCHK(hipMemsetAsync(c->P.shift_jump, 0, 8 * sizeof(int), c->stream));
    *c->h_clk = k;
    HIPCHK(hipMemcpyAsync(c->P.clk, c->h_clk, sizeof(DevClock), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPT_OK;
}

static size_t grid_count(const fcpt_ctx *c, int32_t f)
{
    const bool vec = f == FCPT_F_VRAD || f == FCPT_F_VRAD0 || f == FCPT_F_MASSFLOW || f == FCPT_F_ACCEL_RADIAL ||
                     f == FCPT_F_ACCEL_AZIMUTHAL;
    return (size_t)(c->s.nr + (vec ? 1 : 0)) * c->d.nphi;
}

int fcpt_upload(fcpt_ctx *c, int32_t f, const double *host)
{
    if (!c || !host || f < 0 || f >= FCPT_F_COUNT || !c->grid[f]) {
        set_error("bad argument to fcpt_upload");
        return FCPT_EINVAL;
    }
    join_side(c);
    HIPCHK(hipMemcpyAsync(c->grid[f], host, grid_count(c, f) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (f == FCPT_F_SIGMA || f == FCPT_F_VRAD || f == FCPT_F_VAZI || f == FCPT_F_ENERGY) {
        // a replaced state grid: nothing derived from the old one may be reused.  The non-lazy ideal-EOS paths read
        // c_s, H, nu, T from grids that only fcpt_init_physics / fcpt_recalculate_derived / fcpt_post refresh --
        // that contract (restart_load, restart.cpp:18-139) stays; what the library evaluates lazily is redone.
        c->ls.pressure_valid = false;
        c->ls.potential_valid = false;
        c->ls.stepped = false;
        c->ls.ghosts_unknown = true;
        drop_graph(c); // its launches were chosen for ghost rings that satisfied the boundary conditions
    }
    if (f == FCPT_F_QPLUS || f == FCPT_F_QMINUS)
        c->ls.qdiff_valid = false;
    if (f == FCPT_F_SCALE_HEIGHT)
        c->ls.potential_valid = false;
    c->ls.cfl_interior = false;
    return FCPT_OK;
}

int fcpt_download(fcpt_ctx *c, int32_t f, double *host)
{
    if (!c || !host || f < 0 || f >= FCPT_F_COUNT || !c->grid[f]) {
        set_error("bad argument to fcpt_download");
        return FCPT_EINVAL;
    }
    join_side(c);
    if (f == FCPT_F_PRESSURE || (c->P.adiabatic && (f == FCPT_F_SOUNDSPEED || f == FCPT_F_SCALE_HEIGHT ||
                                                     f == FCPT_F_VISCOSITY || f == FCPT_F_TEMPERATURE)))
        ensure_pressure(c);
    if (f == FCPT_F_POTENTIAL && (!c->ls.potential_valid || c->P.accel_force)) {
        // evaluated inside the source march (ideal EOS), or not at all (BodyForceFromPotential: no): the grid on
        // request, from the current state and bodies
        launch_potential(c->P, c->stream);
        if (!c->P.accel_force) // (there the flag speaks for the acceleration grids)
            c->ls.potential_valid = !c->P.adiabatic;
    }
    HIPCHK(hipMemcpyAsync(host, c->grid[f], grid_count(c, f) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPT_OK;
}

int fcpt_device_ptr(fcpt_ctx *c, int32_t f, void **dptr, uint64_t *count)
{
    if (!c || !dptr || f < 0 || f >= FCPT_F_COUNT || !c->grid[f])
        return FCPT_EINVAL;
    *dptr = c->grid[f];
    if (count)
        *count = grid_count(c, f);
    return FCPT_OK;
}

int fcpt_set_bodies(fcpt_ctx *c, int32_t n, const double *x, const double *y, const double *m,
                    const double *rsm, double ix, double iy)
{
    if (!c || n < 0 || n > FCPT_MAX_BODIES || (n > 0 && (!x || !y || !m))) {
        set_error("bad argument to fcpt_set_bodies (at most %d bodies)", FCPT_MAX_BODIES);
        return FCPT_EINVAL;
    }
    Dev &P = c->P;
    P.nbodies = n;
    for (int k = 0; k < n; ++k) {
        P.bx[k] = x[k];
        P.by[k] = y[k];
        P.bm[k] = m[k];
        P.brsm[k] = rsm ? rsm[k] : 0.0;
    }
    P.indirect_x = ix;
    P.indirect_y = iy;
    c->ls.potential_valid = false;
    c->ls.has_mid = false;
    return FCPT_OK;
}

int fcpt_set_bodies_midstep(fcpt_ctx *c, int32_t n, const double *x, const double *y, const double *m,
                            const double *rsm)
{
    if (!c || n != c->P.nbodies || (n > 0 && (!x || !y || !m))) {
        set_error("fcpt_set_bodies_midstep must follow fcpt_set_bodies with the same number of bodies");
        return FCPT_EINVAL;
    }
    for (int k = 0; k < n; ++k) {
        c->mx[k] = x[k];
        c->my[k] = y[k];
        c->mm[k] = m[k];
        c->mrsm[k] = rsm ? rsm[k] : 0.0;
    }
    c->ls.has_mid = true;
    return FCPT_OK;
}

// init_euler (SourceEuler.cpp:251-285) + the tail of init_physics (init.cpp:337-341)
int fcpt_set_body_irradiation(fcpt_ctx *c, int32_t n, const double *temperature, const double *radius,
                              const double *rampup_time)
{
    if (!c || n < 0 || n > FCPT_MAX_BODIES || (n > 0 && (!temperature || !radius))) {
        set_error("bad argument to fcpt_set_body_irradiation");
        return FCPT_EINVAL;
    }
    if (!c->P.adiabatic) {
        set_error("irradiation needs EquationOfState: ideal");
        return FCPT_EINVAL;
    }
    c->P.heating_star = 0;
    for (int k = 0; k < FCPT_MAX_BODIES; ++k) {
        c->P.btemp[k] = k < n ? temperature[k] : 0.0;
        c->P.bradius[k] = k < n ? radius[k] : 0.0;
        c->P.bramp[k] = (k < n && rampup_time) ? rampup_time[k] : 0.0;
        if (c->P.btemp[k] > 0.0)
            c->P.heating_star = 1; // planetary_system.cpp:137-146
    }
    return FCPT_OK;
}

int fcpt_disk_on_body_accel(fcpt_ctx *c, double x, double y, double r_object, double smoothing_fixed,
                            double cubic_smoothing_radius, double out[4])
{
    if (!c || !out)
        return FCPT_EINVAL;
    join_side(c);
    ProfScope prof_scope(c);
    if (smoothing_fixed < 0.0 && c->P.adiabatic && !c->P.lazy_derived)
        ensure_pressure(c); // the scale-height grid
    double *d_out = c->P.cfl_part + 4 * (size_t)(((c->P.nphi + 255) / 256) * (c->P.nr / DOB_ROWS_HOST + 2));
    launch_disk_on_body(c->P, x, y, r_object, smoothing_fixed, cubic_smoothing_radius, d_out, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out, 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return FCPT_OK;
}

int fcpt_disk_on_bodies_begin(fcpt_ctx *c, int32_t n, const double *x, const double *y, const double *r_object,
                              const double *smoothing_fixed, const double *cubic_smoothing_radius)
{
    if (!c || n < 1 || n > FCPT_MAX_BODIES || !x || !y || !r_object || !smoothing_fixed || !cubic_smoothing_radius) {
        set_error("fcpt_disk_on_bodies_begin: null argument or n = %d outside 1 .. %d", (int)n, FCPT_MAX_BODIES);
        return FCPT_EINVAL;
    }
    const size_t nblocks = disk_on_bodies_blocks(c->P);
    if (!c->dob_part) {
        if (int rc = dev_alloc(c, &c->dob_part, 4 * (nblocks + 1) * FCPT_MAX_BODIES))
            return rc;
        if (hipHostMalloc((void **)&c->dob_host, 4 * FCPT_MAX_BODIES * sizeof(double)) != hipSuccess) {
            set_error("hipHostMalloc failed");
            return FCPT_ENOMEM;
        }
        HIPCHK(hipEventCreateWithFlags(&c->e_dob, hipEventDisableTiming));
    }
    join_side(c);
    ProfScope prof_scope(c);
    DiskBodies B;
    std::memset(&B, 0, sizeof(B));
    bool need_h = false;
    for (int k = 0; k < n; ++k) {
        B.x[k] = x[k];
        B.y[k] = y[k];
        B.r_object[k] = r_object[k];
        B.smoothing_fixed[k] = smoothing_fixed[k];
        B.r_sm[k] = cubic_smoothing_radius[k];
        need_h = need_h || smoothing_fixed[k] < 0.0;
    }
    if (need_h && c->P.adiabatic && !c->P.lazy_derived)
        ensure_pressure(c); // the scale-height grid
    double *d_out = c->dob_part + 4 * nblocks * FCPT_MAX_BODIES;
    launch_disk_on_bodies(c->P, n, B, c->dob_part, d_out, c->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->dob_host, d_out, 4 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(c->e_dob, c->stream));
    c->dob_pending = n;
    return FCPT_OK;
}

int fcpt_disk_on_bodies_end(fcpt_ctx *c, double *out)
{
    if (!c || !out || c->dob_pending < 1) {
        set_error("fcpt_disk_on_bodies_end without a pending fcpt_disk_on_bodies_begin");
        return FCPT_EINVAL;
    }
    HIPCHK(hipEventSynchronize(c->e_dob));
    std::memcpy(out, c->dob_host, 4 * (size_t)c->dob_pending * sizeof(double));
    c->dob_pending = 0;
    return FCPT_OK;
}

int fcpt_init_physics(fcpt_ctx *c)
{
    if (!c)
        return FCPT_EINVAL;
    ProfScope prof_scope(c);
    const Dev &P = c->P;
    hipStream_t st = c->stream;
    if (!P.adiabatic) {
        launch_iso_cs_h(P, c->d_cs_ring, st);
        launch_pressure(P, st);
        launch_temperature(P, st);
    } else {
        launch_temperature(P, st);
        launch_recalculate_viscosity(P, st); // cs, H (and nu when alpha)
        launch_pressure(P, st);
    }
    launch_viscosity_field(P, st);
    // compute_heating_cooling_for_CFL (SourceEuler.cpp:1507-1547) runs before the velocities
    // are initialised (init.cpp:331-332): the gas is at rest, the stress tensor vanishes and
    // Q+ = Q- = 0, which is what the zero-filled grids already hold.
    const size_t ns = (size_t)P.nr * P.nphi * sizeof(double);
    HIPCHK(hipMemsetAsync(P.qplus, 0, ns, st));
    HIPCHK(hipMemsetAsync(P.qminus, 0, ns, st));
    // ... and its compute_viscous_stress_tensor leaves the StabilizeViscosity factors (functions of nu and Sigma
    // only) behind: with StabilizeViscosity 2 they limit the very first time step (cfl.cpp:331-351)
    if (P.adiabatic)
        launch_visc_factors(P, st);
    if (P.adiabatic && (P.cooling_surface || P.cooling_beta || P.heating_star)) {
        // ... but Q- does not vanish: calculate_qminus + the 1/alpha of compute_heating_cooling_for_CFL
        Dev I = P;
        I.cooling_at_init = 1;
        launch_substep3_cooling_only(I, st);
    }
    if (int rc = copy_initial_values(c))
        return rc;
    apply_boundary(c, false);
    if (int rc = copy_initial_values(c))
        return rc;
    c->ls.potential_valid = false;
    c->ls.pressure_valid = true;
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}


// recalculate_derived_disk_quantities (SourceEuler.cpp:225-249) after the state grids were replaced from outside
int fcpt_recalculate_derived(fcpt_ctx *c)
{
    if (!c)
        return FCPT_EINVAL;
    join_side(c);
    ProfScope prof_scope(c);
    c->ls.stepped = false;
    c->ls.cfl_interior = false;
    c->ls.potential_valid = false;
    refresh_derived(c);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

// test hook: the transport kernels' half_limiter on host-supplied operands
int fcpt_selftest_half_limiter(int32_t limiter, int64_t n, const double *a, const double *b, double *out)
{
    if (n < 0 || (n > 0 && (!a || !b || !out)) || (limiter != FCPT_LIMITER_VANLEER && limiter != FCPT_LIMITER_MC))
        return FCPT_EINVAL;
    if (n == 0)
        return FCPT_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available");
        return FCPT_ENODEV;
    }
    double *d = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    HIPCHK(hipMalloc((void **)&d, 3 * nb));
    int rc = FCPT_OK;
    if (hipMemcpy(d, a, nb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + n, b, nb, hipMemcpyHostToDevice) != hipSuccess)
        rc = FCPT_EHIP;
    if (!rc) {
        launch_selftest_half_limiter(limiter, n, d, d + n, d + 2 * n, nullptr);
        if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, d + 2 * n, nb, hipMemcpyDeviceToHost) != hipSuccess)
            rc = FCPT_EHIP;
    }
    (void)hipFree(d);
    if (rc)
        set_error("fcpt_selftest_half_limiter: a HIP call failed");
    return rc;
}

// test hook: the chunk tables of the marching kernels as pure host logic
int fcpt_selftest_chunk_tables(int32_t nr, int32_t nphi, int32_t n_cu, int32_t adiabatic, int32_t damp_inner, int32_t damp_outer,
                               int32_t *transport_first_last, int32_t transport_capacity, int32_t *n_transport,
                               int32_t *source_seg_first_last, int32_t source_capacity, int32_t *n_source)
{
    if (nr < 1 || nphi < 1 || n_cu < 8 || damp_inner < 0 || damp_outer < 0 || !n_transport || !n_source || transport_capacity < 0 ||
        source_capacity < 0 || (transport_capacity > 0 && !transport_first_last) || (source_capacity > 0 && !source_seg_first_last))
        return FCPT_EINVAL;
    Options opt{};
    options_from_environment(opt);
    std::vector<int> t, s;
    selftest_chunk_tables(nr, nphi, n_cu, adiabatic != 0, damp_inner, damp_outer, opt, t, s);
    *n_transport = (int32_t)(t.size() / 4);
    *n_source = (int32_t)(s.size() / 4);
    for (int k = 0; k < *n_transport && k < transport_capacity; ++k)
        for (int q = 0; q < 3; ++q)
            transport_first_last[3 * k + q] = t[4 * k + q];
    for (int k = 0; k < *n_source && k < source_capacity; ++k)
        for (int q = 0; q < 3; ++q)
            source_seg_first_last[3 * k + q] = s[4 * k + q];
    return FCPT_OK;
}

int32_t fcpt_kernel_count(void) { return KID_COUNT; }
const char *fcpt_kernel_name(int32_t id) { return (id >= 0 && id < KID_COUNT) ? kKernelNames[id] : ""; }

int fcpt_profile_start(fcpt_ctx *c, uint64_t mask, int32_t max_launches)
{
    if (!c || max_launches < 0)
        return FCPT_EINVAL;
    Profiler &p = c->prof;
    while ((int)p.events.size() < 2 * max_launches) {
        hipEvent_t e;
        HIPCHK(hipEventCreate(&e));
        p.events.push_back(e);
    }
    p.mask = mask;
    p.used = 0;
    p.open_id = -1;
    p.stride = c->P.opt.profile_stride > 1 ? c->P.opt.profile_stride : 1;
    p.seen = 0;
    p.ids.clear();
    c->profiling = true;
    return FCPT_OK;
}

int fcpt_profile_stop(fcpt_ctx *c, double *ms_total, int64_t *launches)
{
    if (!c || !ms_total || !launches)
        return FCPT_EINVAL;
    c->profiling = false;
    join_side(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < KID_COUNT; ++k) {
        ms_total[k] = 0.0;
        launches[k] = 0;
    }
    Profiler &p = c->prof;
    for (size_t n = 0; n < p.ids.size(); ++n) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, p.events[2 * n], p.events[2 * n + 1]));
        ms_total[p.ids[n]] += ms;
        launches[p.ids[n]] += 1;
    }
    return FCPT_OK;
}

} // extern "C"
