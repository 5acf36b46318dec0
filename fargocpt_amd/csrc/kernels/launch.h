// Part of fcpt_kernels.hip (one translation unit, namespace fcpt): kernel names, per-kernel HIP-event profiler, launchers.
// Not a stand-alone header: included once, in the order given there.

// ---------------------------------------------------------------------------
// per-kernel HIP-event timing (fcpt_profile_start/stop)
const char *const kKernelNames[KID_COUNT] = {
    "k_potential", "k_adi_derived", "k_iso_cs_h", "k_viscosity", "k_pressure", "k_temperature",
    "k_substep3", "k_boundary", "k_damping", "k_transport_radial",
    "k_ring_mean", "k_transport_theta<1>", "k_transport_theta<2>", "k_velocities", "k_cfl_final",
    "k_cfl_cells", "k_clock", "k_src_fused", "k_av_fused", "k_visc_fused", "k_source_march",
    "k_transport_theta_march", "k_transport_fused", "k_massflow", "k_cfl_rings", "k_theta_march_gated_boundary",
    "k_exchange_copy", "k_disk_on_body", "k_visc_factors", "k_source_march_adi", "k_source_march_adi_wide",
    "k_accel_on_gas", "k_source_march_adi_acc",
    "k_transport_radial_means", "k_cfl_rings_bc", "k_disk_on_bodies", "k_particles_step", "k_particles_step_explicit",
    "k_particles_emigrate", "k_particles_emigrate_finish", "k_particles_immigrate", "k_particles_emigrate_count",
    "k_sg_fft_rows", "k_sg_transpose", "k_sg_multiply", "k_sg_kick"};

thread_local Profiler *g_prof = nullptr;

void Profiler::begin(int id, hipStream_t st)
{
    if (!((mask >> id) & 1ull) || used + 2 > (int)events.size())
        return;
    if (stride > 1 && (seen++ % stride) != 0)
        return;
    (void)hipEventRecord(events[used], st);
    open_id = id;
}
void Profiler::end(int id, hipStream_t st)
{
    if (open_id != id)
        return;
    (void)hipEventRecord(events[used + 1], st);
    ids.push_back(id);
    used += 2;
    open_id = -1;
}

#define KLAUNCH(id, kernel, grid, block, ...)                              \
    do {                                                                   \
        if (g_prof)                                                        \
            g_prof->begin((id), st);                                       \
        hipLaunchKernelGGL(kernel, (grid), (block), 0, st, __VA_ARGS__);   \
        if (g_prof)                                                        \
            g_prof->end((id), st);                                         \
    } while (0)

// ---------------------------------------------------------------------------
// runtime values -> template arguments.  f is a generic lambda; it is called with a std::integral_constant, whose
// value TARG() names in a template argument list.  Only the alternatives spelled at the call are instantiated.
template <int V> using int_c = std::integral_constant<int, V>;
#define TARG(c_) decltype(c_)::value
template <class F> static void with_bool(bool b, F &&f)
{
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}
template <int... Vs, class F> static void with_value(int v, F &&f) // v is one of Vs (else nothing is called)
{
    (void)((v == Vs && (f(int_c<Vs>{}), true)) || ...);
}

// compute units of the current device (one device per process): the only HIP query the chunk planner depends on, made
// once and handed to it as an argument (fcpt_schedule.h)
int device_cus()
{
    static const int n_cu = [] {
        int dev = 0, v = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0)
            v = 64;
        return v;
    }();
    return n_cu;
}

// ---------------------------------------------------------------------------
// launchers
#define LAUNCH2D(id, kernel, nrows, ...)                                             \
    do {                                                                             \
        if ((nrows) > 0) {                                                           \
            const Launch2D l = launch2d((nrows), P.nphi);                            \
            if (l.block.x >= 64)                                                     \
                KLAUNCH(id, (kernel<true>), l.grid, l.block, __VA_ARGS__);           \
            else                                                                     \
                KLAUNCH(id, (kernel<false>), l.grid, l.block, __VA_ARGS__);          \
        }                                                                            \
    } while (0)
#define LAUNCH2D_T(id, kernel, targ, nrows, ...)                                     \
    do {                                                                             \
        if ((nrows) > 0) {                                                           \
            const Launch2D l = launch2d((nrows), P.nphi);                            \
            if (l.block.x >= 64)                                                     \
                KLAUNCH(id, (kernel<targ, true>), l.grid, l.block, __VA_ARGS__);     \
            else                                                                     \
                KLAUNCH(id, (kernel<targ, false>), l.grid, l.block, __VA_ARGS__);    \
        }                                                                            \
    } while (0)

void launch_potential(const Dev &P, hipStream_t st) { LAUNCH2D(KID_POTENTIAL, k_potential, P.nr, P); }
void launch_accel_on_gas(const Dev &P, hipStream_t st) { LAUNCH2D(KID_ACCEL_ON_GAS, k_accel_on_gas, P.nr - 1, P); }
void launch_body_force(const Dev &P, hipStream_t st)
{
    if (P.accel_force)
        launch_accel_on_gas(P, st);
    else
        launch_potential(P, st);
}

void launch_recalculate_viscosity(const Dev &P, hipStream_t st)
{
    // recalculate_viscosity, SourceEuler.cpp:205-223 (AspectRatioMode 0): c_s, H (and nu when alpha) in one launch;
    // the isothermal alpha-nu never changes after init
    if (P.adiabatic)
        LAUNCH2D(KID_ADI_CS_H, k_adi_derived, P.nr, P, 0);
}

void launch_viscosity_field(const Dev &P, hipStream_t st) { LAUNCH2D(KID_VISCOSITY, k_viscosity, P.nr, P); }

void launch_iso_cs_h(const Dev &P, const double *cs_ring, hipStream_t st)
{
    LAUNCH2D(KID_ISO_CS_H, k_iso_cs_h, P.nr, P, cs_ring);
}

void launch_source_fused(const Dev &P, hipStream_t st)
{
    if (P.accel_force)
        LAUNCH2D_T(KID_SRC_FUSED, k_src_fused, true, P.nr + 1, P);
    else
        LAUNCH2D_T(KID_SRC_FUSED, k_src_fused, false, P.nr + 1, P);
    LAUNCH2D(KID_AV_FUSED, k_av_fused, P.nr + 1, P);
}
// whole source step in one marching pass (Nphi >= 128); returns 0 if not applicable, else +-segments (> 0: ring sums
// of v_phi were left for the transport).  fold_bc: the caller's next call is apply_boundary_condition(final = false) on
// the kick's result -- *bc_folded reports whether the kernel applied it itself (boundary_column on its edge chunks)
// fold_cfl: the launch stands directly behind the ring kernel of the CFL reduction (launch_cfl / launch_cfl_bc with
// apply_policy = 2): its workgroups fold the reduction and apply the time-step policy themselves (cfl_fold_in_step)
int launch_source_march(const Dev &P, hipStream_t st, bool fold_bc, bool *bc_folded, bool fold_cfl)
{
    if (bc_folded)
        *bc_folded = false;
    if (!source_march_applies(P))
        return 0;
    int bc_fold = 0;
    const bool sched = P.sm_sched_n > 0 && P.opt.source_rows <= 0; // rank-matched chunks (every one of them >= 3 rings)
    // isothermal, measured at 2048x4096: 16 / 24 / 32 / 48 / 64 rings -> 0.133 / 0.132 / 0.141 / 0.152 / 0.188 ms
    const int rows = source_rows(P, device_cus());
    const int segs = segments_of(P.nphi);
    const int chunks = (P.nr + 1 + rows - 1) / rows;
    {
        // the boundary conditions read rows 1, 2 and nr-2 .. nr of the kick's result: the wavefront that applies them
        // must have stored those rows itself
        const int first_rows = sched ? 3 : rows, last_rows = sched ? 3 : (P.nr + 1) - (chunks - 1) * rows;
        if (fold_bc && P.opt.bc_fold != 0 && first_rows >= 3 && last_rows >= 3 && P.nr >= 6 && (!P.adiabatic || P.opt.march_source_adi != 0)) {
            bc_fold = 1;
            if (bc_folded)
                *bc_folded = true;
        }
    }
    if (fold_cfl)
        bc_fold |= 2;
    // per-segment ring sums of v_phi, so that the transport's k_ring_mean reads 70 partials per ring
    // instead of the ring itself
    const int ring_sums = segs <= P.ring_pstride && P.opt.source_ring_parts != 0;
    const int waves = sched ? P.sm_sched_n : segs * chunks; // (the table holds whole workgroups)
    const dim3 grid((waves + 3) / 4), block(256);
    const bool cool = P.cooling_surface != 0 || P.cooling_beta != 0 || P.heating_star != 0;
    const bool stab = P.stabilize != 0;
    const int av = P.art_visc == FCPT_ARTVISC_TW ? 1 : (P.art_visc == FCPT_ARTVISC_SN ? 2 : 0);
    with_value<0, 1, 2>(av, [&](auto AV) {
        if (!P.adiabatic) {
            with_bool(stab, [&](auto STAB) {
                with_bool(P.accel_force, [&](auto ACC) {
                    KLAUNCH(KID_SOURCE_MARCH, (k_source_march<TARG(AV), TARG(STAB), TARG(ACC)>), grid, block, P, segs, rows, ring_sums, bc_fold);
                });
            });
        } else if (P.accel_force) {
            with_bool(cool, [&](auto COOL) {
                with_bool(stab, [&](auto STAB) {
                    KLAUNCH(KID_SOURCE_MARCH_ADI_ACC, (k_source_march_adi_acc<TARG(AV), TARG(COOL), TARG(STAB)>), grid, block, P, segs, rows, ring_sums, bc_fold);
                });
            });
        } else {
            with_bool(P.inline_potential, [&](auto POT) {
                if (!cool && !stab) { // the narrow kernel has no instance with cooling terms or StabilizeViscosity
                    KLAUNCH(KID_SOURCE_MARCH_ADI, (k_source_march_adi<TARG(AV), TARG(POT)>), grid, block, P, segs, rows, ring_sums, bc_fold);
                    return;
                }
                with_bool(cool, [&](auto COOL) {
                    with_bool(stab, [&](auto STAB) {
                        KLAUNCH(KID_SOURCE_MARCH_ADI_WIDE, (k_source_march_adi_wide<TARG(AV), TARG(COOL), TARG(POT), TARG(STAB)>), grid, block, P, segs, rows, ring_sums, bc_fold);
                    });
                });
            });
        }
    });
    return ring_sums ? segs : -segs; // < 0: marched, but no ring sums
}
// stress tensor + viscous update, and for the energy equation viscous heating and -- cell-local, on the Q+ just
// formed -- SubStep3 (SourceEuler.cpp:956-1051) with the temperature floor / ceiling behind it (the TEMPERATURE grid
// the reference refreshes there is read by nothing before recalculate_derived_disk_quantities rewrites it)
// StabilizeViscosity: the factor grids are those of launch_visc_factors, queued ahead by the caller
void launch_viscous_fused(const Dev &P, hipStream_t st)
{
    if (P.stabilize == 1)
        LAUNCH2D_T(KID_VISC_FUSED, k_visc_fused, true, P.nr + 1, P);
    else
        LAUNCH2D_T(KID_VISC_FUSED, k_visc_fused, false, P.nr + 1, P);
}

// viscosity.cpp:256-348: the correction factors depend on nu and Sigma only
void launch_visc_factors(const Dev &P, hipStream_t st)
{
    if (P.stabilize)
        LAUNCH2D(KID_VISC_FACTORS, k_visc_factors, P.nr - 1, P);
}

void launch_substep3_cooling_only(const Dev &P, hipStream_t st)
{
    // compute_heating_cooling_for_CFL at init (SourceEuler.cpp:1507-1547): Q+ = 0 (gas at rest), Q- / alpha
    LAUNCH2D(KID_SUBSTEP3, k_substep3, P.nr, P, 0);
}

// rows [7,14) and [nr-14,nr-7) -> buffers (unpack = 0), buffers -> rows [0,7) and [nr-7,nr) (unpack = 1)
void launch_exchange_copy(const Dev &P, double *inner, double *outer, int unpack, hipStream_t st)
{
    ExchangeArgs a;
    a.field[0] = P.sigma;
    a.field[1] = P.vrad;
    a.field[2] = P.vazi;
    a.field[3] = P.energy;
    a.buf[0] = inner;
    a.buf[1] = outer;
    a.row0[0] = unpack ? 0 : FCPT_OVERLAP;
    a.row0[1] = unpack ? P.nr - FCPT_OVERLAP : P.nr - 2 * FCPT_OVERLAP;
    a.nq = P.adiabatic ? 4 : 3;
    a.nphi = P.nphi;
    a.unpack = unpack;
    const size_t npair = ((size_t)FCPT_OVERLAP * P.nphi) >> 1;
    int bx = (int)((npair + 255) / 256);
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
    KLAUNCH(KID_EXCHANGE_COPY, k_exchange_copy, dim3(bx, 2 * a.nq), dim3(256), a);
}

void launch_selftest_half_limiter(int type, long long n, const double *a, const double *b, double *out, hipStream_t st)
{
    hipLaunchKernelGGL(k_selftest_half_limiter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, type, n, a, b, out);
}

void launch_boundary(const Dev &P, hipStream_t st)
{
    const int bs = 256;
    KLAUNCH(KID_BOUNDARY, k_boundary, dim3((P.nphi + bs - 1) / bs), dim3(bs), P);
}

void launch_damping(const Dev &P, double *q, double *q0, const double *radius, const DampRange &r,
                    int is_density, hipStream_t st)
{
    if (r.type == FCPT_DAMP_NONE || r.lo > r.hi)
        return;
    KLAUNCH(KID_DAMPING, k_damping, dim3(r.hi - r.lo + 1), dim3(256), P, q, q0, radius, r.lo, r.type, r.rlim,
            r.redge, r.tau, is_density);
}

#ifndef FALLBACK_BLOCKS
#define FALLBACK_BLOCKS 256 /* grid of the idle in-stream fallback kernels */
#endif
// one radial sweep + ring means (T1-T4); only_if: see k_transport_radial
static void launch_radial(const Dev &P, const int *only_if, hipStream_t st)
{
    const int rows = march_len(P, device_cus(), RADIAL_ROWS);
    const Launch2D l = launch2d((P.nr + rows - 1) / rows, P.nphi);
    const int gx = (int)l.grid.x, gy = (int)l.grid.y;
    const dim3 grid(only_if && gx * gy > FALLBACK_BLOCKS ? FALLBACK_BLOCKS : gx * gy);
    with_bool(l.block.x >= 64, [&](auto ROWU) {
        KLAUNCH(KID_TRANSPORT_RADIAL, k_transport_radial<TARG(ROWU)>, grid, l.block, P, only_if, gx, gy, rows);
    });
}
void launch_massflow(const Dev &P, hipStream_t st)
{
    if (P.massflow)
        LAUNCH2D(KID_MASSFLOW, k_massflow, P.nr - 1, P);
}
void launch_shift_means(const Dev &P, hipStream_t st)
{
    KLAUNCH(KID_RING_MEAN, k_ring_mean, dim3((P.nr + 3) / 4), dim3(256), P, 1,
            P.src_ring_nparts ? (const double *)P.ring_part : (const double *)nullptr, P.src_ring_nparts, P.ring_pstride);
}
// tiles, rings per wavefront and workgroups of the azimuthal marching kernels with C cells per lane
struct ThetaGeometry {
    int tiles, rows, nvb;
};
static ThetaGeometry theta_geometry(const Dev &P, int C, int periodic)
{
    const int tstride = 64 * C - (THETA_LO + THETA_HI);
    const int tiles = periodic ? 1 : (P.nphi + tstride - 1) / tstride;
    const int rows = P.opt.theta_rows > 0 ? P.opt.theta_rows : march_len(P, device_cus(), THETA_ROWS);
    const int chunks = (P.nr + rows - 1) / rows;
    return {tiles, rows, (chunks * tiles + 3) / 4};
}
// azimuthal marching kernel on set B -> state grids of Wm; returns the tile count
static int launch_theta_march(const Dev &P, const Dev &Wm, int C, int periodic, int advance, const int *only_if,
                              hipStream_t st)
{
    const ThetaSet inB = {P.rmpB, P.rmmB, P.lpB, P.lmB, P.sigB, P.eB};
    const ThetaGeometry g = theta_geometry(P, C, periodic);
    const dim3 grid(only_if && g.nvb > FALLBACK_BLOCKS ? FALLBACK_BLOCKS : g.nvb), block(256);
    auto march = [&](auto CC, auto PP) {
        with_bool(P.adiabatic, [&](auto AA) {
            with_bool(Wm.damp_in_step, [&](auto DD) {
                KLAUNCH(KID_THETA_MARCH, (k_transport_theta_march<TARG(CC), TARG(AA), TARG(DD), TARG(PP)>), grid, block, Wm,
                        (const double *)P.vazi, (const double *)P.vrad, inB, g.tiles, g.rows, advance, only_if, g.nvb);
            });
        });
    };
    if (!periodic) // tiled: 2 cells per lane (1, 4 and 6 were measured slower), DPP lane shifts
        march(int_c<2>{}, std::false_type{});
    else
        with_value<1, 2, 4>(C == 1 || C == 2 ? C : 4, [&](auto CC) { march(CC, std::true_type{}); });
    return g.tiles;
}
// the gated azimuthal launch launch_transport(defer_gated) left out -- alone, or with the final boundary call of the step
// on `boundary_view` (the state after the transport's pointer swap) in the same launch (k_theta_march_gated_boundary)
void launch_gated_theta(const GatedTheta &gt, const Dev *boundary_view, hipStream_t st)
{
    const Dev &P = gt.P, &Wm = gt.Wm;
    if (!boundary_view) {
        launch_theta_march(P, Wm, 2, 0, 0, P.shift_jump, st);
        return;
    }
    const ThetaSet inB = {P.rmpB, P.rmmB, P.lpB, P.lmB, P.sigB, P.eB};
    const ThetaGeometry g = theta_geometry(P, 2, 0);
    const int ntheta = g.nvb > FALLBACK_BLOCKS ? FALLBACK_BLOCKS : g.nvb;
    const dim3 grid(ntheta + (boundary_view->nphi + 255) / 256), block(256);
    with_bool(P.adiabatic, [&](auto AA) {
        with_bool(Wm.damp_in_step, [&](auto DD) {
            KLAUNCH(KID_THETA_GATED_BOUNDARY, (k_theta_march_gated_boundary<2, TARG(AA), TARG(DD), false>), grid, block, Wm,
                    (const double *)P.vazi, (const double *)P.vrad, inB, g.tiles, g.rows, g.nvb, ntheta, *boundary_view);
        });
    });
}

// part: TRANSPORT_ALL, or -- for slabs with neighbours, when transport_can_split() -- launch_shift_means, then
// TRANSPORT_INTERIOR on a side stream and TRANSPORT_EDGES (the chunks holding the rings a neighbour receives, rows
// [7,14) and [nr-14,nr-7)) on the caller's stream, so that the ghost exchange runs under the interior chunks.
TransportResult launch_transport(const Dev &P, const Dev &W, hipStream_t st, int part, GatedTheta *defer_gated)
{
    // P: view whose vrad/vazi are the velocities to transport; W: view that receives the new state
    // Transport, TransportEuler.cpp:112-136
    TransportResult res = {0, W.sigma, W.energy, W.vrad, W.vazi, 0, 0};
    // ---- everything in one kernel (tiled rings only; option transport_fused = 0: off) -----------
    // (the fused kernel addresses its grids with 32-bit byte offsets, 4 GiB each)
    const bool fused = P.nphi >= 256 && P.opt.transport_fused != 0 && (long long)(P.nr + 1) * P.nphi < (1ll << 29);
    if (fused) {
        Dev Wm = W; // the marching kernels cannot work in place
        Wm.sigma = W.sigA;
        Wm.energy = W.eA;
        Wm.vrad = P.vrad == W.vrad ? W.vrad_b : W.vrad;
        Wm.vazi = P.vazi == W.vazi ? W.vazi_b : W.vazi;
        if (part == TRANSPORT_ALL)
            launch_shift_means(P, st); // else: the caller queued it ahead of both parts
        const int rows = transport_rows(P, device_cus());
        const int tiles = tiles_of(P.nphi);
        const int chunks = (P.nr + rows - 1) / rows;
        // The azimuthal half of the two-kernel transport is always queued behind the fused kernel (one idle launch) and
        // runs only if a ring pair exceeds the one-lane shift.  The CFL condition's shear limit
        // (cfl.cpp:207-220) bounds |Nshift[i] - Nshift[i-1]| for the velocities it saw, but the source step that
        // follows can change v_phi enough to break it in violent flows (the fuzzer found one: an ideal-gas
        // spreading ring), and the reference shifts by any amount.  FCPT_TRANSPORT_FALLBACK=0 drops the launches
        // for flows known to be benign; a violation is then reported as FCPT_ESHEAR.
        const int fallback = P.opt.transport_fallback != 0;
        TfChunks ch = {chunks, chunks, 0, 1, nullptr};
        const bool sched = part == TRANSPORT_ALL && P.tf_sched_n > 0 && P.opt.transport_rows <= 0;
        if (sched)
            ch = TfChunks{P.tf_sched_n, P.tf_sched_n, 0, 1, P.tf_sched};
        const int c_lo = (P.nr - 2 * FCPT_OVERLAP) / rows;    // first chunk of the outer tail (holds row nr - 14)
        const int lead = (2 * FCPT_OVERLAP + rows - 1) / rows; // chunks that hold rows [0, 14)
        if (part == TRANSPORT_EDGES)
            ch = TfChunks{lead + (chunks - c_lo), lead, c_lo - lead, 1, nullptr};
        else if (part == TRANSPORT_INTERIOR)
            ch = TfChunks{c_lo - lead, 0, lead, 0, nullptr};
        res.split = part != TRANSPORT_ALL;
        // (8 XCDs x the wavefronts of ceil(count / 8) chunks, four to a workgroup: see the chunk mapping in the kernel)
        const dim3 grid(sched ? (ch.count + 3) / 4
                              : (ch.count >= TF_XCD_CHUNKS ? 8 * ((((ch.count + 7) / 8) * tiles + 3) / 4) : (ch.count * tiles + 3) / 4)),
            block(256);
        with_bool(P.adiabatic, [&](auto AA) {
            with_bool(W.damp_in_step, [&](auto DD) {
                with_value<FCPT_LIMITER_MC, FCPT_LIMITER_VANLEER>(P.limiter == FCPT_LIMITER_MC ? FCPT_LIMITER_MC : FCPT_LIMITER_VANLEER, [&](auto LIM) {
                    KLAUNCH(KID_TRANSPORT_FUSED, (k_transport_fused<TARG(AA), TARG(DD), TARG(LIM)>), grid, block, P, Wm, tiles, rows, fallback, ch);
                });
            });
        });
        // behind it, the azimuthal march of the two-kernel form: its blocks return at once unless k_ring_mean met
        // |Nshift[i] - Nshift[i-1]| > 1 (a time step beyond the FARGO shear limit) -- the fused launch then ran the
        // radial sweep.  (Round 2 did both sweeps in this second launch with a hand-rolled grid barrier between them;
        // the flag now being known before the fused launch starts, no barrier is needed.)
        if (fallback && defer_gated && part == TRANSPORT_ALL) { // the caller queues it with the final boundary call (launch_gated_theta)
            defer_gated->P = P;
            defer_gated->Wm = Wm;
            res.gated_pending = 1;
        } else if (fallback) {
            launch_theta_march(P, Wm, 2, 0, 0, P.shift_jump, st);
        }
        res.marched = tiles;
        res.sigma = Wm.sigma, res.energy = Wm.energy, res.vrad = Wm.vrad, res.vazi = Wm.vazi;
        return res;
    }
    { // radial sweep + ring means (two independent kernels of the reference's sequence) as one launch
        const int rows = march_len(P, device_cus(), RADIAL_ROWS);
        const Launch2D l = launch2d((P.nr + rows - 1) / rows, P.nphi);
        const int gx = (int)l.grid.x, gy = (int)l.grid.y;
        const dim3 grid(gx * gy + (P.nr + 3) / 4);
        const double *part = P.src_ring_nparts ? (const double *)P.ring_part : (const double *)nullptr;
        with_bool(l.block.x >= 64, [&](auto ROWU) {
            KLAUNCH(KID_TRANSPORT_RADIAL_MEANS, k_transport_radial_means<TARG(ROWU)>, grid, l.block, P, gx, gy, rows, part, P.src_ring_nparts, P.ring_pstride);
        });
    }
    ThetaSet inB = {P.rmpB, P.rmmB, P.lpB, P.lmB, P.sigB, P.eB};
    ThetaOut outA = {P.rmpA, P.rmmA, P.lpA, P.lmA, P.sigA, P.eA};
    ThetaSet inA = {P.rmpA, P.rmmA, P.lpA, P.lmA, P.sigA, P.eA};
    ThetaOut outB = {P.rmpB, P.rmmB, P.lpB, P.lmB, P.sigB, P.eB};
    // ring-marching azimuthal kernel when a lane-chunk size fits the ring, else (and with FCPT_THETA_MARCH=0) the
    // per-pass kernels
    int C = 0, periodic = 0;
    for (int c : {1, 2, 4})
        if (!C && P.nphi % c == 0 && P.nphi <= 64 * c && (c == 1 || P.nphi / c >= 1)) {
            C = c;
            periodic = 1;
        }
    if (!C && P.nphi > 64 * 2)
        C = 2;
    const bool march = C != 0 && P.opt.theta_march != 0;
    if (march) {
        // the kernel reads the pre-transport v_phi and v_r of a ring (halo columns included) while other
        // wavefronts already store the new ones: never in place (the source step leaves its result in the *_b twins)
        Dev Wm = W;
        Wm.vrad = P.vrad == W.vrad ? W.vrad_b : W.vrad;
        Wm.vazi = P.vazi == W.vazi ? W.vazi_b : W.vazi;
        res.marched = launch_theta_march(P, Wm, C, periodic, 1, nullptr, st);
        res.vrad = Wm.vrad, res.vazi = Wm.vazi;
    } else {
        LAUNCH2D_T(KID_THETA1, k_transport_theta, 1, P.nr, P, inB, outA);
        LAUNCH2D_T(KID_THETA2, k_transport_theta, 2, P.nr, P, inA, outB);
        if (W.damp_in_step)
            LAUNCH2D_T(KID_VELOCITIES, k_velocities, true, P.nr, W, inB, (const double *)P.vrad);
        else
            LAUNCH2D_T(KID_VELOCITIES, k_velocities, false, P.nr, W, inB, (const double *)P.vrad);
    }
    return res;
}

void launch_derived(const Dev &P, hipStream_t st)
{
    // recalculate_derived_disk_quantities, SourceEuler.cpp:225-249 (AspectRatioMode 0)
    if (P.adiabatic) {
        LAUNCH2D(KID_ADI_CS_H, k_adi_derived, P.nr, P, 3); // T, c_s, H, P, nu
    } else {
        LAUNCH2D(KID_PRESSURE, k_pressure, P.nr, P);
    }
}

void launch_pressure(const Dev &P, hipStream_t st) { LAUNCH2D(KID_PRESSURE, k_pressure, P.nr, P); }
void launch_temperature(const Dev &P, hipStream_t st) { LAUNCH2D(KID_TEMPERATURE, k_temperature, P.nr, P); }

static dim3 disk_on_body_grid(const Dev &P)
{
    const int nrows = P.active_size - P.first_active;
    return dim3((P.nphi + 255) / 256, nrows > 0 ? (nrows + DOB_ROWS - 1) / DOB_ROWS : 1);
}
void launch_disk_on_body(const Dev &P, double x, double y, double r_object, double smoothing_fixed, double r_sm, double *out,
                         hipStream_t st)
{
    const dim3 grid = disk_on_body_grid(P), block(256);
    KLAUNCH(KID_DISK_ON_BODY, k_disk_on_body, grid, block, P, x, y, r_object, smoothing_fixed, r_sm, P.cfl_part);
    KLAUNCH(KID_DISK_ON_BODY, k_disk_on_body_final, dim3(1), dim3(256), (const double *)P.cfl_part, (int)(grid.x * grid.y), out);
}
size_t disk_on_bodies_blocks(const Dev &P)
{
    const dim3 grid = disk_on_body_grid(P);
    return (size_t)grid.x * grid.y;
}
void launch_disk_on_bodies(const Dev &P, int n, const DiskBodies &B, double *part, double *out, hipStream_t st)
{
    if (n < 1 || n > FCPT_MAX_BODIES)
        return;
    const dim3 grid = disk_on_body_grid(P), block(256); // the grid of launch_disk_on_body: the same reduction tree
    int need_h = 0;
    for (int b = 0; b < n; ++b)
        need_h |= B.smoothing_fixed[b] < 0.0;
    static_assert(FCPT_MAX_BODIES == 8, "one instance of k_disk_on_bodies per body count");
    with_value<1, 2, 3, 4, 5, 6, 7, 8>(n, [&](auto N) { KLAUNCH(KID_DISK_ON_BODIES, k_disk_on_bodies<TARG(N)>, grid, block, P, B, need_h, part); });
    KLAUNCH(KID_DISK_ON_BODIES, k_disk_on_bodies_final, dim3(n), dim3(256), (const double *)part, (int)(grid.x * grid.y), out);
}

// one lane per particle slot (dead slots return at once); the view's state grids are those of the start of the step
// slab: the context is one of several slabs (fcpt_particles_slabs), in either form: host arguments (fcpt_particles_step) or
// the device clock (fcpt_run_steps on several slabs)
void launch_particles(const Dev &P, const ParticleArgs &A, hipStream_t st, bool slab)
{
    if (A.n <= 0)
        return;
    const dim3 grid((A.n + 255) / 256), block(256);
    with_bool(P.adiabatic, [&](auto ADI) {
        with_bool(A.gas_drag != 0, [&](auto DRAG) {
            with_bool(A.diffusion != 0, [&](auto DIFF) {
                with_bool(A.step_offset != nullptr, [&](auto DEV) { // (fcpt_run_steps: per-step scalars from the device clock)
                    with_bool(slab, [&](auto SLAB) {
                        KLAUNCH(KID_PARTICLES, (k_particles_step<TARG(ADI), TARG(DRAG), TARG(DIFF), TARG(DEV), TARG(SLAB)>), grid,
                                block, P, A);
                    });
                });
            });
        });
    });
}

// ParticleIntegrator: explicit -- one lane per particle slot, one launch; the block size stands beside the kernel
void launch_particles_explicit(const Dev &P, const ParticleArgs &A, const ParticleAdaptive &X, bool cartesian, hipStream_t st,
                               bool slab)
{
    if (A.n <= 0)
        return;
    const dim3 grid((A.n + PARTICLES_EXPLICIT_BLOCK - 1) / PARTICLES_EXPLICIT_BLOCK), block(PARTICLES_EXPLICIT_BLOCK);
    with_bool(P.adiabatic, [&](auto ADI) {
        with_bool(A.gas_drag != 0, [&](auto DRAG) {
            with_bool(cartesian, [&](auto CART) {
                with_bool(A.step_offset != nullptr, [&](auto DEV) {
                    with_bool(slab, [&](auto SLAB) {
                        KLAUNCH(KID_PARTICLES_EXPLICIT,
                                (k_particles_step_explicit<TARG(ADI), TARG(DRAG), TARG(CART), TARG(DEV), TARG(SLAB)>), grid, block, P, A,
                                X);
                    });
                });
            });
        });
    });
}
void launch_particles_timestep_init(const Dev &P, const ParticleArgs &A, const ParticleAdaptive &X, bool cartesian, hipStream_t st)
{
    if (A.n <= 0)
        return;
    const dim3 grid((A.n + PARTICLES_EXPLICIT_BLOCK - 1) / PARTICLES_EXPLICIT_BLOCK), block(PARTICLES_EXPLICIT_BLOCK);
    with_bool(cartesian, [&](auto CART) { hipLaunchKernelGGL(k_particles_timestep_init<TARG(CART)>, grid, block, 0, st, P, A, X); });
}

void launch_particles_normals(int n, const unsigned long long *id, unsigned long long seed, unsigned long long step, double *snv,
                              hipStream_t st)
{
    if (n > 0)
        hipLaunchKernelGGL(k_particles_normals, dim3((n + 255) / 256), dim3(256), 0, st, n, id, seed, step, snv);
}
// once per fcpt_run_steps, ahead of its first step and outside any captured graph: *offset + clk->n_hydro_iter is then the
// Philox counter of every particle launch of the call
void launch_particles_counter_offset(unsigned long long *offset, unsigned long long counter, const DevClock *clk, hipStream_t st)
{
    hipLaunchKernelGGL(k_particles_counter_offset, dim3(1), dim3(1), 0, st, offset, counter, clk);
}

// fcpt_particles_slabs: the slots in at most PARTICLE_MIGRATE_GROUPS equal stretches of whole workgroup passes, counted,
// summed by one workgroup and placed; the receiver's grid covers the capacity of a side
void launch_particles_emigrate(const ParticleArgs &A, const ParticleAdaptive &X, const ParticleMigrate &M0, hipStream_t st)
{
    if (A.n <= 0)
        return;
    ParticleMigrate M = M0;
    const int passes = ((A.n + 255) / 256 + PARTICLE_MIGRATE_GROUPS - 1) / PARTICLE_MIGRATE_GROUPS;
    M.chunk = 256 * passes;
    M.groups = (A.n + M.chunk - 1) / M.chunk;
    KLAUNCH(KID_PARTICLES_EMIGRATE_COUNT, k_particles_emigrate_count, dim3(M.groups), dim3(256), A, M);
    KLAUNCH(KID_PARTICLES_EMIGRATE_FINISH, k_particles_emigrate_finish, dim3(1), dim3(256), M);
    KLAUNCH(KID_PARTICLES_EMIGRATE, k_particles_emigrate, dim3(M.groups), dim3(256), A, X, M);
}
void launch_particles_immigrate(const ParticleArgs &A, const ParticleAdaptive &X, const ParticleMigrate &M, hipStream_t st)
{
    if (A.n <= 0 || M.capacity <= 0)
        return;
    KLAUNCH(KID_PARTICLES_IMMIGRATE, k_particles_immigrate, dim3((M.capacity + 255) / 256, 2), dim3(256), A, X, M);
}

// rings whose CFL terms read nothing the ghost exchange or the boundary kernels write: ring i reads rows i
// (and i+1 of v_r); fcpt_exchange_unpack writes rows [0,7) and [nr-7,nr)
#define CFL_EDGE_LO (FCPT_OVERLAP + 1)
#define CFL_EDGE_HI (FCPT_OVERLAP + 2)
// rings of 2049 .. 4096 cells: 512 threads with four cell pairs each and ALL their loads ahead of the ring sum, instead
// of 256 with eight.  Isothermal (two grids): 22.7-23.6 us at 2048 x 4096, the step 0.3187 ms, against 37 us for the
// 256-thread form and 23.8-25.6 us / 0.3197 ms for 1024 threads with two pairs each (three A/B pairs,
// profiles/r03_ab_cfl_threads.txt, r03_ab_cfl_512.txt).  Ideal EOS (five grids): 62-65 us against 56 for the 256-thread
// form, which it keeps (profiles/r03_ab_cfl_hoist.txt).
// cfl_wide_blocks: -1 = built-in (isothermal 512 threads, ideal EOS 256), 0 = 256, any other value = 512
static bool cfl_wide_blocks(const Dev &P)
{
    return P.opt.cfl_wide_blocks < 0 ? !P.adiabatic : P.opt.cfl_wide_blocks != 0;
}
// the instance of k_cfl_rings / k_cfl_rings_bc for this grid: f(ideal EOS, cell pairs per thread, threads)
template <class F> static void with_cfl_ring_shape(const Dev &P, F &&f)
{
    const bool wide = P.nphi > 512 * CFL_MAXP;
    with_bool(P.adiabatic, [&](auto ADI) {
        if (!wide && P.nphi > 2048 && cfl_wide_blocks(P)) // 512 threads with four cell pairs each
            f(ADI, int_c<CFL_MAXP / 2>{}, int_c<512>{});
        else if (wide)
            f(ADI, int_c<2 * CFL_MAXP>{}, int_c<256>{});
        else
            f(ADI, int_c<CFL_MAXP>{}, int_c<256>{});
    });
}
static void launch_cfl_rings(const Dev &P, int r1, int n1, int r2, int n2, hipStream_t st)
{
    if (n1 + n2 <= 0)
        return;
    with_cfl_ring_shape(P, [&](auto ADI, auto MAXP, auto NT) {
        KLAUNCH(KID_CFL_RINGS, (k_cfl_rings<TARG(ADI), TARG(MAXP), TARG(NT)>), dim3(n1 + n2), dim3(TARG(NT)), P, P.cfl_part, r1, n1, r2);
    });
}
// launch_cfl with the final boundary call of the previous step inside the ring launch (see k_cfl_rings_bc); the caller
// has checked cfl_bc_mergeable() (fcpt_plan.cpp)
// k_cfl_final folds `nparts` partial maxima
static void launch_cfl_fold(const Dev &P, int nparts, int apply_policy, hipStream_t st)
{
    KLAUNCH(KID_CFL_INIT, k_cfl_final, dim3(1), dim3(1024), P, (const double *)P.cfl_part, nparts, apply_policy);
}
void launch_cfl_bc(const Dev &P, int apply_policy, hipStream_t st)
{
    with_cfl_ring_shape(P, [&](auto ADI, auto MAXP, auto NT) {
        const int nbc = (P.nphi + TARG(NT) - 1) / TARG(NT); // workgroups of the boundary call, ahead of one per ring
        KLAUNCH(KID_CFL_RINGS_BC, (k_cfl_rings_bc<TARG(ADI), TARG(MAXP), TARG(NT)>), dim3(nbc + P.nr), dim3(TARG(NT)), P, P.cfl_part, nbc);
    });
    if (apply_policy != 2)
        launch_cfl_final(P, apply_policy, st);
}
// the fold a launch_cfl / launch_cfl_bc with apply_policy = 2 left out, for a caller whose marching source kernel did not run after all
void launch_cfl_final(const Dev &P, int apply_policy, hipStream_t st) { launch_cfl_fold(P, P.nr, apply_policy, st); }
// phase 1 of a split CFL: the interior rings only (returns false when the one-block-per-ring kernel does not apply)
bool launch_cfl_interior(const Dev &P, hipStream_t st)
{
    if (!cfl_by_rings(P) || P.nr <= CFL_EDGE_LO + CFL_EDGE_HI)
        return false;
    launch_cfl_rings(P, CFL_EDGE_LO, P.nr - CFL_EDGE_LO - CFL_EDGE_HI, 0, 0, st);
    return true;
}
void launch_cfl(const Dev &P, int apply_policy, hipStream_t st, bool interior_done)
{
    if (cfl_by_rings(P)) {
        // (the final fold as its own small launch.  Letting the last workgroup of k_cfl_rings do it, with one
        // agent-scope release per workgroup, was measured at 110 instead of 36 + 6 us: on this GPU a device-scope
        // release writes the XCD's L2 back, 2048 times per launch.)
        if (interior_done)
            launch_cfl_rings(P, 0, CFL_EDGE_LO, P.nr - CFL_EDGE_HI, CFL_EDGE_HI, st);
        else
            launch_cfl_rings(P, 0, P.nr, 0, 0, st);
        if (apply_policy != 2) // (2: the marching source kernel queued next folds for itself)
            launch_cfl_final(P, apply_policy, st);
        return;
    }
    KLAUNCH(KID_RING_MEAN, k_ring_mean, dim3((P.nr + 3) / 4), dim3(256), P, 0, (const double *)nullptr, 0, P.ring_pstride);
    const int nrows = P.active_size - P.first_active;
    int nparts = 0;
    if (nrows > 0) {
        const int rows = march_len(P, device_cus(), CFL_ROWS);
        const Launch2D l = launch2d((nrows + rows - 1) / rows, P.nphi);
        nparts = (int)(l.grid.x * l.grid.y);
        with_bool(l.block.x >= 64, [&](auto ROWU) { KLAUNCH(KID_CFL_CELLS, k_cfl_cells<TARG(ROWU)>, l.grid, l.block, P, P.cfl_part, rows); });
    }
    launch_cfl_fold(P, nparts, apply_policy, st);
}

void launch_clock_export_cfl(DevClock *clk, double *out, hipStream_t st)
{
    KLAUNCH(KID_CLOCK, k_clock_export_cfl, dim3(1), dim3(1), (const DevClock *)clk, out);
}
void launch_clock_policy_ptr(DevClock *clk, double cfl_max_var, const double *cfl_global, hipStream_t st)
{
    KLAUNCH(KID_CLOCK, k_clock_policy_ptr, dim3(1), dim3(1), clk, cfl_max_var, cfl_global);
}
void launch_clock_scale_dt(DevClock *clk, int mode, double dt, double factor, hipStream_t st)
{
    KLAUNCH(KID_CLOCK, k_clock_scale_dt, dim3(1), dim3(1), clk, mode, dt, factor);
}
void launch_clock_set_dt(DevClock *clk, double dt, hipStream_t st)
{
    KLAUNCH(KID_CLOCK, k_clock_set_dt, dim3(1), dim3(1), clk, dt);
}
void launch_clock_advance(DevClock *clk, hipStream_t st)
{
    KLAUNCH(KID_CLOCK, k_clock_advance, dim3(1), dim3(1), clk);
}
void launch_clock_policy(DevClock *clk, double cfl_max_var, int use_device_cfl, double cfl_global,
                         hipStream_t st)
{
    KLAUNCH(KID_CLOCK, k_clock_policy, dim3(1), dim3(1), clk, cfl_max_var, use_device_cfl, cfl_global);
}
