// Part of fcpt_kernels.hip (one translation unit, namespace fcpt): k_transport_fused: the whole Transport() in one marching kernel.
// Not a stand-alone header: included once, in the order given there.

// ===========================================================================
// The whole Transport() (TransportEuler.cpp:112-136) in ONE pass over memory.
//
// A wavefront owns 64 consecutive phi columns (one per lane) in PRE-shift coordinates and marches outward
// ring by ring.  Per step it loads one ring of Sigma, v_r, v_phi(, e) (the only HBM reads), and
//   R  radial sweep: specific momenta w(m), limited half slopes of ring m-1, the upwind fluxes
//      through interface m-1 (each evaluated once, shared mass flux), update of ring m-2
//      (compute_momenta_from_velocities + OneWindRad, :138-167,471-493,545-620) -- all column-local,
//      a rolling register window of three rings;
//   T  both azimuthal passes on ring m-2 (theta_pass, as k_transport_theta_march) with phi
//      neighbours by DPP lane shifts;
//   V  velocities from momenta, floors, wave damping (:498-535,121-131) and the store of the new
//      state at the POST-shift address (column + Nshift[i], AdvectSHIFT :238-268 is free).
// v_r(i) couples rings i-1 and i at one post-shift column, i.e. at lanes that differ by
// Nshift[i] - Nshift[i-1].  The FARGO shear limit of the CFL condition (cfl.cpp:207-220) keeps
// that difference in {-1, 0, 1} for every admissible dt, so one lane shift of the previous ring
// is enough; k_ring_mean raises P.shift_jump otherwise and this launch does the radial sweep of the
// two-kernel transport instead (see there).
// Nothing intermediate reaches memory: 3 (4) grids read + 3 (4) written instead of 8 + 9
// (10 + 11) doubles per cell for k_transport_radial + k_transport_theta_march.
// Validity in cells of a 64-column segment: right 1 (L+ needs v_phi(j+1)), 4 at either end for the
// two passes, left 1 for L+(j-1), 1 at either end for the v_r lane shift.
// The chunks of one launch: `count` of them, the first `lead` are chunks 0..lead-1 of the grid, the others follow
// `skip` chunks further up.  All chunks at once: {n, n, 0, 1}.  Slabs with neighbours march the chunks that hold
// the rings the neighbours are waiting for first (fcpt_step_device_begin): {1 + tail, 1, gap, 1} then {gap, 0, 1, 0}.
// sched != null: wavefront w of the launch (blockIdx.x * 4 + its index in the workgroup) marches tile sched[4w] over rings
// [sched[4w+1], sched[4w+2]) -- transport_schedule() in fcpt_schedule.cpp; count = entries, lead / skip do not apply.
#include "../fcpt_schedule.h" // TF_XCD_CHUNKS, TF_HALO_LO, TF_HALO_HI, TF_STRIDE, shared with the chunk planner
struct TfChunks {
    int count, lead, skip, advance_clock;
    const int *sched;
};

// wave damping with the ring's precomputed exp(-dt f / tau) (k_ring_mean): types as damp_value, X0 the reference value
// of the cell.  The types are wave-uniform and only select: no branch, so that the loads of a ring's reference values
// and all their uses stay in one basic block (see the damped form of new_state in transport_fused_body).
__device__ __forceinline__ double damp_select(double X, int type, double ef, double X0, double zero_target)
{
    const double target = type == 1 ? X0 : zero_target;
    const double damped = (X - target) * ef + target;
    return type != 0 ? damped : X;
}

template <bool ADI, bool DAMP, int LIM>
__device__ __forceinline__ void transport_fused_body(const Dev &P, const Dev &W, int tiles, int rows, int has_fallback,
                                                     const TfChunks &ch)
{
    // P: view whose vrad/vazi are the velocities to transport; W: view that receives the new state
    constexpr int LO = TF_HALO_LO, HI = TF_HALO_HI;
    constexpr int NQ = ADI ? 6 : 5; // s, rmp, rmm, lp, lm(, e)
    constexpr int lim = LIM;
    // Register diet of the ideal-EOS instantiation (156 -> 128 VGPRs = 4 instead of 3 wavefronts per SIMD): the raw
    // energy, the raw v_phi and the slope differences of the previous ring are re-derived from the specific
    // quantities of the rolling window instead of being carried along (ulp-level differences: e = (e / Sigma) Sigma,
    // v_phi = ((v_phi + r Omega) r) / r - r Omega)
    constexpr bool DIET = ADI;
    // PIN: the prefetch of ring m+2 is pinned behind convert() of ring m+1 (bottom of the loop).  -1.8 % per step for
    // the ideal EOS when it was introduced; the isothermal kernel gained nothing then (its time was set by the tail of
    // slow wavefronts) and 1.9 % once the chunks were dealt slow ones first (four A/B pairs each).
    // DVP: v_phi re-derived from (v_phi + r Omega) r instead of carried: a carried copy would share the prefetch registers.
    constexpr bool PIN = true, DVP = true;
    const int lane = threadIdx.x & 63;
    // Chunks are dealt to the 8 XCDs round-robin (workgroup b runs on XCD b % 8; all tiles of a chunk on one XCD, whose
    // L2 then serves their shared halo columns), in an order that starts at both ends of the slab and works inward:
    // the rings of the damping zones cost more (three more loads per cell; ~1.5x while each was waited for on the spot:
    // the figure of the measurements quoted here), and with the chunks in radial order on contiguous XCD ranges the
    // outer zone's wavefronts started last, on one XCD, and ran on alone (2.98 of 4 wavefronts per SIMD on average; -5.5 % kernel time, -3 % / -4.6 % per step, three A/B pairs).
    // (launches of fewer than TF_XCD_CHUNKS chunks -- short slabs -- deal workgroups instead: every XCD gets work)
    if (ch.advance_clock && blockIdx.x == 0 && threadIdx.x == 0) { // sim::time += dt; N_hydro_iter++ (simulation.cpp:226-227)
        clock_advance(W.clk, P.clk->dt);
    }
    // k_ring_mean found a ring pair beyond the one-lane shift (a dt beyond the FARGO shear limit, or a source step that
    // changed v_phi violently): this launch runs the radial sweep of the two-kernel transport instead -- all of its
    // workgroups, with a grid stride -- and the gated azimuthal launch queued behind it finishes the step.
    if (shift_jump_raised(P.shift_jump)) {
        if (has_fallback) {
            const int gx = (P.nphi + 255) / 256, gy = (P.nr + RADIAL_ROWS - 1) / RADIAL_ROWS; // launch2d() of Nphi >= 256
            for (int vb = blockIdx.x; vb < gx * gy; vb += gridDim.x)
                transport_radial_block<true>(P, vb, gx, gx * gy, RADIAL_ROWS);
        } else if (blockIdx.x == 0 && threadIdx.x == 0) {
            W.clk->shear_error = 1; // nothing behind this kernel will redo the step: report it
        }
        return;
    }
    const int nr = P.nr, nphi = P.nphi;
    int tile, r0, r1, trace_slot;
    if (ch.sched) { // (tile, first ring, one past the last) of every wavefront in the order of dispatch: transport_schedule()
        const int wave = __builtin_amdgcn_readfirstlane(blockIdx.x * MARCH_WAVES + (threadIdx.x >> 6));
        if (wave >= ch.count)
            return;
        const int __attribute__((address_space(4))) *e = (const int __attribute__((address_space(4))) *)ch.sched + 4 * wave;
        tile = e[0], r0 = e[1], r1 = e[2];
        trace_slot = wave;
        if (r0 >= r1)
            return;
    } else {
        int chunk_l, wave;
        if (ch.count >= TF_XCD_CHUNKS) {
            const int xcd = blockIdx.x & 7, wq = (blockIdx.x >> 3) * MARCH_WAVES + (threadIdx.x >> 6);
            const int zq = __builtin_amdgcn_readfirstlane(wq / tiles);
            chunk_l = xcd + 8 * zq; // chunk within this launch
            wave = __builtin_amdgcn_readfirstlane(chunk_l * tiles + (wq - zq * tiles));
        } else {
            wave = __builtin_amdgcn_readfirstlane(blockIdx.x * MARCH_WAVES + (threadIdx.x >> 6));
            chunk_l = wave / tiles;
        }
        if (chunk_l >= ch.count)
            return;
        int chunk = chunk_l < ch.lead ? chunk_l : chunk_l + ch.skip;
        if (ch.lead == ch.count && ch.skip == 0) // all chunks in one launch: 0, n-1, 1, n-2, ...
            chunk = (chunk_l & 1) ? ch.count - 1 - (chunk_l >> 1) : (chunk_l >> 1);
        r0 = chunk * rows, r1 = r0 + rows < nr ? r0 + rows : nr;
        if (r0 >= nr)
            return;
        tile = wave - chunk_l * tiles;
        trace_slot = chunk * tiles + tile;
    }
    (void)trace_slot;
#ifdef TF_TRACE /* profiles/tools/wave_trace_transport.py: start and end of every wavefront, 10 ns ticks, in the temperature grid (which no marching kernel touches) */
    if (lane == 0) {
        W.temperature[4 * trace_slot] = (double)wall_clock64();
        W.temperature[4 * trace_slot + 2] = (double)r0;
        W.temperature[4 * trace_slot + 3] = (double)r1;
    }
#endif
    const int a = tile * TF_STRIDE - LO; // first pre-shift column of the segment
    const double dt = P.clk->dt;
    auto wrap = [nphi](int j) { return j < 0 ? j + nphi : (j >= nphi ? j - nphi : j); };

    const int jin = wrap(a + lane); // this lane's pre-shift column
    const bool valid = lane >= LO && lane < 64 - HI && a + lane < nphi;

    // rolling window: index 0 = ring m (newest), 1 = m-1, 2 = m-2
    double w[3][NQ];  // specific quantities: Sigma, v_r(ring+1), v_r(ring), (v_phi(j+1) + r Omega) r, (v_phi + r Omega) r(, e / Sigma)
    double er[3];     // the energy itself (!DIET)
    double vp[3];     // v_phi as loaded (!DVP)
    double d1[NQ];    // (w(m-1) - w(m-2)) InvDiffRmed[m-1] (!DIET; not of slot 3, whose slope comes from the next lane)
    double idr_prev = 0.0; // DIET: InvDiffRmed[m-1], to re-form d1
    double hs1[NQ];   // limited half slope of ring m-2
    double F1[NQ];    // flux through interface m-2
    double rmp_prev = 0.0, S_prev = 0.0; // transported rm+ and Sigma of the previous ring
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        w[0][q] = w[1][q] = w[2][q] = hs1[q] = F1[q] = 0.0;
        if (!DIET)
            d1[q] = 0.0;
    }
    if (!DIET)
        er[0] = er[1] = er[2] = 0.0;
    if (!DVP)
        vp[0] = vp[1] = vp[2] = 0.0;
    // raw loads of one ring: Sigma(k), v_phi(k)(, e(k)) and v_r(k+1); zeros outside the grid
    struct RingRaw {
        double sg, va, en, vr;
    };
    auto fetch = [&](int k, RingRaw &o) {
        const bool in_k = k >= 0 && k < nr;
        const bool in_v = k + 1 >= 0 && k + 1 <= nr;
        o.sg = o.va = o.en = o.vr = 0.0;
        const unsigned row = (unsigned)(in_k ? k : 0) * (unsigned)nphi, rowv = (unsigned)(in_v ? k + 1 : 0) * (unsigned)nphi;
        if (in_k) {
            const unsigned ob = (row + (unsigned)jin) * 8u;
            o.sg = ld_off(P.sigma, ob);
            o.va = ld_off(P.vazi, ob);
            if (ADI)
                o.en = ld_off(P.energy, ob);
        }
        if (in_v)
            o.vr = ld_off(P.vrad, (rowv + (unsigned)jin) * 8u);
    };
    // ring k (raw) -> newest window slot; vr_k = v_r(k) from the previous ring's fetch
    double vr_last;
    // (r, romega: Rmed[k] and Rmed[k] OmegaFrame, from the caller's batch of per-ring scalars)
    auto convert = [&](int k, const RingRaw &o, double r, double romega) {
        const bool in_k = k >= 0 && k < nr;
        w[0][0] = o.sg;
        w[0][1] = in_k ? o.vr : 0.0;                        // rm+ / Sigma = v_r(k+1)   (:484-485)
        w[0][2] = in_k ? vr_last : 0.0;                     // rm- / Sigma = v_r(k)
        w[0][4] = in_k ? (o.va + romega) * r : 0.0;         // L- / Sigma
        w[0][3] = lane_next(w[0][4]);                       // L+ / Sigma = (v_phi(j+1) + r Omega) r: L- / Sigma of cell j+1
        if (ADI) {
            w[0][NQ - 1] = in_k ? o.en * FAST_RCP_TR(o.sg) : 0.0;
            if (!DIET)
                er[0] = o.en;
        }
        if (!DVP)
            vp[0] = o.va;
        vr_last = o.vr;
    };
    // Software pipeline of the memory traffic: ring m+1 is in flight while ring m-2 is computed;
    // at the bottom of an iteration the arrived ring is converted, the loads of ring m+2 are
    // issued, and only then the iteration's stores.  The one s_waitcnt vmcnt(0) per iteration then
    // meets operations that are a whole compute phase old (vmcnt counts stores too; waiting right
    // behind them costs a round trip per ring at 2-3 waves per SIMD).
    // (the three rings that start a chunk are requested together: one memory round trip before the loop, not two)
    RingRaw nxt;
    {
        RingRaw first, second;
        fetch(r0 - 4, first);
        fetch(r0 - 3, second);
        fetch(r0 - 2, nxt);
        vr_last = first.vr; // v_r(r0-3)
        const ThetaRow t3 = crow_load(P.theta_tab, r0 - 3 >= 0 ? r0 - 3 : 0);
        convert(r0 - 3, second, t3.rmed, t3.r_omega);
    }
    // The per-ring scalars of an iteration are two packed rows at index m + 3 of two tables: TfRow, what no step changes
    // (interface k, ring i and the ring m+1 that the bottom of the iteration converts; rows outside the grid hold what a
    // clamped index would fetch), and ShiftRow of ring i, which k_ring_mean completes with every product of the ring's
    // scalars and dt -- the loop clamps no index, forms no wave-uniform product and advances two pointers.
    const TfRow *trow = P.tf_tab + (r0 - 3 + 3);
    const ShiftRow *srow = (const ShiftRow *)P.shift_tab + (r0 - 3 - 2);

    for (int m = r0 - 3; m <= r1 + 1; ++m) {
        // ---- per-ring scalars of this iteration in one batch ----------------------------------
        const int k = m - 1, i = m - 2;
        const bool do_i = i >= r0 - 1 && i >= 0 && i < r1;
        const TfRow tr = crow_load(trow, 0);
        const ShiftRow si = crow_load(srow, 0);
        ++trow, ++srow;        const double r_next = tr.r_next, romega_next = tr.romega_next; // ring m+1
        // ---- R: slopes of ring m-1, fluxes through interface k = m-1 --------------------------
        // (the first iterations of a chunk only fill the window: the first slope that reaches a result is that of ring
        //  r0-2 -- as hs1 of the flux through interface r0-1 -- formed at m = r0-1 from the differences of rings r0-3 ..
        //  r0-1; the kernels that carry the previous difference instead of re-forming it need it from m = r0-2)
        double F0[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            F0[q] = 0.0;
        if (m >= r0 - (DIET ? 1 : 2)) {
            const double idr_m = tr.idr_up;          // 1 / (Rmed[m] - Rmed[m-1]) when both rings exist
            const bool lim_ok = k > 0 && k < nr - 1; // boundary rings carry no slope (:360-372)
            const bool open = k > 0 && k < nr;       // interface carries a flux
            const double g = si.g_up; // dt dphi Rinf[k]: the interface above ring i
            const double v = w[1][2]; // v_r(m-1)
            const bool up = v > 0.0;
            const double dist = up ? (tr.dr_lo - v * dt) : -(tr.dr_hi + v * dt);
            double Fc;
            double hs0[NQ]; // limited half slopes of ring m-1
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                if (q == 3)
                    continue;
                const double d0 = (w[0][q] - w[1][q]) * idr_m;
                const double dprev = DIET ? (w[1][q] - w[2][q]) * idr_prev : d1[q];
                hs0[q] = lim_ok ? half_limiter(lim, d0, dprev) : 0.0;
                if (!DIET)
                    d1[q] = d0;
            }
            // Slot 3 of a lane is slot 4 of the lane to its right in all three rings of the window, bit for bit
            // (convert()), and so are its differences and its limited slope: one lane shift instead of a second
            // half_limiter (lane 63, which has no right-hand lane, is halo: "right 1" above)
            hs0[3] = lane_next(hs0[4]);
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                // (both candidates with the lane's own distance, then one select: see theta_star)
                const double st_up = w[2][q] + dist * hs1[q], st_dn = w[1][q] + dist * hs0[q];
                const double st = up ? st_up : st_dn;
                if (q == 0) {
                    Fc = open ? g * st * w[1][2] : 0.0; // mass flux g rho* v
                    F0[q] = Fc;
                } else {
                    F0[q] = st * Fc;
                }
                hs1[q] = hs0[q];
            }
        }
        // ---- update of ring i = m-2, azimuthal passes, velocities -----------------------------
        bool out_on = false;
        unsigned out_g = 0; // byte offset of the cell this lane stores
        double o_vr = 0.0, o_va = 0.0, o_s = 0.0, o_e = 0.0;
        if (do_i) {
            const double invsurf = tr.invsurf;
            double S[1], Q[4][1], E[1], V[1]; // (theta_pass works on the cells of a lane: one here)
            const double mean = si.mean;
            const double vconst = si.vconst;
            const double vadd = P.fast_transport ? 0.0 : vconst;
            {
                const double s0 = w[2][0];
                S[0] = s0 + (F1[0] - F0[0]) * invsurf;
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    Q[q][0] = s0 * w[2][q + 1] + (F1[q + 1] - F0[q + 1]) * invsurf;
                E[0] = ADI ? (DIET ? s0 * w[2][NQ - 1] : er[2]) + (F1[NQ - 1] - F0[NQ - 1]) * invsurf : 0.0;
                V[0] = vadd + ((DVP ? w[2][4] * tr.invr - tr.r_omega : vp[2]) - mean);
            }
            const double dxtheta = tr.dxtheta;
            const double invdx = tr.inv_dxtheta;
            const double geo_dt = si.geo_dt;
            theta_pass<1, ADI, false, 0>(lim, 0, 0, geo_dt, dxtheta, invdx, dt, V, 0.0, S, Q, E);
            if (P.fast_transport) { // (the ring's one velocity: direction, distance factor and flux factor come with the row)
                if (si.up2)
                    theta_pass<1, ADI, false, 1, true>(lim, 0, 0, geo_dt, dxtheta, invdx, dt, V, vconst, S, Q, E, si.d2u, si.gvu);
                else
                    theta_pass<1, ADI, false, 2, true>(lim, 0, 0, geo_dt, dxtheta, invdx, dt, V, vconst, S, Q, E, si.d2u, si.gvu);
            }
            const int ns = si.ns; // Nshift[i] modulo Nphi, in [0, Nphi)
            if (i >= r0) {
                // the previous ring sits Nshift[i] - Nshift[i-1] lanes further right (folded to -1, 0, 1 by k_ring_mean)
                const int dsh = si.dsh;
                double rp, sp;
                if (dsh == 0) {
                    rp = rmp_prev, sp = S_prev;
                } else if (dsh > 0) {
                    rp = lane_next(rmp_prev), sp = lane_next(S_prev);
                } else {
                    rp = lane_prev(rmp_prev), sp = lane_prev(S_prev);
                }
                const double lpm = lane_prev(Q[2][0]); // L+ and Sigma of cell j-1
                const double sm = lane_prev(S[0]);
                const double invr = tr.invr, romega = tr.r_omega;
                const unsigned row = (unsigned)i * (unsigned)nphi;
                int jo = jin + ns;
                const int jout = jo >= nphi ? jo - nphi : jo;
                const unsigned g = (row + (unsigned)jout) * 8u;
                // Velocities from momenta, floors, wave damping.  A ring of the damping zones -- any quantity of a type
                // other than 0 -- requests the reference values of all its quantities at once, ahead of the
                // reciprocals, and uses them behind: one memory round trip under the arithmetic instead of one per
                // quantity at the end of it (a quantity of type 0 or 2 in such a ring loads its reference as well
                // and drops it in damp_select).  The damped ring is a basic block of its own that holds the loads
                // AND every use: a load whose use is behind another branch leaves the compiler's s_waitcnt pass with
                // a "maybe pending" register at every later store of the loop, and the pinned prefetch (bottom of
                // the loop) would be waited for on the spot again.  The other rings run the block without a load.
                auto new_state = [&](const bool damped) {
                    double vr0 = 0.0, va0 = 0.0, s0 = 0.0, e0 = 0.0;
                    if (damped) {
                        vr0 = ld_off(W.vrad0, g);
                        va0 = ld_off(W.vazi0, g);
                        s0 = ld_off(W.sigma0, g);
                        if (ADI)
                            e0 = ld_off(W.energy0, g);
                    }
                    double vr = 0.0;
                    if (i != 0)
                        vr = (rp + Q[1][0]) * FAST_RCP_TR(sp + S[0]);
                    double va = (lpm + Q[3][0]) * FAST_RCP_TR(sm + S[0]) * invr - romega;
                    double sf = S[0] < P.sigma_floor_abs ? P.sigma_floor_abs : S[0];
                    double e = ADI ? clamp_energy_fast(P, E[0], sf) : 0.0;
                    if (damped) {
                        vr = damp_select(vr, tr.tvr, si.ev, vr0, 0.0);
                        va = damp_select(va, tr.tva, si.es, va0, 0.0);
                        sf = damp_select(sf, tr.tsg, si.es, s0, W.sigma_floor_abs);
                        if (ADI)
                            e = damp_select(e, tr.ten, si.es, e0, 0.0);
                    }
                    o_vr = vr, o_va = va, o_s = sf, o_e = e;
                };
                if (DAMP && (tr.tvr | tr.tva | tr.tsg | (ADI ? tr.ten : 0)) != 0)
                    new_state(true);
                else
                    new_state(false);
                out_g = g;
                out_on = true;
            }
            rmp_prev = Q[0][0];
            S_prev = S[0];
        }
        // ---- bottom: rotate, take ring m+1, start ring m+2, then this iteration's stores ------
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            w[2][q] = w[1][q];
            w[1][q] = w[0][q];
            F1[q] = F0[q];
        }
        if (!DIET)
            er[2] = er[1], er[1] = er[0];
        if (!DVP)
            vp[2] = vp[1], vp[1] = vp[0];
        if (DIET)
            idr_prev = tr.idr_up;
        if (m < r1 + 1) {
            convert(m + 1, nxt, r_next, romega_next);
            // The loads of fetch() must go straight into the registers convert() has just read.  Left alone, the
            // compiler sinks convert() below them, loads into fresh registers and copies those back behind an
            // s_waitcnt vmcnt(0): the prefetch becomes a blocking load, once per ring.  The empty asm pins the
            // results of convert() above it and (memory clobber) the loads below it.
            if (PIN) {
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    asm volatile("" : "+v"(w[0][q]));
                asm volatile("" : "+v"(vr_last));
                asm volatile("" ::: "memory");
            }
            if (m < r1)
                fetch(m + 2, nxt);
        }
        if (out_on) {
            if (valid) {
                st_off(W.vrad, out_g, o_vr);
                st_off(W.vazi, out_g, o_va);
                st_off(W.sigma, out_g, o_s);
                if (ADI)
                    st_off(W.energy, out_g, o_e);
            }
            if (i == nr - 1 && valid) { // v_r row Nr is neither transported nor shifted: copied column by column
                const unsigned gt = ((unsigned)nr * (unsigned)nphi + (unsigned)jin) * 8u;
                double v = ld_off(P.vrad, gt);
                if (DAMP) { // (the reference value requested with the row itself, whatever the type: one round trip)
                    const double v0 = ld_off(W.vrad0, gt);
                    const DampRow dn = crow_load(W.damp_tab, nr);
                    v = damp_select(v, dn.tvr, si.ev_top, v0, 0.0);
                }
                st_off(W.vrad, gt, v);
            }
        }
    }
#ifdef TF_TRACE
    if (lane == 0)
        W.temperature[4 * trace_slot + 1] = (double)wall_clock64();
#endif
}

// The kernel proper: the register allocator is told to aim for 4 wavefronts per SIMD (<= 128 VGPRs, no scratch in
// any instantiation).
template <bool ADI, bool DAMP, int LIM>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4)))
k_transport_fused(const Dev P, const Dev W, int tiles, int rows, int has_fallback, const TfChunks ch)
{
    transport_fused_body<ADI, DAMP, LIM>(P, W, tiles, rows, has_fallback, ch);
}
