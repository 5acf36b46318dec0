// Chunk planner of the marching kernels (see fcpt_schedule.h): pure host arithmetic, no HIP.
#include "fcpt_schedule.h"

#include <cstring>

namespace fcpt {

// Rings per marching chunk.  A marching wavefront is a serial chain of (rows + pre-roll) ring iterations, and the
// GPU holds a fixed number of them at a time (CUs x 4 SIMDs x the kernel's wavefronts per SIMD).  What a launch costs
// is the number of ROUNDS of resident wavefronts -- an integer -- times the length of the chain: the chunk length
// that minimises (rows + pre-roll) x rounds is taken.  Measured (round 2; 2048 rings unless noted):
//   source march, ideal EOS, Nphi = 4096: 36 rings (3 990 wavefronts, one round) 0.5277 ms per step, 24 rings (two
//     rounds, the second 47 % full) 0.5415, 35 rings (4 130 wavefronts: two rounds of long chains) 0.575; Nphi = 6144:
//     54 rings 0.774 against 0.789 at 24; 1024 x 3072: 14 rings 0.2345-0.2362 against 0.2424 at 7;
//   source march, isothermal, Nphi = 6144: 36 rings 0.5104-0.5148 against 0.5303-0.5322 at 24; Nphi = 4096: 24 rings
//     (one round) 0.368, 23 (two) 0.397;
//   transport: see transport_rows().
// Small grids have fewer wavefronts than slots at any length: the shortest chunks (4 rings) win there.

// Rings per thread (or wavefront) of the marching kernels of the per-loop path (k_transport_radial, k_cfl_cells,
// k_transport_theta_march): a thread that owns `rows` rings is a serial chain of rows (+ pre-roll) dependent
// iterations, which pays off only when there are more cells than the GPU has lanes to put them on.  On the small
// grids of the reference's tests the shortest chain wins (measured, round 3, shock tube 4096 x 4: k_transport_radial
// 31.5 us at 16 rings per thread, k_transport_theta_march 27.6 us at 8 rings per wavefront -- 57 % of a 104 us step of
// 15 launches; profiles/r03_narrow_kernels.txt).
int march_len(const Dev &P, int n_cu, int rows_full)
{
    const long lanes = (long)n_cu * 4 * 8 * 64; // every SIMD eight wavefronts deep
    const long cells = (long)P.nr * P.nphi;
    int rows = rows_full;
    while (rows > 1 && cells / rows < lanes)
        rows >>= 1;
    return rows;
}
// wavefronts per SIMD of the source-march instantiation that will run: 6 (isothermal), 4 (with StabilizeViscosity; ideal
// EOS), 2 (ideal EOS with cooling terms or StabilizeViscosity)
static int source_occupancy(const Dev &P)
{
    const bool wide_adi = P.adiabatic && (P.stabilize || P.cooling_surface || P.cooling_beta || P.heating_star || P.accel_force);
    return P.adiabatic ? (wide_adi ? 2 : 4) : (P.stabilize ? 4 : 6);
}
int source_rows(const Dev &P, int n_cu)
{
    if (P.opt.source_rows > 0)
        return P.opt.source_rows;
    const int segs = segments_of(P.nphi);
    const int occ = source_occupancy(P);
    const long slots = (long)n_cu * 4 * occ;
    int r = 4;
    long best_cost = 0;
    for (int rows = 4; rows <= 64; ++rows) {
        const long waves = (long)segs * ((P.nr + 1 + rows - 1) / rows);
        const long cost = (rows + 4) * ((waves + slots - 1) / slots);
        if (best_cost == 0 || cost < best_cost) {
            best_cost = cost;
            r = rows;
        }
    }
    // the boundary call folded into the kick needs the last chunk to hold rows nr-2 .. nr: a slightly longer chunk if
    // the division leaves fewer than three rows over
    for (int dr = 0; dr < 4; ++dr) {
        const int chunks = (P.nr + 1 + r + dr - 1) / (r + dr);
        if ((P.nr + 1) - (chunks - 1) * (r + dr) >= 3)
            return r + dr;
    }
    return r;
}

// One round of wavefronts, all starting together: chunk lengths matched to the SIMD rank of the wavefront that will
// march them.  One entry (column, first ring, one past the last, 0) per wavefront, indexed by blockIdx.x * 4 +
// wavefront of the block, i.e. in the order of dispatch.  Every XCD keeps a contiguous eighth of the rings; within it
// each of the `cols` columns is cut into `cpc` chunks, dealt to the dispatch order in a snake, and a chunk of rank r
// gets (rings + pre) ~ 1 - g r / (occ - 1): see source_schedule() for the why and the measurements.
// wpr: wavefronts of one rank in an XCD; min_len: a shorter chunk means the bounds of the caller do not hold -- an
// empty table (equal chunks) rather than a wrong one.
// cum == null: every ring costs 1, the eighths are x * rows / 8 in integers and an edge is rounded to the nearest ring
// (the source marches).  cum != null: cum[i] is the cost of rings [0, i); eighths and edges are the first ring whose
// cumulated cost reaches the mark (the transport).  The two roundings differ and both are kept: the tables of either
// caller are what was measured.
static std::vector<int> rank_matched_chunks(int cols, int rows, int occ, int wpr, int cpc, int pre, int min_len, double g,
                                            const std::vector<double> *cum)
{
    std::vector<double> w(occ);
    for (int r = 0; r < occ; ++r)
        w[r] = 1.0 - g * r / (occ - 1);
    auto ring_at = [&](double cost) { // first ring index whose cumulated cost reaches `cost`
        int lo = 0, hi = rows;
        while (lo < hi) {
            const int mid = (lo + hi) / 2;
            if ((*cum)[mid] < cost)
                lo = mid + 1;
            else
                hi = mid;
        }
        return lo;
    };
    auto eighth = [&](int x) {
        if (!cum)
            return (int)((long)x * rows / 8);
        return x == 0 ? 0 : x == 8 ? rows : ring_at((*cum)[rows] * x / 8.0);
    };
    const int nblk = (cpc * cols + 3) / 4; // workgroups per XCD
    std::vector<int> out((size_t)nblk * 8 * 4 * 4, 0);
    for (int x = 0; x < 8; ++x) {
        const int A = eighth(x), B = eighth(x + 1);
        const double n = cum ? (*cum)[B] - (*cum)[A] : (double)(B - A);
        for (int c = 0; c < cols; ++c) {
            double sw = 0.0;
            for (int j = 0; j < cpc; ++j) {
                const int q = j * cols + ((j & 1) ? cols - 1 - c : c);
                sw += w[q / wpr < occ ? q / wpr : occ - 1];
            }
            const double scale = (n + (double)cpc * pre) / sw;
            double edge = 0.0;
            int k0 = A;
            for (int j = 0; j < cpc; ++j) {
                const int q = j * cols + ((j & 1) ? cols - 1 - c : c);
                edge += scale * w[q / wpr < occ ? q / wpr : occ - 1] - pre;
                const int k1 = j == cpc - 1 ? B : (cum ? ring_at((*cum)[A] + edge) : A + (int)(edge + 0.5));
                if (k1 < k0 + min_len || k1 > B) // (cannot happen with the bounds of the callers; equal chunks rather than a wrong table)
                    return {};
                const size_t t = ((size_t)(q / 4) * 8 + x) * 4 + (q & 3);
                out[4 * t] = c, out[4 * t + 1] = k0, out[4 * t + 2] = k1;
                k0 = k1;
            }
        }
    }
    return out;
}
// Rank-matched chunks for the marching source kernels: one entry (segment, first ring, one past the last, 0) per
// wavefront, indexed by blockIdx.x * 4 + wavefront of the block, i.e. in the order of dispatch.
//
// Why: these kernels run as ONE round of wavefronts (the cheapest form: source_rows()), all starting together.  A SIMD
// issues for its oldest wavefront first, and the dispatcher hands every CU of an XCD one workgroup before any gets its
// second: the q-th wavefront an XCD receives sits at rank q / (4 x CUs) of its SIMD and advances at a rate that falls
// with the rank -- the trace of k_source_march_adi at 2048 x 4096 (profiles/r03_sm_wave_trace_ideal_uniform.txt) shows
// the four ranks ending at 125 / 135 / 152 / 172 us of 181, i.e. rates 1 : 0.92 : 0.79 : 0.65 while all four are resident,
// and the GPU a third empty for the last 58 us.  Chunk lengths in proportion to the rate of the rank that will march them
// ((rings + pre-roll) ~ 1 - g rank / (ranks - 1)) end all wavefronts together.
// Every XCD keeps a contiguous eighth of the rings (its L2 serves the shared halo cells); within it every segment
// (column of 59 cells) is cut into as many chunks as fit the XCD's slots once, and the chunks of the columns are dealt
// to the dispatch order in a snake (0 .. segs-1, segs-1 .. 0, ...) so that every column gets nearly the same mix of ranks.
// Empty where equal chunks stay: source_rows > 0, source_graded = 0, more than one round, chains beyond 64 rings.
std::vector<int> source_schedule(const Dev &P, int n_cu)
{
    if (P.nphi < 128 || P.opt.source_rows > 0 || P.opt.source_graded == 0)
        return {};
    const int segs = segments_of(P.nphi);
    const int occ = source_occupancy(P);
    const int wpr = n_cu / 8 * 4; // wavefronts of one rank in an XCD: one per SIMD
    const int rows = P.nr + 1;    // v_r has rows 0 .. nr
    if (wpr < 4 || occ < 2 || rows < 64)
        return {};
    const int cpc = wpr * occ / segs; // chunks per column in an XCD's eighth of the rings
    if (cpc < 2)
        return {};
    const int rx = rows / 8;
    if (cpc > rx / 6)
        return {}; // short chunks: the grid does not fill the slots once (source_rows() picks the shortest equal chunks)
    if ((rx + 1 + cpc - 1) / cpc > 64)
        return {}; // one round would be chains longer than any measured: several rounds of equal chunks
    const double g = (P.opt.source_graded > 0 && P.opt.source_graded < 100 ? P.opt.source_graded : (P.adiabatic ? 35 : 20)) * 0.01;
    return rank_matched_chunks(segs, rows, occ, wpr, cpc, 4, 3, g, nullptr);
}
// The same table from an explicit list of chunk lengths (fcpt_set_source_chunks: tuning runs and tests).  The rows
// 0 .. nr of v_r are cut from row 0 upward into chunks of the given lengths, the last entry repeating; a remainder of
// fewer than three rings is joined to the chunk before it (the launcher folds the boundary call into the edge chunks of
// a table, which must have stored the three rows it reads themselves); the same cut serves every segment.  Entries in
// dispatch order, chunk-major and the segments of a chunk side by side, padded with idle entries (first == last) to
// whole workgroups of four wavefronts.  Empty where the marching kernels do not run (rings of fewer than 128 cells,
// slabs of fewer than three rows) -- and, with *refused set, for a list that holds a length below three.
std::vector<int> source_schedule_explicit(const Dev &P, const std::vector<int> &lengths, bool *refused)
{
    if (refused)
        *refused = false;
    for (int len : lengths)
        if (len < 3) {
            if (refused)
                *refused = true;
            return {};
        }
    const int rows = P.nr + 1; // v_r has rows 0 .. nr
    if (lengths.empty() || P.nphi < 128 || rows < 3)
        return {};
    const int segs = segments_of(P.nphi);
    std::vector<int> out;
    int k0 = 0;
    for (size_t c = 0; k0 < rows; ++c) {
        const int len = lengths[c < lengths.size() ? c : lengths.size() - 1];
        int k1 = len < rows - k0 ? k0 + len : rows;
        if (rows - k1 < 3) // no crumbs
            k1 = rows;
        for (int s = 0; s < segs; ++s) {
            const int e[4] = {s, k0, k1, 0};
            out.insert(out.end(), e, e + 4);
        }
        k0 = k1;
    }
    out.resize((out.size() + 15) / 16 * 16, 0);
    return out;
}
// Chunks of graded length for k_transport_fused, in dispatch order: (first ring, one past the last) pairs.
//
// Why: the wavefront trace of the kernel (profiles/tools/wave_trace_transport.py, profiles/r03_tf_wave_trace_uniform.txt) shows
// equal chunks leaving a long tail.  At 2048 x 4096 the 8 034 wavefronts of 103 twenty-ring chunks take two rounds of
// the 4 096 slots; a SIMD issues for its OLDEST wavefront first, so the four wavefronts of a SIMD finish 58 ... 95 us
// after a common start, the second round starts staggered over 40 us and ends staggered over 58 us, during which the
// GPU holds 1 900 wavefronts on average: 188 us for 150 us of full-occupancy work.  Long chunks first and ever shorter
// ones behind them (guided self-scheduling) let the slots run dry together: the last wavefronts a slot receives are
// short, and their pre-roll (4 cheap + 1 full iteration per chunk) is paid on a small share of the rings only.
//
// Three lengths (see the body for the numbers).  Chunks are taken from both ends of the
// slab alternately (the damping zones -- costlier rings, `slow` = 1 -- sit at the ends and start first, and they
// count 1.4 rings each).  Returns an empty vector where equal chunks stay: tuning runs (transport_rows > 0,
// transport_graded = 0) and grids whose wavefronts fit the slots once (the shortest chunks win there: transport_rows()).
static std::vector<int> transport_chunk_list(const Dev &P, int n_cu, const std::vector<int> &slow, const std::vector<int> *lengths)
{
    std::vector<int> out;
    if (P.nphi < 256 || P.opt.transport_rows > 0 || P.opt.transport_graded == 0)
        return out;
    if (P.opt.transport_fused == 0)
        return out;
    const long tiles = tiles_of(P.nphi);
    const long slots = (long)n_cu * 4 * 4; // 4 wavefronts per SIMD (128 VGPRs)
    const double conc = (double)slots / (double)tiles; // chunks resident at once
    const bool explicit_spec = lengths && !lengths->empty(); // fcpt_set_transport_chunks / FCPT_TF_SCHEDULE: tuning runs and tests
    if (!explicit_spec) {
        const int rows_u = transport_rows(P, n_cu);
        if ((long)((P.nr + rows_u - 1) / rows_u) * tiles <= slots || conc < 16.0)
            return out; // equal chunks need one round only / rings so long that a few chunks fill an XCD
    }
    const int COST = 10, COST_SLOW = 14; // tenths of a ring
    long total = 0;
    for (int i = 0; i < P.nr; ++i)
        total += (i < (int)slow.size() && slow[i]) ? COST_SLOW : COST;
    // lengths in dispatch order, in rings of cost
    std::vector<int> len;
    if (explicit_spec) {
        len = *lengths;
    } else {
        // level 0: the same number of chunks for every XCD (they are dealt round-robin), enough of them to fill the
        // XCD's slots once; 74 % of the cost there, then three chunks per XCD of 0.43 of that length, the rest at 0.21
        // (measured at 2048 x 4096, 78 tiles, 512 slots per XCD: 28 x 56, 12 x 24, 6 ...: profiles/r03_tf_schedule_sweep.txt)
        const long slots_xcd = slots / 8;
        const int k0 = (int)((slots_xcd + tiles - 1) / tiles);
        const int n0 = 8 * k0;
        int big = P.opt.transport_big > 0 ? P.opt.transport_big : (int)(0.74 * (double)total / COST / n0 + 0.5);
        big = big < 4 ? 4 : big;
        const double ladder = (P.opt.transport_ladder > 0 && P.opt.transport_ladder <= 100 ? P.opt.transport_ladder : 43) * 0.01;
        const int n1 = 8 * ((int)(0.43 * k0 + 0.5) < 1 ? 1 : (int)(0.43 * k0 + 0.5));
        const int l1 = (int)(big * ladder + 0.5) < 4 ? 4 : (int)(big * ladder + 0.5);
        const int l2 = (int)(big * ladder * 0.5 + 0.5) < 4 ? 4 : (int)(big * ladder * 0.5 + 0.5);
        for (int k = 0; k < n0; ++k)
            len.push_back(big);
        for (int k = 0; k < n1; ++k)
            len.push_back(l1);
        len.push_back(l2); // ... repeated to the end
    }
    int lo = 0, hi = P.nr;
    for (size_t k = 0; lo < hi; ++k) {
        const int lk = len[k < len.size() ? k : len.size() - 1];
        const long target = (long)(lk < 1 ? 1 : lk) * COST;
        long cost = 0;
        if ((k & 1) == 0) {
            const int r0 = lo;
            while (lo < hi && cost < target)
                cost += (lo < (int)slow.size() && slow[lo]) ? COST_SLOW : COST, ++lo;
            if (hi - lo < 3) // no crumbs
                lo = hi;
            out.push_back(r0), out.push_back(lo);
        } else {
            const int r1 = hi;
            while (lo < hi && cost < target)
                cost += (hi - 1 < (int)slow.size() && slow[hi - 1]) ? COST_SLOW : COST, --hi;
            if (hi - lo < 3)
                hi = lo;
            out.push_back(hi), out.push_back(r1);
        }
    }
    return out;
}
// One round of wavefronts (grids whose equal chunks fit the slots once): chunk lengths matched to the SIMD rank of the
// wavefront, exactly as source_schedule() does for the source marches -- the trace of the 1024 x 3072 transport
// (profiles/r03_tf_wave_trace_config3_uniform.txt) shows all 3 712 wavefronts resident for 50 us and then leaving over
// the next 43.  Entries (tile, first ring, one past the last, 0) indexed by blockIdx.x * 4 + wavefront of the workgroup.
static std::vector<int> transport_rank_table(const Dev &P, int n_cu, const std::vector<int> &slow)
{
    if (P.opt.transport_rank_grade == 0)
        return {};
    const int tiles = tiles_of(P.nphi);
    const int occ = 4;
    const int wpr = n_cu / 8 * 4; // wavefronts of one rank in an XCD: one per SIMD
    const int rows = P.nr;
    if (wpr < 4 || rows < 128)
        return {};
    const int cpc = wpr * occ / tiles; // chunks per tile column in an XCD's eighth of the rings
    const int rx = rows / 8;
    if (cpc < 2 || rx / cpc < 10)
        return {}; // short chunks (the grid does not fill the slots with chunks of ten rings): transport_rows()'s equal ones
    if ((rx + cpc) / cpc > 64)
        return {};
    const double g = (P.opt.transport_rank_grade > 0 && P.opt.transport_rank_grade < 100 ? P.opt.transport_rank_grade : (P.adiabatic ? 45 : 60)) * 0.01;
    // cost of the rings: a damping-zone ring (reference values loaded and waited for) counts 1.4 -- the XCDs get equal
    // cost, not equal numbers of rings (the zones sit in the first and the last XCD's range), and so do the chunks
    std::vector<double> cum(rows + 1, 0.0);
    for (int i = 0; i < rows; ++i)
        cum[i + 1] = cum[i] + ((i < (int)slow.size() && slow[i]) ? 1.4 : 1.0);
    return rank_matched_chunks(tiles, rows, occ, wpr, cpc, 5, 2, g, &cum);
}
// The table k_transport_fused runs from: per wavefront (tile, first ring, one past the last, 0) in the order of
// dispatch -- graded chunks (several rounds of wavefronts: transport_chunk_list, every chunk's tiles side by side on one
// XCD), rank-matched chunks (one round: transport_rank_table), or empty: equal chunks of transport_rows() rings.
std::vector<int> transport_schedule(const Dev &P, int n_cu, const std::vector<int> &slow, const std::vector<int> *lengths)
{
    std::vector<int> out;
    if (P.nphi < 256 || P.opt.transport_rows > 0 || P.opt.transport_fused == 0)
        return out;
    const int tiles = tiles_of(P.nphi);
    const std::vector<int> chunks = transport_chunk_list(P, n_cu, slow, lengths);
    if (chunks.empty()) {
        const bool explicit_spec = lengths && !lengths->empty();
        if (explicit_spec || P.opt.transport_graded == 0)
            return out;
        // one round of equal chunks?
        const int rows_u = transport_rows(P, n_cu);
        if ((long)((P.nr + rows_u - 1) / rows_u) * tiles > (long)n_cu * 4 * 4)
            return out;
        return transport_rank_table(P, n_cu, slow);
    }
    const int count = (int)(chunks.size() / 2);
    // as the kernel deals equal chunks: workgroup b runs on XCD b % 8; chunk c on XCD c % 8, its tiles side by side
    const int nblk = 8 * ((((count + 7) / 8) * tiles + 3) / 4);
    out.assign((size_t)nblk * 4 * 4, 0);
    for (int b = 0; b < nblk; ++b)
        for (int wv = 0; wv < 4; ++wv) {
            const int xcd = b & 7, wq = (b >> 3) * 4 + wv, zq = wq / tiles, c = xcd + 8 * zq;
            if (c >= count)
                continue;
            const size_t t = (size_t)b * 4 + wv;
            out[4 * t] = wq - zq * tiles, out[4 * t + 1] = chunks[2 * c], out[4 * t + 2] = chunks[2 * c + 1];
        }
    return out;
}
void selftest_chunk_tables(int nr, int nphi, int n_cu, int adiabatic, int damp_inner, int damp_outer, const Options &opt,
                           std::vector<int> &transport, std::vector<int> &source)
{
    Dev P;
    std::memset(&P, 0, sizeof(P));
    P.nr = nr, P.nphi = nphi, P.adiabatic = adiabatic, P.opt = opt;
    P.damp_in_step = (damp_inner > 0 || damp_outer > 0) ? 1 : 0;
    std::vector<int> slow(nr > 0 ? nr : 0, 0);
    for (int i = 0; i < nr; ++i)
        slow[i] = (i < damp_inner || i >= nr - damp_outer) ? 1 : 0;
    transport = transport_schedule(P, n_cu, slow, nullptr);
    source = source_schedule(P, n_cu);
}
// The transport deals whole chunks to the 8 XCDs (k_transport_fused), so the rounds are counted per XCD; and its
// chunks are not equal: the rings of the damping zones (folded into the kernel) cost ~1.5x and are started first, which
// adds half a round to the last one.  cost = (rows + 5) x (rounds - 1 + slow).  Measured: 2048 x 4096 (78 tiles): 20
// rings (13 chunks per XCD, 1 014 wavefronts for 512 slots: 2 rounds) 0.363 ms per step; 18 (15 chunks: 3 rounds) 0.377;
// 24 (2 rounds of longer chains) 0.367-0.371; 40 (7 chunks on some XCDs = 546 wavefronts: 2 rounds of 45) 0.41;
// 1024 x 3072 ideal (58 tiles): 16 rings (8 chunks per XCD, one round) 0.2374-0.2383 against 0.2434-0.2448 at 8
// and 0.250 at 14 (10 chunks per XCD: 580 wavefronts, two rounds).
int transport_rows(const Dev &P, int n_cu)
{
    if (P.opt.transport_rows > 0)
        return P.opt.transport_rows;
    const long tiles = tiles_of(P.nphi);
    const long slots_xcd = (long)n_cu / 8 * 4 * 4; // 4 wavefronts per SIMD (128 VGPRs)
    const double slow = P.damp_in_step ? 1.5 : 1.0;
    int r = 4;
    double best_cost = 0.0;
    for (int rows = 4; rows <= 32; ++rows) { // (longer single-round chains are unmeasured)
        const long chunks = (P.nr + rows - 1) / rows;
        // (launches of fewer than TF_XCD_CHUNKS chunks deal workgroups, not chunks: all wavefronts over all slots)
        const long rounds = chunks >= TF_XCD_CHUNKS ? (((chunks + 7) / 8) * tiles + slots_xcd - 1) / slots_xcd
                                                    : (chunks * tiles + 8 * slots_xcd - 1) / (8 * slots_xcd);
        const double cost = (rows + 5) * (rounds - 1 + slow);
        if (best_cost == 0.0 || cost < best_cost * (1.0 - 1e-12))
            best_cost = cost, r = rows;
    }
    return r;
}
// will launch_source_march() take the step?
bool source_march_applies(const Dev &P)
{
    if (P.nphi < 128)
        return false;
    if ((long long)(P.nr + 1) * P.nphi >= (1ll << 29))
        return false; // the kernels address cells by 32-bit byte offsets (ld_off): grids below 4 GiB
    return !P.adiabatic || P.opt.march_source_adi != 0;
}
// the fused kernel runs, nothing is queued behind it, and there are chunks between the two ends
bool transport_can_split(const Dev &P, int n_cu, bool shear_safe)
{
    if (P.nphi < 256 || !shear_safe)
        return false;
    if (P.opt.transport_fallback != 0)
        return false; // the fallback kernels behind the fused one need all of its chunks in one launch
    if (P.opt.transport_fused == 0 || P.opt.transport_rows > 0)
        return false; // no fused kernel / tuning runs keep the one-launch form
    if (P.opt.transport_split == 0)
        return false;
    const int rows = transport_rows(P, n_cu);
    const int chunks = (P.nr + rows - 1) / rows, c_lo = (P.nr - 2 * FCPT_OVERLAP) / rows;
    const int lead = (2 * FCPT_OVERLAP + rows - 1) / rows; // chunks that hold rows [0, 14)
    return c_lo > lead && c_lo < chunks;
}

} // namespace fcpt
