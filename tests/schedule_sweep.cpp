// Stand-alone sweep of the chunk planner (fargocpt_amd/csrc/fcpt_schedule.cpp, linked alone): every table it returns
// over a range of grids, device sizes and physics must be well formed.  Built and run by tests/test_schedule_sweep.py
// with the address and undefined-behaviour sanitizers, so that an index outside a table is a failure here, on a CPU,
// and not a fault on a GPU.  Exit status 0 and nothing on stderr: all tables passed.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../fargocpt_amd/csrc/fcpt_schedule.h"

using namespace fcpt;

static int failures = 0;
static char what[256];
static void fail(const char *msg, int a = 0, int b = 0, int c = 0)
{
    if (++failures <= 20)
        std::fprintf(stderr, "%s: %s (%d, %d, %d)\n", what, msg, a, b, c);
}

// entries (column, first ring, one past the last, 0), idle ones with first == last
static void check_table(const std::vector<int> &t, int cols, int rows, int min_len)
{
    if (t.empty())
        return;
    if (t.size() % 16 != 0)
        fail("length is no multiple of 16 ints", (int)t.size());
    std::vector<unsigned char> seen((size_t)cols * rows, 0);
    for (size_t k = 0; k + 3 < t.size(); k += 4) {
        const int c = t[k], r0 = t[k + 1], r1 = t[k + 2];
        if (r0 == r1)
            continue; // idle wavefront
        if (c < 0 || c >= cols || r0 < 0 || r0 >= r1 || r1 > rows) {
            fail("entry out of range", c, r0, r1);
            continue;
        }
        if (r1 - r0 < min_len)
            fail("chunk too short", c, r0, r1);
        for (int r = r0; r < r1; ++r)
            if (seen[(size_t)c * rows + r]++)
                fail("ring covered twice", c, r);
    }
    for (int c = 0; c < cols; ++c)
        for (int r = 0; r < rows; ++r)
            if (!seen[(size_t)c * rows + r]) {
                fail("ring not covered", c, r);
                return;
            }
}

// source_schedule_explicit (fcpt_set_source_chunks): besides check_table, the first live chunk of every segment starts
// at row 0 and its last one ends behind row `rows - 1`, and the entries stand chunk by chunk with the segments side by side
static void check_explicit_ends(const std::vector<int> &t, int cols, int rows)
{
    if (t.empty()) {
        fail("no table for an admissible list");
        return;
    }
    std::vector<int> first(cols, -1), last(cols, -1);
    size_t live = 0;
    for (size_t k = 0; k + 3 < t.size(); k += 4) {
        const int c = t[k], r0 = t[k + 1], r1 = t[k + 2];
        if (r0 == r1)
            continue;
        if (c < 0 || c >= cols)
            continue; // (reported by check_table)
        if (k / 4 != live)
            fail("an idle entry before a live one", (int)(k / 4));
        if (c != (int)(live % (size_t)cols))
            fail("segments of a chunk not side by side", (int)(k / 4), c);
        ++live;
        if (first[c] < 0)
            first[c] = r0;
        last[c] = r1;
    }
    for (int c = 0; c < cols; ++c) {
        if (first[c] != 0)
            fail("first live chunk does not start at row 0", c, first[c]);
        if (last[c] != rows)
            fail("last live chunk does not end behind the last row", c, last[c], rows);
    }
    if (t.size() / 4 - live >= 4)
        fail("more idle entries than fill the last workgroup", (int)(t.size() / 4), (int)live);
}

int main()
{
    const int NR[] = {6, 63, 64, 127, 128, 129, 500, 1024, 1367, 2048, 4099};
    // (1536, 3072, 6144 and 8192 were in the first list too: no other path than their neighbours, and half of the run time)
    const int NPHI[] = {2, 64, 127, 128, 255, 256, 384, 4096, 5462};
    const int CUS[] = {8, 32, 64, 104, 256, 304};
    const std::vector<int> LENGTHS[] = {{}, {1}, {28, 28, 12, 6}, {4096}};
    const std::vector<int> SOURCE_LENGTHS[] = {{3}, {3, 64}, {5, 3, 17, 4}, {4096}, {7, 7, 7, 3, 5, 13, 3}};
    const std::vector<int> SOURCE_REFUSED[] = {{2}, {5, 2, 9}, {7, 7, 2}, {3, 0}, {-4}};
    Options opt;
    std::memset(&opt, 0xff, sizeof(opt)); // every switch -1: the built-in choice
    opt.transport_graded = 1;
    long tables = 0;
    for (int nr : NR)
        for (int nphi : NPHI)
            for (int n_cu : CUS)
                for (int adiabatic = 0; adiabatic < 2; ++adiabatic)
                    for (int damp : {0, 33}) {
                        Dev P;
                        std::memset(&P, 0, sizeof(P));
                        P.nr = nr, P.nphi = nphi, P.adiabatic = adiabatic, P.opt = opt;
                        P.damp_in_step = damp > 0;
                        std::vector<int> slow(nr, 0);
                        for (int i = 0; i < nr; ++i)
                            slow[i] = i < damp || i >= nr - damp;
                        // source occupancy 6 / 4 (isothermal: plain / StabilizeViscosity), 4 / 2 (ideal EOS: plain / any of the three)
                        for (int variant = 0; variant < 4; ++variant) {
                            Dev Q = P;
                            Q.stabilize = variant == 1, Q.cooling_surface = variant == 2, Q.accel_force = variant == 3;
                            std::snprintf(what, sizeof(what), "source %d x %d, %d CUs, ideal %d, variant %d", nr, nphi, n_cu, adiabatic, variant);
                            check_table(source_schedule(Q, n_cu), segments_of(nphi), nr + 1, 3);
                            ++tables;
                        }
                        // explicit lists for the source marches: the device size and the physics do not enter
                        if (n_cu == CUS[0] && damp == 0) {
                            for (const std::vector<int> &len : SOURCE_LENGTHS) {
                                std::snprintf(what, sizeof(what), "explicit source %d x %d, ideal %d, %d lengths (%d ..)", nr, nphi, adiabatic,
                                              (int)len.size(), len[0]);
                                bool refused = true;
                                const std::vector<int> t = source_schedule_explicit(P, len, &refused);
                                if (refused)
                                    fail("an admissible list was refused");
                                if (nphi < 128) { // the marching kernels do not run on rings this short: no table
                                    if (!t.empty())
                                        fail("a table for rings of fewer than 128 cells");
                                } else {
                                    check_table(t, segments_of(nphi), nr + 1, 3);
                                    check_explicit_ends(t, segments_of(nphi), nr + 1);
                                }
                                ++tables;
                            }
                            for (const std::vector<int> &len : SOURCE_REFUSED) {
                                std::snprintf(what, sizeof(what), "refused source list %d x %d (%d ..)", nr, nphi, len[0]);
                                bool refused = false;
                                if (!source_schedule_explicit(P, len, &refused).empty() || !refused)
                                    fail("a list with a chunk of fewer than 3 rings was not refused");
                                ++tables;
                            }
                        }
                        for (const std::vector<int> &len : LENGTHS) {
                            std::snprintf(what, sizeof(what), "transport %d x %d, %d CUs, ideal %d, damp %d, %d lengths (%d ..)", nr, nphi, n_cu,
                                          adiabatic, damp, (int)len.size(), len.empty() ? 0 : len[0]);
                            // rank-matched (and not graded) tables: built-in lengths, and equal chunks would fit the slots once
                            const int rows_u = transport_rows(P, n_cu);
                            const bool ranked = len.empty() && (long)((nr + rows_u - 1) / rows_u) * tiles_of(nphi) <= (long)n_cu * 4 * 4;
                            check_table(transport_schedule(P, n_cu, slow, &len), tiles_of(nphi), nr, ranked ? 2 : 1);
                            ++tables;
                        }
                    }
    std::printf("%ld tables, %d failures\n", tables, failures);
    return failures ? 1 : 0;
}
