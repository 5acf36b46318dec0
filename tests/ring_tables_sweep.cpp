// Stand-alone sweep of the per-ring tables of fcpt_create (fargocpt_amd/csrc/fcpt_tables.cpp, linked with fcpt_host.cpp
// and nothing else): over a range of small grids, ring lengths, slab splits and damping settings every table must have
// its size and hold finite numbers.  Built and run by tests/test_ring_tables_sweep.py with the address and
// undefined-behaviour sanitizers: the builder reads the geometry arrays at Rinf[i + 1] for i = nr and fills rows up to
// nr + 5, and a read outside them is a failure here, on a CPU.  Exit status 0 and nothing on stderr: all grids passed.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../fargocpt_amd/csrc/fcpt_internal.h"

using namespace fcpt;

static int failures = 0;
static char what[256];
static void fail(const char *msg, long a = 0, long b = 0)
{
    if (++failures <= 20)
        std::fprintf(stderr, "%s: %s (%ld, %ld)\n", what, msg, a, b);
}

static void check_size(const char *name, size_t have, size_t want)
{
    if (have != want) {
        std::fprintf(stderr, "%s: ", name);
        fail("wrong size", (long)have, (long)want);
    }
}

static void check_finite(const char *name, const double *v, size_t n)
{
    for (size_t k = 0; k < n; ++k)
        if (!std::isfinite(v[k])) {
            std::fprintf(stderr, "%s: ", name);
            fail("not finite at", (long)k);
            return;
        }
}

template <class Row> static void check_rows(const char *name, const std::vector<Row> &rows, size_t want, size_t doubles_per_row)
{
    check_size(name, rows.size(), want);
    for (const Row &r : rows)
        check_finite(name, reinterpret_cast<const double *>(&r), doubles_per_row);
}

static void check_tables(const fcpt_desc &d, const fcpt_split &s, const RingTables &t)
{
    const size_t nr = (size_t)s.nr, nphi = (size_t)d.nphi;
    const struct {
        const char *name;
        const std::vector<double> &v;
        size_t n;
    } arrays[] = {{"cosphi", t.cosphi, nphi}, {"sinphi", t.sinphi, nphi}, {"cs_ring", t.cs_ring, nr}, {"nu_ring", t.nu_ring, nr},
                  {"g_dxtheta", t.g_dxtheta, nr + 1}, {"g_inv_dxtheta", t.g_inv_dxtheta, nr + 1}, {"g_dr_invsurf", t.g_dr_invsurf, nr + 1},
                  {"g_r_omega", t.g_r_omega, nr + 1}, {"g_inv_omk", t.g_inv_omk, nr + 1}, {"g_omk", t.g_omk, nr + 1},
                  {"g_ra3", t.g_ra3, nr + 2}, {"fs", t.fs, nr + 1}, {"ts", t.ts, nr + 1}, {"fv", t.fv, nr + 1}, {"tv", t.tv, nr + 1}};
    for (const auto &a : arrays) {
        check_size(a.name, a.v.size(), a.n);
        check_finite(a.name, a.v.data(), a.v.size());
    }
    check_rows("SrcRow", t.src, nr + 8, sizeof(SrcRow) / sizeof(double));
    check_rows("RadRow", t.rad, nr + 2, sizeof(RadRow) / sizeof(double));
    check_rows("ThetaRow", t.theta, nr, sizeof(ThetaRow) / sizeof(double));
    check_rows("DampRow", t.damp_rows, nr + 1, 4); // (four doubles, then the four types)
    check_size("ring_ref_damped", t.ring_ref_damped.size(), nr);
    for (int q = 0; q < 4; ++q) {
        check_size("dtype", t.dtype[q].size(), nr + 1);
        for (int v : t.dtype[q])
            if (v < 0 || v > 2)
                fail("damping type out of range", q, v);
        for (int o = 0; o < 2; ++o) {
            const DampRange &r = t.damp[q][o];
            if (r.lo <= r.hi && (r.lo < 0 || r.hi > (int)nr - (q == 0 ? 0 : 1)))
                fail("damping range outside the slab", r.lo, r.hi);
            if (!std::isfinite(r.rlim) || !std::isfinite(r.redge) || !std::isfinite(r.tau))
                fail("damping range not finite", q, o);
        }
    }
    if (t.damp_foldable && !t.damp_any)
        fail("damp_foldable without damp_any");
}

int main()
{
    const int NPHI[] = {2, 16, 17, 128};
    long grids = 0, refused = 0;
    std::vector<double> radii;
    for (int nranks : {1, 2, 4})
        // one slab: 3 .. 40 rings; more slabs: from the narrowest grid the split accepts (2 * FCPT_OVERLAP rings per
        // slab before the overlap is added) to slabs of 40 rings
        for (int nr_global = nranks == 1 ? 3 : 2 * FCPT_OVERLAP * nranks; nr_global <= (nranks == 1 ? 40 : nranks == 2 ? 66 : 104); ++nr_global)
            for (int spacing : {FCPT_SPACING_ARITHMETIC, FCPT_SPACING_LOGARITHMIC, FCPT_SPACING_EXPONENTIAL})
                for (int nphi : NPHI)
                    for (int damping = 0; damping < 3; ++damping) // off; zones several rings wide; zones wider than the grid
                        for (int rank = 0; rank < nranks; ++rank) {
                            if (spacing == FCPT_SPACING_EXPONENTIAL && (nranks != 1 || nphi != 16 || nr_global % 4))
                                continue; // (its Newton iteration takes 500 000 steps per grid: a few grids only)
                            fcpt_desc d;
                            fcpt_desc_default(&d);
                            d.nr_global = nr_global, d.nphi = nphi, d.rank = rank, d.nranks = nranks, d.radial_spacing = spacing;
                            d.viscous_alpha = (nr_global & 1) ? 1.0e-3 : 0.0;
                            d.constant_viscosity = 1.0e-5;
                            d.omega_frame = 1.0;
                            d.damping = damping > 0;
                            d.damping_inner_limit = damping == 2 ? 10.0 : 1.35;
                            d.damping_outer_limit = damping == 2 ? 0.01 : 0.75;
                            for (int o = 0; o < 2; ++o) {
                                d.damp_vrad[o] = o ? FCPT_DAMP_REFERENCE : FCPT_DAMP_ZERO;
                                d.damp_vaz[o] = FCPT_DAMP_REFERENCE;
                                d.damp_sigma[o] = o ? FCPT_DAMP_NONE : ((nphi == 17) ? FCPT_DAMP_MEAN : FCPT_DAMP_REFERENCE);
                                d.damp_energy[o] = o ? FCPT_DAMP_ZERO : FCPT_DAMP_NONE;
                            }
                            std::snprintf(what, sizeof(what), "%d x %d, slab %d of %d, spacing %d, damping %d", nr_global, nphi, rank, nranks,
                                          spacing, damping);
                            radii.assign((size_t)nr_global + FCPT_GEOM_PAD + 1, 0.0);
                            fcpt_split s;
                            if (build_radii(d, radii.data()) || validate_create(&d, radii.data()) || split_domain(d, s)) {
                                ++refused; // (coarse grids: NaN radii of the exponential spacing, a first arithmetic interface below 0)
                                continue;
                            }
                            HostGeometry g;
                            build_geometry(d, s, radii.data(), g);
                            RingTables t;
                            build_ring_tables(d, s, g, t);
                            check_tables(d, s, t);
                            // the test hook with a buffer of exactly the size it reports (it builds everything again: one ring length)
                            for (int table = FCPT_TABLE_SRC; table <= FCPT_TABLE_AZIMUTH && nphi == 17; ++table) {
                                int32_t rows = 0, cols = 0;
                                if (fcpt_selftest_ring_tables(&d, radii.data(), table, nullptr, 0, &rows, &cols) || rows < 1 || cols < 1) {
                                    fail("the test hook refused table", table);
                                    continue;
                                }
                                std::vector<double> out((size_t)rows * cols, 0.0);
                                if (fcpt_selftest_ring_tables(&d, radii.data(), table, out.data(), (int64_t)out.size(), &rows, &cols))
                                    fail("the test hook failed for table", table);
                                check_finite("hook", out.data(), out.size());
                            }
                            ++grids;
                        }
    std::printf("%ld grids, %ld refused, %d failures\n", grids, refused, failures);
    if (grids < 2000)
        fail("the sweep lost its grids", grids);
    return failures ? 1 : 0;
}
