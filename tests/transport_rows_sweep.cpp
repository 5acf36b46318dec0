// Stand-alone check of the per-iteration rows of k_transport_fused (TfRow, fargocpt_amd/csrc/fcpt_tables.cpp, linked with
// fcpt_host.cpp and nothing else): for slabs of 8, 33 and 2048 rings, with and without damping zones, and every iteration
// m = -3 .. nr + 1 of the marching loop, each field of row m + 3 must be the field of the per-type table (RadRow, ThetaRow,
// DampRow) at the index the kernel's clamped loads used: interface max(m - 1, -1), ring m - 2 and ring m + 1, each
// replaced by ring 0 outside the grid.  Built and run by tests/test_transport_rows_host.py, plain and with the address
// and undefined-behaviour sanitizers.  Exit status 0 and nothing on stderr: all rows passed.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../fargocpt_amd/csrc/fcpt_internal.h"

using namespace fcpt;

static int failures = 0;
static void fail(const char *what, int nr, int m)
{
    if (++failures <= 20)
        std::fprintf(stderr, "nr = %d, iteration %d: %s differs\n", nr, m, what);
}
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; } // bit for bit

int main()
{
    long rows = 0, typed = 0;
    for (int nr : {8, 33, 2048})
        for (int damping = 0; damping < 2; ++damping) {
            fcpt_desc d;
            fcpt_desc_default(&d);
            d.nr_global = nr, d.nphi = 64, d.rank = 0, d.nranks = 1;
            d.omega_frame = 0.75;
            d.damping = damping;
            d.damping_inner_limit = 1.35, d.damping_outer_limit = 0.75;
            for (int o = 0; o < 2; ++o) {
                d.damp_vrad[o] = o ? FCPT_DAMP_REFERENCE : FCPT_DAMP_ZERO;
                d.damp_vaz[o] = FCPT_DAMP_REFERENCE;
                d.damp_sigma[o] = o ? FCPT_DAMP_NONE : FCPT_DAMP_REFERENCE;
                d.damp_energy[o] = o ? FCPT_DAMP_ZERO : FCPT_DAMP_NONE;
            }
            std::vector<double> radii((size_t)nr + FCPT_GEOM_PAD + 1, 0.0);
            fcpt_split s;
            if (build_radii(d, radii.data()) || validate_create(&d, radii.data()) || split_domain(d, s) || s.nr != nr) {
                std::fprintf(stderr, "nr = %d: the grid was refused\n", nr);
                return 1;
            }
            HostGeometry g;
            build_geometry(d, s, radii.data(), g);
            RingTables t;
            build_ring_tables(d, s, g, t);
            if (t.tf.size() != (size_t)nr + TF_ROW_GUARD || t.rad.size() != (size_t)nr + 2 || t.theta.size() != (size_t)nr ||
                t.damp_rows.size() != (size_t)nr + 1) {
                std::fprintf(stderr, "nr = %d: wrong table sizes\n", nr);
                return 1;
            }
            for (int m = -3; m <= nr + 1; ++m) {
                const int k = m - 1, i = m - 2;
                // the kernel's index expressions before the rows: rad_tab[(k < -1 ? -1 : k) + 1], theta_tab[do_i ? i : 0]
                // (do_i implies 0 <= i < nr), theta_tab[m + 1 in the grid ? m + 1 : 0], damp_tab[do_i ? i : 0]
                const RadRow &rk = t.rad[(size_t)((k < -1 ? -1 : k) + 1)];
                const ThetaRow &ti = t.theta[(size_t)((i >= 0 && i < nr) ? i : 0)];
                const ThetaRow &tn = t.theta[(size_t)((m + 1 >= 0 && m + 1 < nr) ? m + 1 : 0)];
                const DampRow &di = t.damp_rows[(size_t)((i >= 0 && i < nr) ? i : 0)];
                const TfRow &R = t.tf[(size_t)(m + 3)];
                if (!same(R.dr_lo, rk.dr_lo)) fail("dr_lo", nr, m);
                if (!same(R.dr_hi, rk.dr_hi)) fail("dr_hi", nr, m);
                if (!same(R.idr_up, rk.idr_up)) fail("idr_up", nr, m);
                if (!same(R.gphi, rk.gphi)) fail("gphi", nr, m);
                if (!same(R.invsurf, ti.invsurf)) fail("invsurf", nr, m);
                if (!same(R.dxtheta, ti.dxtheta)) fail("dxtheta", nr, m);
                if (!same(R.inv_dxtheta, ti.inv_dxtheta)) fail("inv_dxtheta", nr, m);
                if (!same(R.dr_invsurf, ti.dr_invsurf)) fail("dr_invsurf", nr, m);
                if (!same(R.invr, ti.invr)) fail("invr", nr, m);
                if (!same(R.r_omega, ti.r_omega)) fail("r_omega", nr, m);
                if (!same(R.r_next, tn.rmed)) fail("r_next", nr, m);
                if (!same(R.romega_next, tn.r_omega)) fail("romega_next", nr, m);
                if (R.tvr != di.tvr || R.tva != di.tva || R.tsg != di.tsg || R.ten != di.ten) fail("a damping type", nr, m);
                if (R.pad[0] != 0.0 || R.pad[1] != 0.0) fail("the padding", nr, m);
                typed += (R.tvr | R.tva | R.tsg | R.ten) != 0;
                ++rows;
            }
        }
    std::printf("%ld rows, %ld of them in a damping zone, %d failures\n", rows, typed, failures);
    if (typed == 0) {
        std::fprintf(stderr, "no row of the sweep lies in a damping zone\n");
        return 1;
    }
    return failures ? 1 : 0;
}
