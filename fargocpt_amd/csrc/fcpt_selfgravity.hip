// Self-gravity of the gas (include/fargocpt_hip.h, "self-gravity of the gas"): the polar convolution of selfgravity.cpp with
// the library's own FFT (kernels/fft.h), the kick, and their entry points.  What needs no device -- refusals, transform
// plans, kernel tables, ring weights -- is fcpt_selfgravity_tables.cpp's.
#include "fcpt_ctx.h"

using namespace fcpt;

namespace fcpt {
#include "kernels/selfgravity.h"
} // namespace fcpt

namespace {

#define SG_LAUNCH(id, kernel, grid, block, lds, st, ...)                     \
    do {                                                                     \
        if (g_prof)                                                          \
            g_prof->begin((id), st);                                         \
        hipLaunchKernelGGL(kernel, (grid), (block), (lds), st, __VA_ARGS__); \
        if (g_prof)                                                          \
            g_prof->end((id), st);                                           \
    } while (0)

template <int LOAD, int STORE> void launch_fft_rows(const SgFftArgs &a, hipStream_t st)
{
    if (a.rows <= 0)
        return;
    const size_t lds = (size_t)a.plan.n * 2 * sizeof(double);
    SG_LAUNCH(KID_SG_FFT_ROWS, (k_sg_fft_rows<LOAD, STORE>), dim3(a.rows), dim3(a.plan.threads), lds, st, a);
}

// a row of more than 4096 complex numbers needs more than the 64 KiB of dynamic LDS a kernel may ask for unprepared
template <int LOAD, int STORE> hipError_t allow_lds(size_t bytes)
{
    if (bytes <= 65536)
        return hipSuccess;
    return hipFuncSetAttribute((const void *)k_sg_fft_rows<LOAD, STORE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
hipError_t allow_lds_all(int n)
{
    const size_t bytes = (size_t)n * 2 * sizeof(double);
    hipError_t e = allow_lds<SG_LOAD_SIGMA, SG_STORE_PLAIN>(bytes);
    if (e == hipSuccess)
        e = allow_lds<SG_LOAD_PLAIN, SG_STORE_PLAIN>(bytes);
    if (e == hipSuccess)
        e = allow_lds<SG_LOAD_CONJ, SG_STORE_PLAIN>(bytes);
    if (e == hipSuccess)
        e = allow_lds<SG_LOAD_PLAIN, SG_STORE_ACCEL>(bytes);
    if (e == hipSuccess)
        e = allow_lds<SG_LOAD_REAL_PAIR, SG_STORE_PLAIN>(bytes);
    return e;
}

void launch_transpose(const double *in, double *out, int rows, int cols, hipStream_t st)
{
    const dim3 grid((cols + SG_TILE - 1) / SG_TILE, (rows + SG_TILE - 1) / SG_TILE);
    SG_LAUNCH(KID_SG_TRANSPOSE, k_sg_transpose, grid, dim3(SG_TILE, 8), 0, st, in, out, rows, cols);
}

template <class T> int sg_alloc(fcpt_ctx *c, T **p, size_t n)
{
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, n * sizeof(T));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("fcpt_selfgravity: hipMalloc(%zu bytes) failed: %s", n * sizeof(T), hipGetErrorString(e));
        return FCPT_ENOMEM;
    }
    c->sg_allocs.push_back(q);
    *p = (T *)q;
    return FCPT_OK;
}

} // namespace

namespace fcpt {

void selfgravity_free(fcpt_ctx *c)
{
    for (void *p : c->sg_allocs)
        (void)hipFree(p);
    c->sg_allocs.clear();
    std::memset(&c->sg, 0, sizeof(c->sg));
    c->sg_params = {0, 0, 0.0, 0.0};
    c->ls.selfgravity = false;
    c->grid[FCPT_F_SG_ACCEL_RAD] = nullptr;
    c->grid[FCPT_F_SG_ACCEL_AZI] = nullptr;
}

// compute_FFT_density + compute_acceleration (selfgravity.cpp:321-416, 520-703) from the density of the view
void enqueue_selfgravity_compute(fcpt_ctx *c, const Dev &P)
{
    const SgDev &S = c->sg;
    hipStream_t st = c->stream;
    const int nr = S.nr, nphi = S.nphi, n2 = 2 * S.nr;
    SgFftArgs a = {};
    a.sqrt_ratio = S.sqrt_ratio, a.norm_r = S.norm_r, a.norm_t = S.norm_t, a.Rmed = P.Rmed, a.rmed0 = S.rmed0;
    // density -> packed, along phi -> A
    a.plan = S.plan_phi, a.rows = nr, a.in = P.sigma, a.out = S.A, a.n_out = nphi, a.out_stride = nphi;
    launch_fft_rows<SG_LOAD_SIGMA, SG_STORE_PLAIN>(a, st);
    launch_transpose(S.A, S.B, nr, nphi, st);
    // rows of B padded with zeros to 2 nr -> C
    a.plan = S.plan_rad, a.rows = nphi, a.in = S.B, a.n_in = nr, a.in_stride = nr, a.out = S.C, a.n_out = n2, a.out_stride = n2;
    launch_fft_rows<SG_LOAD_PLAIN, SG_STORE_PLAIN>(a, st);
    {
        const size_t total = (size_t)nphi * n2;
        SG_LAUNCH(KID_SG_MULTIPLY, k_sg_multiply, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, S.C, (const double *)S.KC,
                  nphi, n2, S.minus_G);
    }
    // back: rows of C, of which only the lower nr results are needed -> B
    a.in = S.C, a.n_in = n2, a.in_stride = n2, a.out = S.B, a.n_out = nr, a.out_stride = nr;
    launch_fft_rows<SG_LOAD_CONJ, SG_STORE_PLAIN>(a, st);
    launch_transpose(S.B, S.A, nphi, nr, st);
    a.plan = S.plan_phi, a.rows = nr, a.in = S.A, a.n_in = nphi, a.in_stride = nphi;
    a.out = c->grid[FCPT_F_SG_ACCEL_RAD], a.out2 = c->grid[FCPT_F_SG_ACCEL_AZI];
    launch_fft_rows<SG_LOAD_PLAIN, SG_STORE_ACCEL>(a, st);
}

void enqueue_selfgravity_kick(fcpt_ctx *c, const Dev &P, bool dt_from_clock, double dt)
{
    enqueue_selfgravity_compute(c, P);
    hipStream_t st = c->stream;
    const size_t cells = (size_t)P.nr * P.nphi;
    SG_LAUNCH(KID_SG_KICK, k_sg_kick, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, P,
              (const double *)c->grid[FCPT_F_SG_ACCEL_RAD], (const double *)c->grid[FCPT_F_SG_ACCEL_AZI], (const DevClock *)P.clk, dt,
              dt_from_clock ? 1 : 0);
}

} // namespace fcpt

extern "C" {

int fcpt_selfgravity(fcpt_ctx *c, const fcpt_selfgravity_params *p)
{
    if (!c || !p) {
        set_error("null argument");
        return FCPT_EINVAL;
    }
    FftPlan plan_phi = {}, plan_rad = {};
    if (p->mode != FCPT_SG_OFF) { // a refused call changes nothing
        if (int rc = sg_validate(c->d, *p, &plan_phi, &plan_rad))
            return rc;
        if (c->s.nr != c->d.nr_global) {
            set_error("fcpt_selfgravity: the context holds %d of %d rings; self-gravity runs on one slab only", c->s.nr, c->d.nr_global);
            return FCPT_EINVAL;
        }
    }
    join_side(c);
    HIPCHK(hipStreamSynchronize(c->stream));
    drop_graph(c); // its launches were chosen without (or with the buffers of) the self-gravity that is about to go
    selfgravity_free(c);
    if (p->mode == FCPT_SG_OFF)
        return FCPT_OK;

    const int nr = c->s.nr, nphi = c->d.nphi, n2 = 2 * nr;
    const size_t cells = (size_t)nr * nphi;
    SgDev &S = c->sg;
    S.nr = nr, S.nphi = nphi, S.plan_phi = plan_phi, S.plan_rad = plan_rad;
    S.rmed0 = c->geo.Rmed[0];
    S.minus_G = -c->d.G;
    SgRingWeights w;
    sg_ring_weights(c->d, c->radii.data(), c->geo, nr, w);
    std::vector<double> kr, kt;
    try {
        kr.resize(2 * cells), kt.resize(2 * cells);
    } catch (const std::bad_alloc &) {
        set_error("fcpt_selfgravity: no host memory for the kernel tables (%zu bytes)", 4 * cells * sizeof(double));
        return FCPT_ENOMEM;
    }
    sg_kernel_tables(c->d, c->radii.data(), *p, kr.data(), kt.data());

    double *wts = nullptr, *g_r = nullptr, *g_t = nullptr;
    int rc = sg_alloc(c, &S.A, 2 * cells);
    rc = rc ? rc : sg_alloc(c, &S.B, 2 * cells);
    rc = rc ? rc : sg_alloc(c, &S.C, 4 * cells);
    rc = rc ? rc : sg_alloc(c, &S.KC, 4 * cells);
    rc = rc ? rc : sg_alloc(c, &g_r, cells);
    rc = rc ? rc : sg_alloc(c, &g_t, cells);
    rc = rc ? rc : sg_alloc(c, &wts, (size_t)3 * nr);
    hipError_t e = hipSuccess;
    if (!rc) {
        e = allow_lds_all(nphi > n2 ? nphi : n2);
        if (e == hipSuccess)
            e = hipMemset(g_r, 0, cells * sizeof(double));
        if (e == hipSuccess)
            e = hipMemset(g_t, 0, cells * sizeof(double));
        if (e == hipSuccess)
            e = hipMemcpy(wts, w.sqrt_ratio.data(), nr * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(wts + nr, w.norm_r.data(), nr * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(wts + 2 * nr, w.norm_t.data(), nr * sizeof(double), hipMemcpyHostToDevice);
        // the two real tables side by side in C (2 nr x nphi doubles each)
        if (e == hipSuccess)
            e = hipMemcpy(S.C, kr.data(), 2 * cells * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = hipMemcpy(S.C + 2 * cells, kt.data(), 2 * cells * sizeof(double), hipMemcpyHostToDevice);
    }
    if (!rc && e == hipSuccess) {
        S.sqrt_ratio = wts, S.norm_r = wts + nr, S.norm_t = wts + 2 * nr;
        ProfScope prof_scope(c);
        hipStream_t st = c->stream;
        // the spectrum of K_radial + i K_azimuthal, once: along phi -> KC (2 nr x nphi), transposed -> C, along r in place -> KC
        SgFftArgs a = {};
        a.plan = plan_phi, a.rows = n2, a.in = S.C, a.in2 = S.C + 2 * cells, a.out = S.KC, a.n_out = nphi, a.out_stride = nphi;
        launch_fft_rows<SG_LOAD_REAL_PAIR, SG_STORE_PLAIN>(a, st);
        launch_transpose(S.KC, S.C, n2, nphi, st);
        a.plan = plan_rad, a.rows = nphi, a.in = S.C, a.in2 = nullptr, a.n_in = n2, a.in_stride = n2, a.out = S.C, a.n_out = n2,
        a.out_stride = n2;
        launch_fft_rows<SG_LOAD_PLAIN, SG_STORE_PLAIN>(a, st);
        e = hipGetLastError();
        if (e == hipSuccess)
            e = hipMemcpyAsync(S.KC, S.C, 4 * cells * sizeof(double), hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess)
            e = hipStreamSynchronize(st);
    }
    if (rc || e != hipSuccess) {
        if (!rc) {
            set_error("fcpt_selfgravity: building the kernel spectra failed: %s", hipGetErrorString(e));
            rc = FCPT_EHIP;
        }
        (void)hipGetLastError();
        selfgravity_free(c);
        return rc;
    }
    c->grid[FCPT_F_SG_ACCEL_RAD] = g_r;
    c->grid[FCPT_F_SG_ACCEL_AZI] = g_t;
    c->sg_params = *p;
    c->sg_params.in_step = p->in_step ? 1 : 0;
    c->ls.selfgravity = p->in_step != 0;
    return FCPT_OK;
}

int fcpt_selfgravity_get(fcpt_ctx *c, fcpt_selfgravity_params *out)
{
    if (!c || !out)
        return FCPT_EINVAL;
    *out = c->sg_params;
    return FCPT_OK;
}

static int sg_require(fcpt_ctx *c, const char *who)
{
    if (!c)
        return FCPT_EINVAL;
    if (c->sg_params.mode == FCPT_SG_OFF) {
        set_error("%s: self-gravity is switched off (fcpt_selfgravity)", who);
        return FCPT_EINVAL;
    }
    return FCPT_OK;
}

int fcpt_selfgravity_compute(fcpt_ctx *c)
{
    if (int rc = sg_require(c, "fcpt_selfgravity_compute"))
        return rc;
    join_side(c);
    ProfScope prof_scope(c);
    enqueue_selfgravity_compute(c, c->P);
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_selfgravity_kick(fcpt_ctx *c, double dt)
{
    if (int rc = sg_require(c, "fcpt_selfgravity_kick"))
        return rc;
    join_side(c);
    ProfScope prof_scope(c);
    enqueue_selfgravity_kick(c, c->P, false, dt);
    c->ls.cfl_interior = false; // the velocities changed
    HIPCHK(hipGetLastError());
    return FCPT_OK;
}

int fcpt_selftest_fft(int32_t rows, int32_t n, int32_t inverse, double *interleaved)
{
    FftPlan plan;
    if (rows < 1 || !interleaved) {
        set_error("fcpt_selftest_fft: rows < 1 or a null array");
        return FCPT_EINVAL;
    }
    if (!fft_plan(n, &plan)) {
        set_error("transform length %d is refused: a length must be in 1 .. %d and have no prime factor above 5", n, FFT_MAX_N);
        return FCPT_EINVAL;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        set_error("no HIP device available");
        return FCPT_ENODEV;
    }
    const size_t bytes = (size_t)rows * n * 2 * sizeof(double);
    double *buf = nullptr;
    if (hipMalloc((void **)&buf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("fcpt_selftest_fft: hipMalloc(%zu bytes) failed", bytes);
        return FCPT_ENOMEM;
    }
    hipError_t e = allow_lds_all(n);
    if (e == hipSuccess)
        e = hipMemcpy(buf, interleaved, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        SgFftArgs a = {};
        a.plan = plan, a.rows = rows, a.in = buf, a.n_in = n, a.in_stride = n, a.out = buf, a.n_out = n, a.out_stride = n;
        if (inverse)
            launch_fft_rows<SG_LOAD_CONJ, SG_STORE_PLAIN>(a, nullptr); // conj(FFT(conj x)): the last conjugation below, on the host
        else
            launch_fft_rows<SG_LOAD_PLAIN, SG_STORE_PLAIN>(a, nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess)
        e = hipMemcpy(interleaved, buf, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(buf);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_error("fcpt_selftest_fft failed: %s", hipGetErrorString(e));
        return FCPT_EHIP;
    }
    if (inverse)
        for (size_t k = 0; k < (size_t)rows * n; ++k)
            interleaved[2 * k + 1] = -interleaved[2 * k + 1];
    return FCPT_OK;
}

} // extern "C"
