// Kernels of the self-gravity solver (selfgravity.cpp:321-416, 520-703, 712-747).  Part of fcpt_selfgravity.hip: included
// once, after fcpt_selfgravity.h and kernels/fft.h.
//
// One evaluation, with Z = S_r + i S_t (both real, so one complex transform does the work of two real ones; the two
// spectra are separated by Hermitian symmetry in k_sg_multiply):
//   k_sg_fft_rows<LOAD_SIGMA>   rows of the density -> packed, transformed along phi            -> A  (nr x nphi)
//   k_sg_transpose              A -> B (nphi x nr): the radial direction becomes contiguous
//   k_sg_fft_rows<LOAD_PAD>     rows of B, zero-padded to 2 nr, transformed                      -> C  (nphi x 2 nr)
//   k_sg_multiply               C <- -G (K_r^ S_r^ + i K_t^ S_t^), in place, pairs (k, -k)
//   k_sg_fft_rows<LOAD_CONJ>    rows of C, inverse; only the lower nr results are stored         -> B
//   k_sg_transpose              B -> A
//   k_sg_fft_rows<STORE_ACCEL>  rows of A, inverse along phi, ring weights                       -> g_r, g_phi
// (the two inverse passes are conj(FFT(conj .))): the conjugations between them cancel, one is left at each end)

enum { SG_LOAD_PLAIN = 0, SG_LOAD_SIGMA = 1, SG_LOAD_CONJ = 2, SG_LOAD_REAL_PAIR = 3 };
enum { SG_STORE_PLAIN = 0, SG_STORE_ACCEL = 1 };

struct SgFftArgs {
    FftPlan plan;
    int rows;
    // SG_LOAD_PLAIN / _CONJ: `in` holds rows of in_stride complex numbers of which the first n_in are read, the rest of the
    // row counts as zero; SG_LOAD_SIGMA: `in` is the density (rows of n doubles); SG_LOAD_REAL_PAIR: in and in2 are two real
    // tables (rows of n doubles), the row becomes in + i in2
    const double *in, *in2;
    int n_in, in_stride;
    // SG_STORE_PLAIN: the first n_out results to rows of out_stride complex numbers; SG_STORE_ACCEL: Re and -Im, times the
    // ring weights, to the two grids (rows of n doubles)
    double *out, *out2;
    int n_out, out_stride;
    const double *sqrt_ratio, *norm_r, *norm_t; // per ring
    CArr Rmed;
    double rmed0;
};

template <int LOAD, int STORE> __global__ void __launch_bounds__(FFT_MAX_THREADS) k_sg_fft_rows(const SgFftArgs a)
{
    extern __shared__ double sg_lds[];
    cplx *x = (cplx *)sg_lds;
    const int row = (int)blockIdx.x, n = a.plan.n, T = (int)blockDim.x, tid = (int)threadIdx.x;
    if (row >= a.rows)
        return;
    if (LOAD == SG_LOAD_SIGMA) {
        // S_r = sigma sqrt(Rmed / Rmed[0]), S_t = S_r Rmed / Rmed[0] (selfgravity.cpp:356-358)
        const double w = a.sqrt_ratio[row], rm = a.Rmed[row];
        for (int j = tid; j < n; j += T) {
            const double s_r = a.in[(size_t)row * n + j] * w;
            x[j] = {s_r, s_r * rm / a.rmed0};
        }
    } else if (LOAD == SG_LOAD_REAL_PAIR) {
        for (int j = tid; j < n; j += T)
            x[j] = {a.in[(size_t)row * n + j], a.in2[(size_t)row * n + j]};
    } else {
        const cplx *src = (const cplx *)a.in + (size_t)row * a.in_stride;
        for (int j = tid; j < n; j += T) {
            cplx v = {0.0, 0.0};
            if (j < a.n_in)
                v = src[j];
            x[j] = LOAD == SG_LOAD_CONJ ? cconj(v) : v;
        }
    }
    __syncthreads();
    fft_row(x, a.plan);
    if (STORE == SG_STORE_ACCEL) {
        const double nr_ = a.norm_r[row], nt_ = a.norm_t[row];
        for (int j = tid; j < n; j += T) {
            a.out[(size_t)row * n + j] = x[j].x * nr_;
            a.out2[(size_t)row * n + j] = -x[j].y * nt_;
        }
    } else {
        cplx *dst = (cplx *)a.out + (size_t)row * a.out_stride;
        for (int j = tid; j < a.n_out; j += T)
            dst[j] = x[j];
    }
}

// out (cols x rows) = in (rows x cols) transposed, complex; 32 x 32 tiles through LDS, 32 x 8 threads
#define SG_TILE 32
__global__ void __launch_bounds__(256) k_sg_transpose(const double *in_, double *out_, int rows, int cols)
{
    __shared__ cplx tile[SG_TILE][SG_TILE + 1];
    const cplx *in = (const cplx *)in_;
    cplx *out = (cplx *)out_;
    const int c0 = (int)blockIdx.x * SG_TILE, r0 = (int)blockIdx.y * SG_TILE;
    const int tx = (int)threadIdx.x, ty = (int)threadIdx.y;
    for (int k = ty; k < SG_TILE; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        if (r < rows && c < cols)
            tile[k][tx] = in[(size_t)r * cols + c];
    }
    __syncthreads();
    for (int k = ty; k < SG_TILE; k += 8) {
        const int c = c0 + k, r = r0 + tx; // row c of the output, column r
        if (r < rows && c < cols)
            out[(size_t)c * rows + r] = tile[tx][k];
    }
}

// The spectra of the two real fields out of the spectrum Z^ of S_r + i S_t, element a = (k, m) with its partner
// b = (-k mod nphi, -m mod n2):  S_r^(a) = (Z^(a) + conj Z^(b)) / 2,  S_t^(a) = (Z^(a) - conj Z^(b)) / (2 i),
// likewise K_r^ and K_t^ out of the spectrum of K_r + i K_t.  With P_r = K_r^ S_r^ and P_t = K_t^ S_t^ at a (selfgravity.cpp:
// 534-548) the spectrum of g_r + i g_phi is -G (P_r + i P_t) at a and -G (conj P_r + i conj P_t) at b.  One thread per pair (the
// element with the lower index acts), in place.
__global__ void __launch_bounds__(256) k_sg_multiply(double *C_, const double *KC_, int nphi, int n2, double minus_G)
{
    cplx *C = (cplx *)C_;
    const cplx *KC = (const cplx *)KC_;
    const size_t total = (size_t)nphi * n2;
    const size_t ia = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ia >= total)
        return;
    const int k = (int)(ia / n2), m = (int)(ia - (size_t)k * n2);
    const int kb = k ? nphi - k : 0, mb = m ? n2 - m : 0;
    const size_t ib = (size_t)kb * n2 + mb;
    if (ib < ia)
        return;
    const cplx za = C[ia], zb = cconj(C[ib]), ka = KC[ia], kb_ = cconj(KC[ib]);
    const cplx s_r = {0.5 * (za.x + zb.x), 0.5 * (za.y + zb.y)};
    const cplx s_t = {0.5 * (za.y - zb.y), -0.5 * (za.x - zb.x)}; // -i / 2 (za - zb)
    const cplx k_r = {0.5 * (ka.x + kb_.x), 0.5 * (ka.y + kb_.y)};
    const cplx k_t = {0.5 * (ka.y - kb_.y), -0.5 * (ka.x - kb_.x)};
    const cplx p_r = cmul(k_r, s_r), p_t = cmul(k_t, s_t);
    // P_r + i P_t and conj P_r + i conj P_t
    C[ia] = {minus_G * (p_r.x - p_t.y), minus_G * (p_r.y + p_t.x)};
    if (ib != ia)
        C[ib] = {minus_G * (p_r.x + p_t.y), minus_G * (p_t.x - p_r.y)};
}

// update_velocities (selfgravity.cpp:712-747) in place, the step length from the device clock (from_clock) or the argument:
// every IEEE operation as the reference writes it, no contraction, so the kick has the bits of the plain expression
__global__ void __launch_bounds__(256) k_sg_kick(const Dev P, const double *g_r, const double *g_t, const DevClock *clk,
                                                 double dt_arg, int from_clock)
{
#pragma clang fp contract(off)
    const int nphi = P.nphi;
    const size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= (size_t)P.nr * nphi)
        return;
    const int i = (int)(l / nphi), j = (int)(l - (size_t)i * nphi);
    const double dt = from_clock ? clk->dt : dt_arg;
    if (i > 0)
        P.vrad[l] += dt * ((P.Rinf[i] - P.Rmed[i - 1]) * g_r[l] + (P.Rmed[i] - P.Rinf[i]) * g_r[l - nphi]) * P.InvDiffRmed[i];
    const size_t lm1 = (size_t)i * nphi + (j == 0 ? nphi - 1 : j - 1);
    P.vazi[l] += 0.5 * dt * (g_t[l] + g_t[lm1]);
}
