// Complex FP64 FFT of one row per workgroup: mixed-radix Stockham transform (radices 2, 3, 4, 5) with the whole row in LDS.
// Included by fcpt_selfgravity.hip (the kernels) and, for the plan alone, by fcpt_selfgravity_tables.cpp (no HIP).
//
// Departure from the reference, which hands its transforms to FFTW and so takes any length: a length must be 5-smooth
// and at most FFT_MAX_N = 8192 (16 bytes x 8192 = 128 KiB of the 160 KiB of LDS one workgroup may hold); anything else
// is refused by fft_plan() and, through it, by fcpt_selfgravity with FCPT_EINVAL and the length in the message.
//
// A stage of radix R on the row x[0 .. n) with n_cur = the length still to be transformed and s = n / n_cur the stride
// (product of the radices already done), butterfly t = q + s p of n / R (p < n_cur / R, q < s):
//   a_k = x[t + k n / R]                                  k < R   (every element is read by exactly one butterfly)
//   b_j = sum_k a_k exp(-2 pi i j k / R)
//   x[q + s (R p + j)] = b_j exp(-2 pi i j p / n_cur)     j < R   (every element is written by exactly one butterfly)
// All reads of a stage happen before all of its writes (a barrier between them), so one buffer serves: the values wait
// in registers.  After the last stage the row is in natural order.  The twiddle is sincospi of the fraction
// 2 ((j p) mod n_cur) / n_cur in FP64 -- never a recurrence, so the error of a transform is that of its log n stages.
// The inverse transform is conj(FFT(conj(x))), unnormalised: the conjugations ride in the load and the store.
#ifndef FCPT_KERNELS_FFT_H
#define FCPT_KERNELS_FFT_H

#include "../../../include/fargocpt_hip.h"

#define FFT_MAX_N FCPT_FFT_MAX_N /* 8192 */
#define FFT_MAX_STAGES 13 /* 2^13 = 8192 with radix 2 alone */
#define FFT_MAX_THREADS 1024

namespace fcpt {

struct FftPlan {
    int n;
    int nstages;
    int radix[FFT_MAX_STAGES];
    int threads; // of the workgroup: a multiple of 64 with n / (R threads) <= 8 / R for every radix R of the plan
};

// radices 4 first, then 2, 3, 5; false for n < 1, n > FFT_MAX_N or a prime factor above 5 (the plan is then untouched)
inline bool fft_plan(int n, FftPlan *out)
{
    if (n < 1 || n > FFT_MAX_N)
        return false;
    FftPlan p = {};
    p.n = n;
    int m = n;
    const int order[4] = {4, 2, 3, 5};
    for (int r : order)
        while (m % r == 0 && m > 1)
            p.radix[p.nstages++] = r, m /= r;
    if (m != 1)
        return false;
    int t = ((n + 7) / 8 + 63) / 64 * 64;
    p.threads = t < 64 ? 64 : t > FFT_MAX_THREADS ? FFT_MAX_THREADS : t;
    *out = p;
    return true;
}

#ifdef __HIPCC__

struct cplx {
    double x, y;
};
__device__ __forceinline__ cplx operator+(cplx a, cplx b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cplx operator-(cplx a, cplx b) { return {a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cplx cmul(cplx a, cplx b) { return {a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x}; }
__device__ __forceinline__ cplx mul_minus_i(cplx a) { return {a.y, -a.x}; }
__device__ __forceinline__ cplx cconj(cplx a) { return {a.x, -a.y}; }

// b_j = sum_k a_k exp(-2 pi i j k / R), in place
template <int R> __device__ __forceinline__ void fft_butterfly(cplx (&a)[R]);
template <> __device__ __forceinline__ void fft_butterfly<2>(cplx (&a)[2])
{
    const cplx b0 = a[0] + a[1], b1 = a[0] - a[1];
    a[0] = b0, a[1] = b1;
}
template <> __device__ __forceinline__ void fft_butterfly<4>(cplx (&a)[4])
{
    const cplx t0 = a[0] + a[2], t1 = a[0] - a[2], t2 = a[1] + a[3], t3 = mul_minus_i(a[1] - a[3]);
    a[0] = t0 + t2, a[1] = t1 + t3, a[2] = t0 - t2, a[3] = t1 - t3;
}
template <> __device__ __forceinline__ void fft_butterfly<3>(cplx (&a)[3])
{
    const double s = 0.86602540378443864676; // sin(2 pi / 3); cos(2 pi / 3) = -1/2
    const cplx t = a[1] + a[2], d = a[1] - a[2];
    const cplx m = {a[0].x - 0.5 * t.x, a[0].y - 0.5 * t.y};
    const cplx r = {s * d.y, -s * d.x}; // -i s d
    a[0] = a[0] + t, a[1] = m + r, a[2] = m - r;
}
template <> __device__ __forceinline__ void fft_butterfly<5>(cplx (&a)[5])
{
    const double c1 = 0.30901699437494742410, s1 = 0.95105651629515357212;  // cos, sin (2 pi / 5)
    const double c2 = -0.80901699437494742410, s2 = 0.58778525229247312917; // cos, sin (4 pi / 5)
    const cplx t1 = a[1] + a[4], t2 = a[2] + a[3], d1 = a[1] - a[4], d2 = a[2] - a[3];
    const cplx m1 = {a[0].x + c1 * t1.x + c2 * t2.x, a[0].y + c1 * t1.y + c2 * t2.y};
    const cplx m2 = {a[0].x + c2 * t1.x + c1 * t2.x, a[0].y + c2 * t1.y + c1 * t2.y};
    const cplx e1 = {s1 * d1.x + s2 * d2.x, s1 * d1.y + s2 * d2.y};
    const cplx e2 = {s2 * d1.x - s1 * d2.x, s2 * d1.y - s1 * d2.y};
    const cplx r1 = mul_minus_i(e1), r2 = mul_minus_i(e2);
    a[0] = a[0] + t1 + t2, a[1] = m1 + r1, a[4] = m1 - r1, a[2] = m2 + r2, a[3] = m2 - r2;
}

// exp(-2 pi i num / den), 0 <= num < den
__device__ __forceinline__ cplx fft_twiddle(int num, int den)
{
    double s, c;
    sincospi(2.0 * (double)num / (double)den, &s, &c);
    return {c, -s};
}

// one stage on the row in LDS; every thread of the workgroup calls it (it holds two barriers)
template <int R> __device__ __forceinline__ void fft_stage(cplx *x, int n, int n_cur, int s)
{
    constexpr int MAXB = (8 + R - 1) / R; // butterflies per thread at the most (FftPlan::threads)
    const int nb = n / R, T = (int)blockDim.x, tid = (int)threadIdx.x;
    cplx v[MAXB][R];
#pragma unroll
    for (int b = 0; b < MAXB; ++b) {
        const int t = tid + b * T;
        if (t < nb) {
#pragma unroll
            for (int k = 0; k < R; ++k)
                v[b][k] = x[t + k * nb];
        }
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < MAXB; ++b) {
        const int t = tid + b * T;
        if (t < nb) {
            const int p = t / s, q = t - p * s;
            fft_butterfly<R>(v[b]);
            cplx *y = x + q + s * R * p;
            y[0] = v[b][0];
#pragma unroll
            for (int j = 1; j < R; ++j)
                y[s * j] = cmul(v[b][j], fft_twiddle((int)(((long long)j * p) % n_cur), n_cur));
        }
    }
    __syncthreads();
}

// the forward transform of the row in LDS (all threads; the row must be complete and a barrier passed)
__device__ __forceinline__ void fft_row(cplx *x, const FftPlan &plan)
{
    int n_cur = plan.n, s = 1;
    for (int st = 0; st < plan.nstages; ++st) {
        const int r = plan.radix[st];
        if (r == 4)
            fft_stage<4>(x, plan.n, n_cur, s);
        else if (r == 2)
            fft_stage<2>(x, plan.n, n_cur, s);
        else if (r == 3)
            fft_stage<3>(x, plan.n, n_cur, s);
        else
            fft_stage<5>(x, plan.n, n_cur, s);
        n_cur /= r;
        s *= r;
    }
}

#endif // __HIPCC__
} // namespace fcpt
#endif
