// Philox4x32-10 (Salmon, Moraes, Dror, Shaw 2011, "Parallel random numbers: as easy as 1, 2, 3") and the standard
// normal deviate of the dust-diffusion kick.  Host and device, a stand-alone header: included by fcpt_kernels.hip
// (for kernels/particles.h) and by fcpt_host.cpp, which exports both functions so that tests need no device.
//
// Counter-based: the four output words depend only on (counter, key), so a particle's deviate is a function of
// (seed, id, step) and not of its slot, its lane or the number of steps taken since a restart:
//   counter = (id low, id high, step low, step high),  key = (seed low, seed high).
// Replaces fargo_random::get_std_normal (a host generator drawn in loop order, one stream per thread) of the
// reference's particles/dust_diffusion.cpp:89.
#ifndef FCPT_PHILOX_H
#define FCPT_PHILOX_H

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define FCPT_HD __host__ __device__ __forceinline__
#else
#define FCPT_HD inline
#endif

namespace fcpt {

// high word of the 32 x 32 -> 64 product
FCPT_HD uint32_t philox_mulhi(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32);
#endif
}

FCPT_HD void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    uint32_t k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = philox_mulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = philox_mulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u; // (the bump after the tenth round is unused)
        k1 += 0xBB67AE85u;
    }
    out[0] = c0;
    out[1] = c1;
    out[2] = c2;
    out[3] = c3;
}

// 52 bits of two words, centred in their cell: exact in FP64 and strictly inside (0, 1)
FCPT_HD double philox_unit(uint32_t hi, uint32_t lo)
{
    const uint64_t m = ((uint64_t)hi << 20) | (uint64_t)(lo >> 12);
    return ((double)m + 0.5) * 0x1p-52;
}

// Box-Muller, cosine branch; the sine partner is discarded.  u1 >= 2^-53, so |snv| <= sqrt(2 * 53 ln 2) = 8.57.
FCPT_HD double particle_std_normal(uint64_t seed, uint64_t id, uint64_t step)
{
    const uint32_t ctr[4] = {(uint32_t)id, (uint32_t)(id >> 32), (uint32_t)step, (uint32_t)(step >> 32)};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    const double u1 = philox_unit(w[0], w[1]), u2 = philox_unit(w[2], w[3]);
    return sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
}

} // namespace fcpt

#endif
