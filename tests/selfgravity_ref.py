"""numpy restatement of the reference's self-gravity solver (src/selfgravity.cpp) in the modes basic and symmetric, in two
forms: `sg_direct` evaluates the discrete convolution of compute_FFT_density / compute_acceleration as an O(N^2) sum and
contains no FFT -- it is the truth the HIP solver is held to --, `sg_fft` is the same convolution through numpy.fft, for
grids on which the sum would be too long (the reference's own 128 x 256 known answer).  Plus update_velocities and
init_azimuthal_velocity.  Plain numpy, no GPU.

Conventions: `radii` are the global interface radii (Library.radii), Nr = the number of rings, ghost rings included; a
grid is [Nr, Nphi] (v_r: [Nr + 1, Nphi])."""
from __future__ import annotations

import numpy as np

BASIC, SYMMETRIC = 1, 2


def geometry(radii, nr):
    """(Rinf, Rmed) of rings 0 .. nr-1 (src/init.cpp:147-190)."""
    ri, rs = np.asarray(radii[:nr], dtype=float), np.asarray(radii[1:nr + 1], dtype=float)
    rmed = 2.0 / 3.0 * (rs * rs * rs - ri * ri * ri)
    rmed = rmed / (rs * rs - ri * ri)
    return ri, rmed


def kernel_tables(radii, nr, nphi, mode, aspect_ratio, thickness_smoothing_sg=0.0):
    """(K_radial, K_azimuthal), [2 Nr, Nphi] each: compute_FFT_kernel (:418-518) with update_sg_constants (:171-179)."""
    radii = np.asarray(radii, dtype=float)
    h = aspect_ratio
    i = np.arange(2 * nr)
    u = np.where(i < nr, np.log(radii[np.minimum(i, nr)] / radii[0]), -np.log(radii[2 * nr - np.maximum(i, nr)] / radii[0]))[:, None]
    theta = (2.0 * np.pi / nphi * np.arange(nphi))[None, :]
    if mode == SYMMETRIC:
        lambda_sq = (0.4571 * h + 0.6737 * np.sqrt(h)) ** 2
        chi_sq = ((-0.7543 * h + 0.6472) * h) ** 2
        den = (2 * (np.cosh(u) - np.cos(theta)) + lambda_sq * (np.exp(u) + np.exp(-u) - 2) + chi_sq) ** -1.5
        kr = (1.0 - np.cos(theta) * np.exp(-u)) * den
    elif mode == BASIC:
        eps = thickness_smoothing_sg * h
        den = (eps * eps * np.exp(u) + 2.0 * (np.cosh(u) - np.cos(theta))) ** -1.5
        kr = (1.0 + eps * eps - np.cos(theta) * np.exp(-u)) * den
    else:
        raise ValueError(mode)
    kt = np.sin(theta) * den
    return kr, kt


def reduced_density(sigma, rmed):
    """(S_r, S_t) of compute_FFT_density (:356-358)."""
    s_r = sigma * np.sqrt(rmed / rmed[0])[:, None]
    s_t = s_r * rmed[:, None] / rmed[0]
    return s_r, s_t


def ring_norms(radii, nr, nphi, rmed):
    """The weights of the convolution sum per ring: normaccr and normacct of :673-683 without their 1 / (2 Nr Nphi), which
    only undoes the factor an unnormalised transform pair leaves: r_step t_step / sqrt(Rmed / Rmed[0]) (g_phi: / (..)^1.5)."""
    r_step = np.log(radii[nr] / radii[0]) / nr
    t_step = 2.0 * np.pi / nphi
    base = r_step * t_step
    ratio = rmed / rmed[0]
    return base / np.sqrt(ratio), base / (ratio * np.sqrt(ratio))


def sg_direct(sigma, radii, mode, aspect_ratio, thickness_smoothing_sg=0.0, G=1.0):
    """(g_r, g_phi) [Nr, Nphi] by the plain double sum over all source cells -- no transform anywhere:
    g(i, j) = -G norm(i) sum_{i', j'} K[(i - i') mod 2 Nr, (j - j') mod Nphi] S(i', j'), i' < Nr (the padding rows are zero)."""
    nr, nphi = sigma.shape
    _, rmed = geometry(radii, nr)
    kr, kt = kernel_tables(radii, nr, nphi, mode, aspect_ratio, thickness_smoothing_sg)
    s_r, s_t = reduced_density(sigma, rmed)
    di = (np.arange(nr)[:, None] - np.arange(nr)[None, :]) % (2 * nr)          # [i, i']
    dj = (np.arange(nphi)[:, None] - np.arange(nphi)[None, :]) % nphi          # [j, j']
    g_r, g_t = np.zeros((nr, nphi)), np.zeros((nr, nphi))
    for i in range(nr):   # [j, i', j'] at a time
        g_r[i] = np.einsum("jkl,kl->j", kr[di[i][None, :, None], dj[:, None, :]], s_r)
        g_t[i] = np.einsum("jkl,kl->j", kt[di[i][None, :, None], dj[:, None, :]], s_t)
    nrm_r, nrm_t = ring_norms(radii, nr, nphi, rmed)
    return -G * g_r * nrm_r[:, None], -G * g_t * nrm_t[:, None]


def sg_fft(sigma, radii, mode, aspect_ratio, thickness_smoothing_sg=0.0, G=1.0):
    """The same convolution through numpy.fft on the zero-padded [2 Nr, Nphi] arrays, as the reference does with FFTW."""
    nr, nphi = sigma.shape
    _, rmed = geometry(radii, nr)
    kr, kt = kernel_tables(radii, nr, nphi, mode, aspect_ratio, thickness_smoothing_sg)
    pad = np.zeros((2 * nr, nphi)), np.zeros((2 * nr, nphi))
    pad[0][:nr], pad[1][:nr] = reduced_density(sigma, rmed)
    acc_r = np.fft.irfft2(-G * np.fft.rfft2(kr) * np.fft.rfft2(pad[0]), s=(2 * nr, nphi))[:nr]
    acc_t = np.fft.irfft2(-G * np.fft.rfft2(kt) * np.fft.rfft2(pad[1]), s=(2 * nr, nphi))[:nr]
    nrm_r, nrm_t = ring_norms(radii, nr, nphi, rmed)
    # (irfft2 divides by 2 Nr Nphi, as the reference's norm does after FFTW's unnormalised pair)
    return acc_r * nrm_r[:, None], acc_t * nrm_t[:, None]


def weighted_kernel(radii, nr, nphi, mode, aspect_ratio, thickness_smoothing_sg, i0, j0, amplitude, G=1.0):
    """(g_r, g_phi) of a density that is `amplitude` in cell (i0, j0) and zero elsewhere: the kernel tables read off at
    (i - i0, j - j0) with the source's and the ring's weights -- a known answer without any sum."""
    _, rmed = geometry(radii, nr)
    kr, kt = kernel_tables(radii, nr, nphi, mode, aspect_ratio, thickness_smoothing_sg)
    s_r = amplitude * np.sqrt(rmed[i0] / rmed[0])
    s_t = s_r * rmed[i0] / rmed[0]
    rows = (np.arange(nr) - i0) % (2 * nr)
    cols = (np.arange(nphi) - j0) % nphi
    nrm_r, nrm_t = ring_norms(radii, nr, nphi, rmed)
    return (-G * kr[rows][:, cols] * s_r * nrm_r[:, None], -G * kt[rows][:, cols] * s_t * nrm_t[:, None])


def kick(vrad, vazi, g_r, g_t, radii, dt):
    """update_velocities (:712-747): new (v_r, v_phi), every operation in the reference's order."""
    nr, nphi = vazi.shape
    rinf, rmed = geometry(radii, nr)
    inv_diff = np.zeros(nr)
    inv_diff[1:] = 1.0 / (rmed[1:] - rmed[:-1])
    vr, va = vrad.copy(), vazi.copy()
    w_hi = (rinf[1:] - rmed[:-1])[:, None]
    w_lo = (rmed[1:] - rinf[1:])[:, None]
    vr[1:nr] += dt * (w_hi * g_r[1:] + w_lo * g_r[:-1]) * inv_diff[1:, None]
    va += 0.5 * dt * (g_t + np.roll(g_t, 1, axis=1))
    return vr, va


def init_azimuthal_velocity(g_r, radii, omega_cell):
    """init_azimuthal_velocity (:749-781): v_phi per ring from the ring means of g_r and the angular velocity `omega_cell`
    [Nr] the disk would have without self-gravity: Rmed sqrt(omega_cell^2 - <g_r> / Rmed)."""
    nr = g_r.shape[0]
    _, rmed = geometry(radii, nr)
    return rmed * np.sqrt(omega_cell ** 2 - g_r.mean(axis=1) / rmed)
