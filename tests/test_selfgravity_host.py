"""Self-gravity without a GPU: the numpy restatement against itself (plain sum against numpy.fft), against the reference's
own known answer (test/self_gravity: the direct sum of Newton's law over a 128 x 256 disk), and the host-side stages of the
library -- kernel tables and transform plans -- against numpy."""
import os

import numpy as np
import pytest

from fargocpt_amd import binding as B, setups

from tests import selfgravity_ref as R

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "self_gravity_gr_direct_128x256.txt")
SHAPES = [(16, 24), (20, 30)]          # transform lengths 32, 24 (radices 2, 3, 4) and 40, 30 (radix 5 too)
MODES = [(R.BASIC, "basic"), (R.SYMMETRIC, "symmetric")]


def small_grid(lib, nr, nphi):
    d = setups.planet_disk(lib, nr, nphi)
    return d, lib.radii(d)


def random_sigma(nr, nphi, seed):
    return np.random.default_rng(seed).uniform(0.5, 1.5, size=(nr, nphi))


@pytest.mark.parametrize("mode,name", MODES)
@pytest.mark.parametrize("nr,nphi", SHAPES)
def test_direct_sum_agrees_with_numpy_fft(product, nr, nphi, mode, name):
    d, radii = small_grid(product, nr, nphi)
    sigma = random_sigma(nr, nphi, 7 * nr + nphi)
    a = R.sg_direct(sigma, radii, mode, 0.05, 0.6)
    b = R.sg_fft(sigma, radii, mode, 0.05, 0.6)
    for x, y, what in zip(a, b, ("g_r", "g_phi")):
        err = np.abs(x - y).max() / np.abs(x).max()
        print(f"{nr}x{nphi} {name} {what}: direct against numpy.fft {err:.3e}")
        assert err <= 1e-13


def test_planted_delta_is_the_weighted_kernel(product):
    """The known answer the GPU test uses, held to the plain sum first."""
    nr, nphi = 16, 24
    d, radii = small_grid(product, nr, nphi)
    for i0, j0 in ((0, 0), (nr - 1, nphi - 1), (5, 7)):
        sigma = np.zeros((nr, nphi))
        sigma[i0, j0] = 1.25
        a = R.sg_direct(sigma, radii, R.SYMMETRIC, 0.05)
        b = R.weighted_kernel(radii, nr, nphi, R.SYMMETRIC, 0.05, 0.0, i0, j0, 1.25)
        for x, y in zip(a, b):
            assert np.abs(x - y).max() <= 1e-14 * np.abs(y).max()


def reference_setup(lib):
    """The grid and disk of test/self_gravity/setup.yml: Rmin 1, Rmax 12.5, logarithmic, 128 x 256, Sigma = 200 g/cm2 / r."""
    d = setups.planet_disk(lib, 128, 256)
    d.rmin, d.rmax = 1.0, 12.5
    radii = lib.radii(d)
    _, rmed = R.geometry(radii, 128)
    sigma = np.broadcast_to((200.0 / setups.SIGMA_CGS / rmed)[:, None], (128, 256)).copy()
    return d, radii, rmed, sigma


ACCEL_CGS = setups._L0 / setups._T0 ** 2   # cm/s^2 per code acceleration


def known_answer_deviation(rmed, g_r):
    """max over r > 2 of |<g_r> / g_direct - 1|: the criterion of the reference's check_results.py (threshold 0.0014)."""
    r_direct, gr_direct = np.loadtxt(GOLDEN, unpack=True)
    assert np.abs(r_direct - rmed).max() <= 1e-13, "the fixture's radii are the grid's Rmed"
    diff = np.abs(g_r.mean(axis=1) * ACCEL_CGS / gr_direct - 1)
    return diff[rmed > 2].max()


def test_reference_known_answer_128x256(product):
    d, radii, rmed, sigma = reference_setup(product)
    g_r, _ = R.sg_fft(sigma, radii, R.SYMMETRIC, 0.05, 0.6)
    dev = known_answer_deviation(rmed, g_r)
    print(f"numpy form against the reference's direct sum, r > 2: {dev:.4e} (threshold 0.0014)")
    assert dev < 0.0014


@pytest.mark.parametrize("mode,name", MODES)
@pytest.mark.parametrize("nr,nphi", SHAPES)
def test_kernel_tables_against_numpy(product, nr, nphi, mode, name):
    d, radii = small_grid(product, nr, nphi)
    p = B.SelfGravityParams(mode, 0, 0.05, 0.6)
    kr, kt = product.selftest_selfgravity_kernel(d, radii, p)
    ref_r, ref_t = R.kernel_tables(radii, nr, nphi, mode, 0.05, 0.6)
    for a, b, what in ((kr, ref_r, "K_radial"), (kt, ref_t, "K_azimuthal")):
        assert a.shape == b.shape == (2 * nr, nphi)
        err = np.abs(a - b) / np.maximum(np.abs(b), np.finfo(float).tiny)
        print(f"{nr}x{nphi} {name} {what}: {err.max():.3e}")
        assert err.max() <= 1e-13
    assert np.abs(kr).max() > 0 and np.abs(kt).max() > 0


def test_kernel_selftest_refusals(product):
    d, radii = small_grid(product, 16, 24)
    bad = [(B.SelfGravityParams(3, 0, 0.05, 0.6), d, "unknown mode"),
           (B.SelfGravityParams(B.SG_BASIC, 0, 0.0, 0.6), d, "aspect_ratio")]
    arith = d.copy()
    arith.radial_spacing = B.SPACING_ARITHMETIC
    bad.append((B.SelfGravityParams(B.SG_BASIC, 0, 0.05, 0.6), arith, "logarithmic"))
    slab = setups.planet_disk(product, 64, 24)
    slab.rank, slab.nranks = 0, 2
    bad.append((B.SelfGravityParams(B.SG_BASIC, 0, 0.05, 0.6), slab, "slabs"))
    odd = setups.planet_disk(product, 16, 28)   # 28 = 4 * 7
    bad.append((B.SelfGravityParams(B.SG_BASIC, 0, 0.05, 0.6), odd, "28"))
    for p, dd, word in bad:
        with pytest.raises(B.FcptError, match=word):
            product.selftest_selfgravity_kernel(dd, product.radii(dd), p)


def five_smooth(n):
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


def test_fft_radices(product):
    for n in range(1, 65):
        if five_smooth(n):
            radices = product.selftest_fft_radices(n)
            assert all(r in (2, 3, 4, 5) for r in radices), (n, radices)
            assert int(np.prod(radices, dtype=np.int64)) == n, (n, radices)
        else:
            with pytest.raises(B.FcptError, match=str(n)):
                product.selftest_fft_radices(n)
    for n in (6144, 8192):
        assert int(np.prod(product.selftest_fft_radices(n), dtype=np.int64)) == n
    for n in (7, 8190, 16384):
        with pytest.raises(B.FcptError, match=str(n)):
            product.selftest_fft_radices(n)
