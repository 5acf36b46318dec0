"""The generator of the dust-diffusion kick without a GPU: kernels/philox.h as fcpt_host.cpp exports it, against the
published known answers and against the numpy restatement (tests/particles_diffusion_ref.py)."""
import numpy as np
import pytest

import tests.particles_diffusion_ref as D

# Random123's known answers for philox4x32_10 (counter, key, output), recomputed with a plain-Python statement of the
# published algorithm
KNOWN_ANSWERS = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KNOWN_ANSWERS)
def test_philox_known_answers(product, counter, key, want):
    assert tuple(int(v) for v in product.philox4x32(counter, key)) == want
    assert tuple(int(v) for v in D.philox4x32(counter, key)) == want


def test_the_uniforms_are_exact_and_inside_the_unit_interval():
    u1, u2 = D.uniforms(3, np.arange(1 << 16, dtype=np.uint64), 5)
    for u in (u1, u2):
        assert (u > 0.0).all() and (u < 1.0).all()
        assert np.array_equal(u * 2.0 ** 53 % 2.0, np.ones(u.size))      # an odd multiple of 2^-53: nothing was rounded


def test_std_normal_matches_the_restatement(product):
    rng = np.random.default_rng(20240919)
    n = 4096
    seed = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    ids = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    step = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    ids[:64], step[:64] = np.arange(64), np.arange(64)[::-1]                 # small values too
    ids[64:128] = (np.uint64(1) << np.uint64(32)) + np.arange(64, dtype=np.uint64)   # just above 2^32
    step[128:192] = (np.uint64(1) << np.uint64(32)) + np.arange(64, dtype=np.uint64)
    assert (ids > 2 ** 32).sum() > n // 2 and (step > 2 ** 32).sum() > n // 2
    want = D.std_normal(seed, ids, step)
    got = np.array([product.particles_std_normal(s, i, t) for s, i, t in zip(seed.tolist(), ids.tolist(), step.tolist())])
    u1, _ = D.uniforms(seed, ids, step)
    diff = np.abs(got - want)
    for name, k in (("smallest u1", int(np.argmin(u1))), ("largest u1", int(np.argmax(u1)))):
        print("%s = %.3e: host %.17g, restatement %.17g" % (name, u1[k], got[k], want[k]))
        assert diff[k] <= 1e-13
    print("largest difference %.3e, largest |snv| %.3f" % (diff.max(), np.abs(got).max()))
    assert diff.max() <= 1e-13
    assert np.abs(got).max() <= np.sqrt(2.0 * 53.0 * np.log(2.0))


def _moments(x):
    n = x.size
    mean, var = x.mean(), x.var()
    lag1 = np.mean((x[1:] - mean) * (x[:-1] - mean)) / var
    return n, mean, var, lag1


@pytest.mark.parametrize("along", ["ids", "steps"])
def test_moments_of_the_deviates(along):
    """Mean, variance and lag-1 correlation of 2^20 deviates, each within 5 sigma of its sampling error."""
    k = np.arange(1 << 20, dtype=np.uint64)
    base = (np.uint64(1) << np.uint64(32)) - np.uint64(1 << 19)      # the run crosses 2^32
    x = D.std_normal(20110711, base + k, 12345) if along == "ids" else D.std_normal(20110711, 4242424242, base + k)
    n, mean, var, lag1 = _moments(x)
    print("%s: mean %.3e (bar %.3e), var - 1 %.3e (bar %.3e), lag-1 %.3e (bar %.3e)"
          % (along, mean, 5 / np.sqrt(n), var - 1.0, 5 * np.sqrt(2.0 / n), lag1, 5 / np.sqrt(n)))
    assert abs(mean) <= 5.0 / np.sqrt(n)
    assert abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert abs(lag1) <= 5.0 / np.sqrt(n)
