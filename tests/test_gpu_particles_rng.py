"""The deviates of the device (fcpt_particles_normals: one launch of the kick's own device function over the live slots)
against the numpy restatement, and their independence of the slot order."""
import numpy as np
import pytest

from fargocpt_amd import driver

import tests.particles_cases as cases
import tests.particles_diffusion_cases as dcases
import tests.particles_diffusion_ref as D
import tests.particles_ref as R

pytestmark = pytest.mark.gpu

STEPS = (0, (1 << 32) - 1, (1 << 63) + 12345)


@pytest.fixture(scope="module")
def ctx_and_draw(product):
    d = cases.parity_desc(product, 48, 256)
    radii = product.radii(d)
    ctx = driver.make_context(product, d, radii=radii)
    prm = cases.parity_params(product, d, cartesian=False)
    yield ctx, prm, d, radii
    ctx.close()


@pytest.mark.parametrize("n", [1000, 257])
def test_device_deviates_match_the_restatement(ctx_and_draw, n):
    ctx, prm, d, radii = ctx_and_draw
    s = dcases.diffusion_draw(d, radii, n=n)
    ctx.particles_diffusion(seed=dcases.PARITY_SEED)
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    for step in STEPS:
        got = ctx.particles_normals(step)
        want = D.std_normal(dcases.PARITY_SEED, s["id"], step)
        assert got.shape == want.shape
        print("n = %d, step %d: largest difference %.3e" % (n, step, np.abs(got - want).max()))
        assert np.abs(got - want).max() <= 1e-13
    assert ctx.particles_diffusion_get().step == 0        # nothing was stepped


def test_permuting_the_upload_permutes_the_deviates(ctx_and_draw):
    ctx, prm, d, radii = ctx_and_draw
    s = dcases.diffusion_draw(d, radii, n=1000)
    ctx.particles_diffusion(seed=dcases.PARITY_SEED)
    ctx.particles_set(prm, s["id"], *(s[k] for k in R.FIELDS))
    a = ctx.particles_normals(77)
    perm = np.random.default_rng(3).permutation(1000)
    ctx.particles_set(prm, s["id"][perm], *(s[k][perm] for k in R.FIELDS))
    b = ctx.particles_normals(77)
    assert np.array_equal(b, a[perm])
    assert not np.array_equal(ctx.particles_normals(78), b)
