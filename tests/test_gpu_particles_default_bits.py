"""k_particles_step<ADI, true, false> computes the bits it computed before drag and diffusion became template
arguments: the SHA-256 of every final array of the four parity cases, recorded from a build of the parent commit
(tests/golden/make_particles_parent_bits.py), with and without a particles_diffusion call that sets the defaults."""
import hashlib
import json
import os

import numpy as np
import pytest

from fargocpt_amd import binding as B

import tests.particles_cases as cases
import tests.test_gpu_particles_parity as parity

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "particles_parent_bits.json")
CASES = [(False, False, 0.6, 1.0, 1000), (True, True, 0.6, 1.0, 1000), (False, True, 0.0, 0.0, 257), (True, False, 0.0, 0.0, 1)]


def case_key(adiabatic, cartesian, smoothing, omega_frame, n):
    return "adiabatic=%d cartesian=%d smoothing=%g omega_frame=%g n=%d" % (adiabatic, cartesian, smoothing, omega_frame, n)


def hashes(product, case):
    adiabatic, cartesian, smoothing, omega_frame, n = case
    d = cases.parity_desc(product, 48, 256, adiabatic=adiabatic, smoothing=smoothing, omega_frame=omega_frame)
    out, _, _ = parity._run(product, d, n, cartesian, compare=False)
    return {k: hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).hexdigest() for k in sorted(out)}


class _DefaultsSetExplicitly:
    """The library, with contexts that call particles_diffusion(defaults) before their first particles_set."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def create(self, d, radii):
        ctx = self._lib.create(d, radii)
        ctx.particles_diffusion(gas_drag=True, diffusion=False, seed=0, step=0)
        return ctx


@pytest.mark.parametrize("explicit_defaults", [False, True])
@pytest.mark.parametrize("case", CASES, ids=[case_key(*c) for c in CASES])
def test_default_kernel_gives_the_parent_bits(product, case, explicit_defaults):
    want = json.load(open(GOLDEN))["cases"][case_key(*case)]
    got = hashes(_DefaultsSetExplicitly(product) if explicit_defaults else product, case)
    assert got == want
