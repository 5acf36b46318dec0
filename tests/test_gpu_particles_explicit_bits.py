"""k_particles_step_explicit<ADI, DRAG, CART> computes the bits it computed as the first of four kernels of that text, before
the clock and slab forms became template arguments: the SHA-256 of the ids and of every state and adaptive array of the live
particles after particles_timestep_init and three calls of particles_step, recorded from a build of the parent commit
(tests/golden/make_particles_explicit_parent_bits.py).  The bar is equality.  The clock, slab and slab-clock instances are held
bit-equal to this one by test_gpu_particles_run_steps.py, test_gpu_particles_slabs.py and test_gpu_particles_slab_loop.py."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X
import tests.test_gpu_particles_explicit_parity as parity

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "particles_explicit_parent_bits.json")
CASES = list(itertools.product([False, True], repeat=3))      # ADI x DRAG x CART: the eight host-argument instances
N = 257                                                       # a full workgroup and one lane of a second
CALLS = 3
STATE = ("r", "phi", "r_dot", "phi_dot", "radius", "stokes")
ADAPTIVE = ("timestep", "facold", "r_ddot", "phi_ddot", "accepted", "rejected")


def case_key(adiabatic, drag, cartesian):
    return "adiabatic=%d drag=%d cartesian=%d" % (adiabatic, drag, cartesian)


def hashes(product, case):
    """The 48 x 256 parity grid after 8 gas steps, the draw of 257 in the form asked for -> {array: SHA-256}"""
    adiabatic, drag, cartesian = case
    b = parity.Bench(product, adiabatic)
    s = xc.explicit_draw(b.d, b.radii, n=N)
    s["stokes"] = R.initial_stokes(b.g, b.gas, b.phys, s)
    s = X.add_adaptive(xc.to_cartesian(s) if cartesian else s)
    before = {k: s[k].copy() for k in ("r", "phi")}
    b.upload(s, drag, cartesian)
    for _ in range(CALLS):
        b.ctx.particles_step(xc.EXPLICIT_DT, cases.PARITY_INDIRECT, b.d.omega_frame * xc.EXPLICIT_DT)
    got, ad = b.ctx.particles_get(), b.ctx.particles_adaptive_get()
    b.ctx.close()
    assert got["id"].size > 0
    live = np.isin(s["id"], got["id"])
    assert (got["r"] != before["r"][live]).any() or (got["phi"] != before["phi"][live]).any(), "nobody moved"
    out = {"id": got["id"]}
    out.update({k: got[k] for k in STATE})
    out.update({k: ad[k] for k in ADAPTIVE})
    return {k: hashlib.sha256(np.ascontiguousarray(out[k]).tobytes()).hexdigest() for k in sorted(out)}


@pytest.mark.parametrize("case", CASES, ids=[case_key(*c) for c in CASES])
def test_explicit_kernel_gives_the_parent_bits(product, case):
    want = json.load(open(GOLDEN))["cases"][case_key(*case)]
    assert hashes(product, case) == want
