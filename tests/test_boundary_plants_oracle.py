"""The planted states and the numpy statement of tests/boundary_plants.py do what they are meant to do (no GPU: the
generator, the statement and the oracle only), the way test_cfl_plants_oracle.py holds the CFL plants to their purpose.

  * CASES covers every (variable, condition, side), both frames, damping off and every damping target;
  * the oracle's apply_boundary(0, False) and (dt, True) on the direct-call states equal the statement at its bars;
  * after each of 3 full oracle steps the ghost rings of the oracle's state are `ghost_rings` of its own active rings;
  * the census: every outflow branch is reached in the compared post-step states, every damping zone holds >= 3 rings;
  * the GHOST_BINDS_DT plant moves the oracle's dt of steps 2 to 4 by >= 1e-3;
  * from every state the GPU tests compare, the oracle amplifies cell-wise 1e-15 noise by less than 0.8 GROWTH_CAP
    over the compared steps, so that the GPU tests need no relaxed bar.

Measured on the CPU (oracle against the statement, in units of each bar): every copying condition 0 cells with other
bits; Keplerian v_r, Keplerian v_phi, zero-shear and the reference and zero damping targets 0 bars (the oracle rounds as
numpy does); the mean target 0.016 bars, its ring mean 0.12 bars (a serial sum against math.fsum).  The oracle amplifies
1e-15 noise by 13 .. 1.4e3 over the compared steps (8 steps: at most 8.4e2), against a cap of 8e3.

Two one-line mutations of the oracle were tried against this file in a scratch copy: the sign of the outer outflow
test flipped, and Rmed of the neighbouring ring in the inner Keplerian v_r.  Each fails the direct-call test and the
after-steps test of the case that holds the condition, both EOS (the first by 8 of 8 columns with other bits on the
coarsest grid, the second by 3.6e13 bars).
"""
import numpy as np
import pytest

from fargocpt_amd import binding as B
from tests import boundary_plants as BP
from tests.util import GROWTH_CAP, cell_err, cell_scales

EOS = [False, True]
EOS_IDS = ["iso", "ideal"]
STEP_GRIDS = ((40, 320), (24, 67))      # the grids of the GPU tests' full steps


def test_cases_cover_every_condition_on_both_sides():
    seen = set()
    for c in BP.CASES:
        for var, pair in c.conditions().items():
            assert pair[0] != pair[1], f"{c.name}: {var} has the same condition on both sides"
            seen |= {(var, pair[0], 0), (var, pair[1], 1)}
        assert c.kep_vrad[0] != c.kep_vrad[1] and c.kep_vaz[0] != c.kep_vaz[1] and 1.0 not in c.kep_vrad + c.kep_vaz
        for which, types in c.damp:   # the mean target overwrites column 0 of the `*0` grid a reference condition reads
            for side in (0, 1):
                assert not (types[side] == B.DAMP_MEAN and c.conditions()[which][side] == BP.REF), (c.name, which, side)
        assert dict(c.damp).get("sigma", (0, 0))[1] != B.DAMP_ZERO, f"{c.name}: see the module docstring of boundary_plants"
    missing = {(v, t, s) for v, t in BP.WANTED for s in (0, 1)} - seen
    assert not missing, f"not covered: {sorted(missing)}"
    assert sum(c.omega_frame == 0.0 for c in BP.CASES) >= 2 and sum(c.omega_frame == 1.0 for c in BP.CASES) >= 2
    assert any(not c.damping for c in BP.CASES)
    targets = {t for c in BP.CASES if c.damping for _, ts in c.damp for t in ts}
    assert targets >= {B.DAMP_REFERENCE, B.DAMP_ZERO, B.DAMP_MEAN}
    assert BP.GHOST_BINDS_DT.vrad == (BP.REF, BP.REF)


@pytest.mark.parametrize("ideal", EOS, ids=EOS_IDS)
@pytest.mark.parametrize("case", BP.CASES, ids=[c.name for c in BP.CASES])
def test_direct_calls_equal_the_statement(product, oracle, case, ideal):
    worst = {}
    for nr, nphi in BP.GRIDS:
        bad, w = BP.direct_calls(oracle, product, case, nr, nphi, ideal)
        assert not bad, "\n".join(bad[:8])
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for rank in range(3):
        bad, w = BP.direct_calls(oracle, product, case, 24, 67, ideal, rank, 3)
        assert not bad, "\n".join(bad[:8])
    print(f"[boundary plants] {case.name} {'ideal' if ideal else 'iso'}: largest deviation in bars {worst}")


@pytest.mark.parametrize("ideal", EOS, ids=EOS_IDS)
@pytest.mark.parametrize("case", BP.CASES, ids=[c.name for c in BP.CASES])
def test_ghost_rings_after_steps_and_census(product, oracle, case, ideal):
    for nr, nphi in BP.GRIDS + (BP.SLAB_GRIDS if case.name in BP.SLAB_CASES else ()):
        r = BP.oracle_run(product, oracle, case, nr, nphi, ideal)
        d0, radii, st, st0 = r.planted
        rad = BP.slab_radii(product, d0, radii)
        assert len(r.snaps) == BP.NSTEPS
        for k, snap in enumerate(r.snaps):
            assert all(np.isfinite(v).all() for v in snap.values()), f"{case.name} {nr}x{nphi}, step {k + 1}: not finite"
            bad, _ = BP.ghost_mismatch(d0, rad, snap, st0)
            assert not bad, f"{case.name} {nr}x{nphi}, step {k + 1}: " + "\n".join(bad[:6])
            for branch, n in BP.outflow_census(d0, snap).items():
                need = 16 if nphi >= 67 else 1
                assert n >= need, f"{case.name} {nr}x{nphi}, step {k + 1}: outflow branch {branch} reached by {n} columns"
        if case.damps():
            for which, types in case.damp:
                for side in (0, 1):
                    if types[side] != B.DAMP_NONE:
                        lo, hi = BP.damping_zone(d0, rad, which, side)[:2]
                        assert hi - lo + 1 >= 3, f"{case.name} {nr}x{nphi}: zone of {which}, side {side}: rows {lo} .. {hi}"


def test_ghost_value_binds_dt(product, oracle):
    nr, nphi = BP.BINDS_GRID
    with_plant = BP.oracle_run(product, oracle, BP.GHOST_BINDS_DT, nr, nphi, False, plant=BP.binds_plant, nsteps=4)
    without = BP.oracle_run(product, oracle, BP.GHOST_BINDS_DT, nr, nphi, False, nsteps=4)
    for k in (1, 2, 3):
        rel = abs(with_plant.dts[k] - without.dts[k]) / without.dts[k]
        assert rel >= 1e-3, f"step {k + 1}: dt {with_plant.dts[k]!r} with the plant, {without.dts[k]!r} without ({rel:.2e})"
    d0, radii, st, st0 = with_plant.planted
    for snap in with_plant.snaps:
        assert not BP.ghost_mismatch(d0, BP.slab_radii(product, d0, radii), snap, st0)[0]


def _growth(product, oracle, case, nr, nphi, ideal, leapfrog=False, plant=None, nsteps=BP.NSTEPS):
    base = BP.oracle_run(product, oracle, case, nr, nphi, ideal, leapfrog=leapfrog, plant=plant, nsteps=nsteps)
    d0, radii, st, st0 = base.planted
    noisy = BP.run(oracle, d0, radii, st, st0, nsteps, noise=1.0e-15)
    scales = cell_scales(d0, radii, base.state)
    return max(cell_err(noisy.state[k], base.state[k], scales[k])[0] for k in base.state) / 1.0e-15


@pytest.mark.parametrize("ideal", EOS, ids=EOS_IDS)
def test_growth_stays_under_the_search_bar(product, oracle, ideal):
    cap = 0.8 * GROWTH_CAP
    runs = [(c, nr, nphi, False, None, BP.NSTEPS) for c in BP.CASES for nr, nphi in STEP_GRIDS]
    runs += [(c, nr, nphi, False, None, BP.GRAPH_NSTEPS) for c in BP.CASES for nr, nphi in STEP_GRIDS]
    runs += [(BP.CASE_BY_NAME[n], 40, 320, True, None, BP.NSTEPS) for n in BP.LEAPFROG_CASES]
    runs += [(BP.CASE_BY_NAME[n], nr, nphi, False, None, BP.NSTEPS) for n in BP.SLAB_CASES for nr, nphi in BP.SLAB_GRIDS]
    if not ideal:
        runs += [(BP.GHOST_BINDS_DT, *BP.BINDS_GRID, False, BP.binds_plant, k) for k in (4, BP.GRAPH_NSTEPS)]
    for case, nr, nphi, frog, plant, nsteps in runs:
        g = _growth(product, oracle, case, nr, nphi, ideal, frog, plant, nsteps)
        print(f"[boundary plants] growth {case.name} {nr}x{nphi} {'ideal' if ideal else 'iso'}"
              f"{' leapfrog' if frog else ''}, {nsteps} steps: {g:.2e}")
        assert g < cap, f"{case.name} {nr}x{nphi}, {nsteps} steps: the oracle amplifies 1e-15 noise by {g:.2e} (>= {cap:.1e})"
