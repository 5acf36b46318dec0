"""k_transport_fused in the damping zones: the reference values of a ring, requested in one batch.

A ring in which any quantity is damped loads the reference values of all its quantities at once and selects by the
quantity's wave-uniform type: towards the reference (type 1), towards zero / the density floor (type 2), or not at
all (type 0: the loaded value is dropped).  A value that is dropped where it is needed, swapped with a neighbour's,
or selected by another quantity's type is a gross error -- the reference state is the initial disk, v_phi ~ 1,
v_r ~ 0, Sigma ~ 1e-4 -- so every combination of the three types over (v_r, v_phi, Sigma) must give the oracle's
state, cell by cell, and the bits of the same run with other chunks.

The grid is the 40 x 320 planet disk (Nphi >= 256: the fused kernel runs) with damping limits 1.30 / 0.78: zones of
about six rings at either end.  The chunks are set explicitly, one to three rings each, so that the inner zone holds
a whole chunk and ends inside another (checked against the chunk table and the rings the oracle's damping moves).
The outer side runs another combination than the inner side (the inner one reversed), so that one run has rings of
two different type sets.  Row Nr of v_r, which the kernel copies and damps by itself, is part of the comparison."""
import itertools

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups
from tests.util import cell_err, cell_scales, perturb

pytestmark = pytest.mark.gpu

NR, NPHI, NSTEPS = 40, 320, 3
TOL = 1e-10
TYPES = {"none": B.DAMP_NONE, "reference": B.DAMP_REFERENCE, "zero": B.DAMP_ZERO}
# (dealt from both ends alternately: inner, outer, inner, ...; the last entry repeats)
CHUNK_PATTERNS = ([2, 3, 3, 1, 3, 3, 1, 2, 1, 2, 2, 3], [2, 3, 3, 2, 2, 3, 2, 2, 2, 1, 1, 2],
                  [1, 3, 1, 2, 1, 2, 2, 2, 3, 2, 1, 1])

ISO_COMBOS = list(itertools.product(TYPES, repeat=3))          # (v_r, v_phi, Sigma): all 27
# ideal EOS, (v_r, v_phi, Sigma, e): every type of e with every type of one other quantity at least once, the ring
# whose only damped quantity is e, and the all-of-a-kind rings
ADI_COMBOS = [("none", "none", "none", "reference"), ("none", "none", "none", "zero"),
              ("reference", "reference", "reference", "reference"), ("zero", "zero", "zero", "zero"),
              ("reference", "none", "zero", "none"), ("zero", "reference", "none", "reference"),
              ("none", "zero", "reference", "zero"), ("reference", "zero", "zero", "reference"),
              ("zero", "none", "reference", "none"), ("none", "reference", "zero", "zero"),
              ("reference", "reference", "none", "zero"), ("zero", "zero", "reference", "none")]


def _desc(product, adi, combo):
    d = setups.planet_disk(product, NR, NPHI, adiabatic=adi)
    d.damping_inner_limit, d.damping_outer_limit = 1.30, 0.78
    arrs = (d.damp_vrad, d.damp_vaz, d.damp_sigma, d.damp_energy)
    inner = tuple(combo) + (("none",) if len(combo) == 3 else ())
    outer = tuple(reversed(combo[:3])) + inner[3:]
    for arr, ti, to in zip(arrs, inner, outer):
        arr[0], arr[1] = TYPES[ti], TYPES[to]
    return d


_SHARED = {}


def _shared(product, oracle, adi):
    """(radii, perturbed initial fields, rings of the inner zone, first ring of the outer zone) -- the zones as the
    oracle's damping draws them: the rings one step with every quantity damped towards zero moves against the same
    step without damping."""
    if adi not in _SHARED:
        d = _desc(product, adi, ("zero",) * (4 if adi else 3))
        radii = product.radii(d)
        fields = perturb(product.initial_fields(d.copy(), radii), d, 1e-3)
        out = []
        for damping in (1, 0):
            dd = d.copy()
            dd.damping = damping
            ctx = driver.make_context(oracle, dd, fields=fields, radii=radii, bodies=setups.jupiter_bodies(dd))
            S = driver.SlabSet([ctx])
            S.prepare()
            S.run(1)
            out.append(ctx.state()["sigma"])
            ctx.close()
        moved = np.flatnonzero((out[0] != out[1]).any(axis=1))
        n_in = int(np.flatnonzero(np.diff(moved) > 1)[0]) + 1
        assert (moved[:n_in] == np.arange(n_in)).all() and moved[-1] == NR - 1, moved
        first_out = int(moved[n_in])
        assert (moved[n_in:] == np.arange(first_out, NR)).all(), moved
        assert 4 <= n_in <= 9 and 4 <= NR - first_out <= 9, moved   # (about six rings each)
        _SHARED[adi] = (radii, fields, n_in, first_out)
    return _SHARED[adi]


def _ragged(ctx, n_in, first_out):
    """Sets the first pattern with a chunk wholly inside the inner zone and one that the zone's edge cuts; chunks of
    one to three rings (plus the crumbs of the chunk dealt last)."""
    for lengths in CHUNK_PATTERNS:
        ctx.set_transport_chunks(lengths)
        tab = ctx.transport_chunks()
        live = tab[tab[:, 2] > tab[:, 1]]
        cover = np.zeros(NR, dtype=np.int64)
        for a, b in {(int(a), int(b)) for _, a, b in live[:, :3]}:
            cover[a:b] += 1
        assert (cover == 1).all(), (lengths, cover)
        spans = sorted({(int(a), int(b)) for _, a, b in live[:, :3]})
        n = np.array([b - a for a, b in spans])
        whole = any(b <= n_in for a, b in spans)
        cut = any(a < n_in < b for a, b in spans)
        cut_out = any(a < first_out < b for a, b in spans)
        if whole and cut and cut_out and n.min() == 1 and (n > 3).sum() <= 1 and n.max() <= 5:
            return spans
    raise AssertionError(f"no chunk pattern holds a chunk inside rings [0, {n_in}) and cuts its edge and ring {first_out}")


def _run(lib, d, radii, fields, chunks=None, n_in=None, first_out=None):
    ctx = driver.make_context(lib, d, fields=fields, radii=radii, bodies=setups.jupiter_bodies(d))
    try:
        if chunks == "ragged":
            _ragged(ctx, n_in, first_out)
        elif chunks == "equal":
            ctx.set_option("transport_graded", 0)
            assert len(ctx.transport_chunks()) == 0
        S = driver.SlabSet([ctx])
        S.prepare()
        if chunks is None:
            S.run(NSTEPS)
        else:
            assert ctx.run_steps(NSTEPS) == NSTEPS
        c = ctx.clock
        return ctx.state(), (c.time, c.last_dt, c.n_hydro_iter)
    finally:
        ctx.close()


def _check(product, oracle, adi, combo):
    radii, fields, n_in, first_out = _shared(product, oracle, adi)
    d = _desc(product, adi, combo)
    ref, _ = _run(oracle, d, radii, fields)
    ragged, clk_r = _run(product, d, radii, fields, "ragged", n_in, first_out)
    equal, clk_e = _run(product, d, radii, fields, "equal")
    names = ["sigma", "vrad", "vazi"] + (["energy"] if adi else [])
    assert ref["vrad"].shape == (NR + 1, NPHI)   # (row Nr of v_r is compared with the rest)
    scales = cell_scales(d, radii, ref)
    for k in names:
        err, pos = cell_err(ragged[k], ref[k], scales[k])
        print(f"{'ideal' if adi else 'iso'} {combo} {k}: {err:.3e} at {pos}")
        assert err <= TOL, (k, err, pos)
    assert clk_r == clk_e
    for k in ragged:
        assert np.array_equal(ragged[k], equal[k]), k


@pytest.mark.parametrize("combo", ISO_COMBOS, ids=["-".join(c) for c in ISO_COMBOS])
def test_isothermal_type_combinations(product, oracle, combo):
    _check(product, oracle, False, combo)


@pytest.mark.parametrize("combo", ADI_COMBOS, ids=["-".join(c) for c in ADI_COMBOS])
def test_ideal_eos_type_combinations(product, oracle, combo):
    _check(product, oracle, True, combo)
