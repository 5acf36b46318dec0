"""The planted maxima of tests/cfl_plants.py do what they are meant to do (no GPU: the generator, the numpy
restatement of condition_cfl and the oracle only), the way test_rough_states_census.py holds the rough states to
their purpose.  A plant that quietly stops binding would let the GPU tests pass while testing nothing.

For every case (grid shape, EOS, descriptor variant, slab) and every plant:
  * the oracle's dt equals the numpy restatement's to 1e-13 relative (two float64 evaluations of cfl.cpp:185-376;
    measured: bit for bit on every plant);
  * a plant meant to bind brings the oracle's dt to at most half the base dt, the restatement's argmin is the cell
    (or ring pair) the plant names, and the largest inverse limit there is the term it names;
  * a dead plant leaves the oracle's dt bit for bit;
  * a `mean` plant (a v_phi spike in ring 0 or ring active_size, whose cells do not count but whose mean enters a
    counted shear limit) is only compared, oracle against numpy.
No plant is skipped: every plant `make_plants` returns is checked, and the census below is what it returns.

Plants per case (the test prints the census by kind), 24 rings unless a slab: total (of them dead / mean),
isothermal | ideal EOS:
  Nphi 17: 136 (12/16) | 202 (28/16)      96: 452 (12/16) | 676 (28/16)       128: 580 (12/16) | 868 (28/16)
  263: 1180 (20/32) | 1770 (52/32)        320, on either path, leapfrog, SN, None, constant nu: 1408 (20/32) | 2112 (52/32)
  320 with StabilizeViscosity 2: 2112 (52/32) | 2816 (84/32), 672 of them cfac
  320 without FastTransport: 1404 | 2108 (no shear plants: a ring offset is a plant of term 3 there)
  514: 2184 (20/32) | 3276 (52/32)        2048: 272 (20/32) | 380 (52/32)     2050: 276 (20/32)
  4096, each of its forms: 400 (20/32) | 540 (52/32)                          4098: 404 (20/32) | 545 (52/32)
  6144: 528 (20/32) | 700 (52/32)         8192: 656 (20/32) | 860 (52/32)     8194: 660 (20/32) | 865 (52/32)
  slabs of 3 x 40 rings x 320, with the rings at the split launch's boundaries: rank 0 1566 (50/32) | 2334 (82/32),
  rank 1 1563 (95/16) | 2315 (127/16), rank 2 1533 (65/16) | 2285 (97/16)
Rings of up to 514 cells carry every kind at every column of the middle ring; longer rings carry v_r+ and v_phi- (and
e or Q+ at every other one) at the block-boundary columns of the middle ring, and every kind at the wrap (columns 0, 1,
Nphi-2, Nphi-1) and at cells 126-129 of all planted rings.

The asymmetry of v_r plants in ring 1 (test_negative_vr_in_the_first_active_ring): at 24 x 320 the base dt is the
shear limit of ring pair (0, 1), 2.66 times tighter than the tightest cell.  +4 c_s at face (1, j) compresses cell 1
(4 C^2 times the jump: dt falls to 0.36 of base); -4 c_s expands it, leaves term 2 alone in quadrature with the
sound term (a cell limit 1.9 times the base dt, which does not bind), and compresses cell 0, which is not active.
Nothing is wrong in ring 1; a plant sized from the local sound speed was too weak, hence PLANT_TIGHTEN times the
base dt as the size rule.
"""
import numpy as np
import pytest

from fargocpt_amd import binding as B
from tests import cfl_plants as CP

TOL_NUMPY = 1e-13


@pytest.mark.parametrize("case", CP.ALL_CASES, ids=[c.name for c in CP.ALL_CASES])
def test_plants_bind_where_meant(product, oracle, case):
    split = case.nranks > 1
    d0, _, g, base, res, plants = CP.setup_case(product, case, split)
    dt0, dts = CP.oracle_dts(product, oracle, case, split)
    assert abs(dt0 - res.dt) <= TOL_NUMPY * dt0, f"{case.name}: base dt {dt0!r} (oracle) vs {res.dt!r} (numpy)"
    if case.const_nu:
        assert res.binding()[3] == "visc", f"{case.name}: the constant viscosity does not bind: {res.binding()}"
    kinds = {}
    work = {k: v.copy() for k, v in base.items()}
    for p, dt in zip(plants, dts):
        kinds[p.kind] = kinds.get(p.kind, 0) + 1
        p.apply(work)
        r = CP.condition_cfl(d0, g, work, res, p.rings)
        p.restore(work, base)
        assert abs(dt - r.dt) <= TOL_NUMPY * dt, f"{case.name} {p.name}: dt {dt!r} (oracle) vs {r.dt!r} (numpy)"
        if p.kind == "dead":
            assert dt == dt0, f"{case.name} {p.name}: a dead plant moved dt from {dt0!r} to {dt!r}"
        elif p.kind != "mean":
            assert dt <= 0.5 * dt0, f"{case.name} {p.name}: dt only {dt / dt0:.4f} of base"
            b = r.binding()
            assert b[:3] == p.bind and b[3] == p.term, f"{case.name} {p.name}: meant {p.bind} {p.term}, binds {b}"
    for f in work:
        assert np.array_equal(work[f], base[f])
    # every kind the case calls for is there, at live and at dead places
    want = {"vr+", "vr-", "vphi+", "vphi-", "dead"} | ({"e", "q"} if case.ideal else set()) | \
        ({"shear"} if d0.fast_transport else set()) | ({"cfac"} if d0.stabilize_viscosity == 2 else set())
    assert want <= set(kinds), f"{case.name}: kinds {sorted(kinds)}"
    print(f"[cfl plants] {case.name}: {len(plants)} plants {kinds}, none left out; base dt {dt0:.6e} from {res.binding()}")


def test_restatement_is_whole_without_a_base(product):
    """The ring-wise update used for the plants gives what a full evaluation of the planted state gives."""
    case = CP.Case("check", 96, True)
    d0, _, g, base, res, plants = CP.setup_case(product, case)
    work = {k: v.copy() for k, v in base.items()}
    for p in plants[::7]:
        p.apply(work)
        a, b = CP.condition_cfl(d0, g, work, res, p.rings), CP.condition_cfl(d0, g, work)
        p.restore(work, base)
        assert a.dt == b.dt and np.array_equal(a.dt_cell, b.dt_cell) and np.array_equal(a.shear, b.shear), p.name


def test_oracle_needs_its_derived_grids_refreshed(product, oracle):
    """An upload of e alone leaves the oracle's sound-speed and viscosity grids those of the state before: its dt
    does not move until recalculate_derived -- which is why Session.load calls it."""
    case = CP.Case("fresh", 96, True)
    d0, radii, _, base, _, plants = CP.setup_case(product, case)
    p = next(p for p in plants if p.kind == "e")
    s = CP.Session(oracle, d0, radii, base)
    dt0 = s.cfl()
    work = {k: v.copy() for k, v in base.items()}
    p.apply(work)
    s.ctx.upload(B.F_ENERGY, work["energy"])
    stale = s.ctx.cfl()
    s.ctx.recalculate_derived()
    fresh = s.ctx.cfl()
    s.close()
    assert stale > 0.9 * dt0 and fresh <= 0.5 * dt0, (dt0, stale, fresh)


def test_negative_vr_in_the_first_active_ring(product):
    """See the module docstring: -4 c_s in ring 1 does not bind at 24 x 320, and nothing is wrong there."""
    case = CP.Case("asym", 320)
    d0, _, g, base, res, plants = CP.setup_case(product, case)
    assert res.binding() == ("shear", 0, 1, "shear")
    out = {}
    for s in (4.0, -4.0):
        st = {k: v.copy() for k, v in base.items()}
        st["vrad"][1, 5] = s * g.cs_iso[1]
        out[s] = CP.condition_cfl(d0, g, st)
    assert out[4.0].binding() == ("cell", 1, 5, "artvisc") and abs(out[4.0].dt / res.dt - 0.36) < 0.01
    assert out[-4.0].dt == res.dt and out[-4.0].invdt[3, 1, 5] == 0.0          # expanding: no artificial viscosity
    assert 1.5 * res.dt < out[-4.0].dt_cell[1, 5] < res.dt_cell[1, 5]           # tighter than before, not binding
    # the plant sized from the base dt binds there, through the advection term alone
    p = next(p for p in plants if p.name == f"vr-@face{g.first_active}c0")
    assert p.bind == ("cell", g.first_active, 0) and p.term == "vr"
