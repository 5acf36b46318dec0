"""The CFL reduction against planted maxima (tests/cfl_plants.py): every kernel form that `kernels/launch.h` picks
by grid shape, every term, every place where a reduction goes wrong -- a skipped thread slot or cell pair, the wrong
azimuthal neighbour at a pair boundary, a wavefront boundary or the ring wrap, an active ring range off by one, a
ring covered twice or not at all by the split launch, a partial maximum kept from an earlier call.

One context per library and shape, one upload and one cfl() per plant, the base state again after every few plants.
Every dt is held against the oracle's at TOL_DT = 1e-12 (the bar of tests/test_gpu_rough_states.py for one CFL
reduction); the base dt must come back bit for bit; the profiler's launch counts say that the intended kernels ran.
tests/test_cfl_plants_oracle.py shows (without a GPU) that every plant binds where it is meant to, so a kernel
that misses the planted cell, or the term it binds through, returns a dt at least twice too large.  A failure
names the plants: kind, ring (or face, or ring pair) and column."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver
from tests import cfl_plants as CP

pytestmark = pytest.mark.gpu
TOL_DT = 1e-12
BASE_EVERY = 16   # plants between two returns to the base state

_PRODUCT_DTS = {}


def _assert_path(case, prof):
    ran = lambda n: prof.get(n, (0, 0))[1]
    if case.path == "rings":
        assert ran("k_cfl_rings") > 0 and ran("k_cfl_cells") == 0, f"{case.name}: expected k_cfl_rings: {sorted(prof)}"
    else:
        assert ran("k_cfl_rings") == 0 and ran("k_cfl_cells") > 0 and ran("k_ring_mean") > 0, \
            f"{case.name}: expected k_ring_mean + k_cfl_cells: {sorted(prof)}"


def _report(case, bad, n):
    assert not bad, (f"{case.name}: {len(bad)} of {n} calls off by more than {TOL_DT} (dt HIP, dt oracle, relative): "
                     + "; ".join(f"{name}: {a!r} vs {b!r} ({abs(a - b) / b:.2e})" for name, a, b in bad[:8]))


def product_dts(product, oracle, case, split=False):
    """The product's dt for the base state and every plant of the case, each checked against the oracle's; the base
    state returns after every BASE_EVERY plants and must give its first dt again.  Once per process and case."""
    key = (case, split)
    if key in _PRODUCT_DTS:
        return _PRODUCT_DTS[key]
    d0, radii, _, base, _, plants = CP.setup_case(product, case, split)
    dt0_o, dts_o = CP.oracle_dts(product, oracle, case, split)
    s = CP.Session(product, d0, radii, base, case.options)
    try:
        names = product.kernel_names()
        s.ctx.profile_start([names.index(k) for k in ("k_cfl_rings", "k_cfl_cells", "k_ring_mean")], max_launches=64)
        dt0 = s.cfl()
        first = [s.cfl(p) for p in plants[:4]]
        _assert_path(case, s.ctx.profile_stop())
        bad = [("base", dt0, dt0_o)] if abs(dt0 - dt0_o) > TOL_DT * dt0_o else []
        dts, stale = [], []
        for k, p in enumerate(plants):
            dt = first[k] if k < len(first) else s.cfl(p)
            dts.append(dt)
            if abs(dt - dts_o[k]) > TOL_DT * dts_o[k]:
                bad.append((p.name, dt, dts_o[k]))
            if k % BASE_EVERY == BASE_EVERY - 1 or k == len(plants) - 1:
                again = s.cfl()
                if again != dt0:
                    stale.append((p.name, again))
        assert not stale, f"{case.name}: the base dt {dt0!r} did not come back after {stale[:4]} ({len(stale)} times)"
        _report(case, bad, len(plants) + 1)
    finally:
        s.close()
    _PRODUCT_DTS[key] = (dt0, dts)
    return _PRODUCT_DTS[key]


@pytest.mark.parametrize("case", CP.SHAPE_CASES + CP.VARIANT_CASES,
                         ids=[c.name for c in CP.SHAPE_CASES + CP.VARIANT_CASES])
def test_planted_maxima(product, oracle, case):
    product_dts(product, oracle, case)


@pytest.mark.parametrize("nphi", [320, 4096])
@pytest.mark.parametrize("ideal", [False, True], ids=["iso", "ideal"])
def test_both_paths_give_the_same_dt(product, oracle, nphi, ideal):
    """k_cfl_rings and k_ring_mean + k_cfl_cells (option cfl_rings = 0) on the same plants: each within TOL_DT of the
    oracle, and of each other."""
    tag = "ideal" if ideal else "iso"
    by_name = {c.name: c for c in CP.SHAPE_CASES}
    rings = by_name[f"rings320-{tag}" if nphi == 320 else ("rings512x4_4096-ideal" if ideal else "rings512x4_4096-iso")]
    cells = by_name[f"cells_for_rings{nphi}-{tag}"]
    plants = CP.setup_case(product, rings)[5]
    assert [p.name for p in plants] == [p.name for p in CP.setup_case(product, cells)[5]]
    (a0, a), (b0, b) = product_dts(product, oracle, rings), product_dts(product, oracle, cells)
    bad = [(p.name, x, y) for p, x, y in zip(plants, a, b) if abs(x - y) > TOL_DT * y]
    bad += [("base", a0, b0)] if abs(a0 - b0) > TOL_DT * b0 else []
    _report(rings, bad, len(plants) + 1)


@pytest.mark.parametrize("name", ["rings320-ideal", "rings512x4_2050-iso", "cells263-iso"])
def test_device_value(product, oracle, name):
    """cfl_device(ptr) leaves at ptr the bits that cfl() returns."""
    import torch
    case = next(c for c in CP.SHAPE_CASES if c.name == name)
    d0, radii, _, base, _, plants = CP.setup_case(product, case)
    dt0_o, dts_o = CP.oracle_dts(product, oracle, case)
    out = torch.zeros(1, dtype=torch.float64, device="cuda")
    s = CP.Session(product, d0, radii, base, case.options)
    try:
        bad = []
        for k in [None] + list(range(0, len(plants), 11)) + [None]:
            p, want = (None, dt0_o) if k is None else (plants[k], dts_o[k])
            s.load(p)
            out.fill_(-1.0)
            torch.cuda.synchronize()
            s.ctx.cfl_device(out.data_ptr())
            s.ctx.synchronize()
            v = float(out.cpu()[0])
            dt = s.ctx.cfl()
            assert v == dt, f"{name} {p.name if p else 'base'}: cfl_device left {v!r}, cfl() returns {dt!r}"
            if abs(v - want) > TOL_DT * want:
                bad.append((p.name if p else "base", v, want))
        _report(case, bad, len(plants) // 11 + 3)
    finally:
        s.close()


def _near_split_boundary(g, p):
    lo, hi = CP.CFL_EDGE_LO, g.nr - CP.CFL_EDGE_HI
    return p.ring in (lo - 1, lo, hi - 1, hi, hi + 1) and p.col in (-1, 0, 1, 127, 128, g.nphi - 1)


@pytest.mark.parametrize("case", CP.SLAB_CASES, ids=[c.name for c in CP.SLAB_CASES])
def test_slabs_unsplit_and_split(product, oracle, case, monkeypatch):
    """3 x 40 rings x 320, each slab against the oracle's slab of the same rank.  First every plant through cfl().
    Then the reduction split around the ghost exchange: fcpt_cfl_begin evaluates the interior rings only once a step
    is queued, so each plant near a launch boundary (rings CFL_EDGE_LO - 1, CFL_EDGE_LO, nr - CFL_EDGE_HI - 1,
    nr - CFL_EDGE_HI) is uploaded, stepped by 1e-6 of its CFL step (the plant stays what binds; the ghost rings keep
    their values: no neighbour writes them here), and cfl_begin -> post -> cfl gives the bits of the same sequence without the split (FCPT_CFL_SPLIT=0)
    and the oracle's value for the same sequence; the ring kernel launches twice per split reduction."""
    product_dts(product, oracle, case, split=True)
    d0, radii, g, base, _, plants = CP.setup_case(product, case, split=True)
    chosen = [p for p in plants if p.kind not in ("dead", "mean", "q") and _near_split_boundary(g, p)]   # (the step writes Q+ anew)
    assert len(chosen) >= 16 and {p.ring for p in chosen} >= {CP.CFL_EDGE_LO - 1, CP.CFL_EDGE_LO,
                                                             g.nr - CP.CFL_EDGE_HI - 1, g.nr - CP.CFL_EDGE_HI}
    names = product.kernel_names()

    def sequence(lib, split_env):
        monkeypatch.setenv("FCPT_CFL_SPLIT", split_env)
        s = CP.Session(lib, d0, radii, base, case.options if lib is product else ())
        dts, launches = [], 0
        try:
            for p in chosen:
                s.load(p)
                dt = s.ctx.calculate_timestep(s.ctx.cfl())
                tiny = 1.0e-6 * dt
                s.ctx.step(tiny)
                if lib is product:
                    s.ctx.profile_start([names.index("k_cfl_rings")], max_launches=8)
                    s.ctx.cfl_begin()
                s.ctx.post(tiny)
                dts.append(s.ctx.cfl())
                if lib is product:
                    launches += s.ctx.profile_stop()["k_cfl_rings"][1]
                s.dirty = set(base)   # the step moved every grid: the whole base state before the next plant
        finally:
            s.close()
        return dts, launches

    ref, _ = sequence(oracle, "1")
    split, n_split = sequence(product, "1")
    whole, n_whole = sequence(product, "0")
    assert n_split == 2 * len(chosen) and n_whole == len(chosen), (n_split, n_whole, len(chosen))
    diff = [(p.name, a, b) for p, a, b in zip(chosen, split, whole) if a != b]
    assert not diff, f"{case.name}: split and unsplit reductions differ: {diff[:6]}"
    _report(case, [(p.name, a, b) for p, a, b in zip(chosen, split, ref) if abs(a - b) > TOL_DT * b], len(chosen))


MERGED_CFL = 0.02
MERGED_TIGHTEN = 2.0


def _grids(ctx, d0):
    st = {k: ctx.download(CP.FIELD_IDS[k]) for k in ("sigma", "vrad", "vazi", "energy")}
    if d0.eos == B.EOS_IDEAL:
        st["qplus"], st["qminus"] = ctx.download(B.F_QPLUS), ctx.download(B.F_QMINUS)
    return st


@pytest.mark.parametrize("nr,nphi", [(32, 320), (24, 2050)])
@pytest.mark.parametrize("ideal", [False, True], ids=["iso", "ideal"])
@pytest.mark.parametrize("where", ["ring1", "ring_nr-2"])
def test_merged_and_folded_forms(product, oracle, nr, nphi, ideal, where):
    """fcpt_run_steps with the boundary call inside the ring launch (k_cfl_rings_bc, option bc_in_cfl = 2) and with the
    fold inside the marching source kernel forced on and off: clock and state of the host loop
    cfl -> calculate_timestep -> step -> post, bit for bit; the host loop's dt history is the oracle's to TOL_DT.

    One state per plant, in ring 1 or in ring nr-2: the rings whose workgroups k_cfl_rings_bc holds back behind the
    boundary workgroups' stamp (they read v_r rows 1 and nr-1, which the boundary call rewrites).  Each plant is sized
    by Planter from the base dt (MERGED_TIGHTEN times tighter), and the numpy restatement, fed the oracle's grids
    ahead of every one of the three steps, must find dt in the planted ring through the planted term each time -- so
    a merged kernel that drops or reads stale one of the held-back rings, or a fold that loses its partial maximum,
    returns another dt in steps 2 and 3, which ride in k_cfl_rings_bc.

    A jump of at most 2 c_s cannot bind in ring nr-2: against the shear limit of ring pair (0, 1) it takes 6.9 c_s at
    32 x 320 and 9.2 c_s at 24 x 2050 (0.5 and 0.7 c_s in ring 1; e x 10 to x 1800).  Such jumps are no benign start
    at a CFL number of 0.5, and at 2050 cells per ring even the one in ring 1 is not (cells 27 times longer in r than
    in phi: the oracle's dt goes 2e-3, 5e-8, 1e-10).  The binding structure does not depend on the CFL number, so all
    cases run at MERGED_CFL = 0.02, where the oracle's dt changes by at most a factor 2.4 per step and the planted ring
    binds throughout (measured on the CPU)."""
    ring = 1 if where == "ring1" else nr - 2
    d0, radii, g, base = CP.base_state(product, CP.case_desc(product, nr, nphi, ideal))
    d0.first_dt, d0.cfl_max_var = 1.0, 1.0e3   # CalculateTimeStep takes the CFL value at every step, not 1.1 x the step before
    d0.cfl = MERGED_CFL
    res = CP.condition_cfl(d0, g, base)        # (the base dt of the descriptor the plants run with)
    planter = CP.Planter(d0, g, base, res, tighten=MERGED_TIGHTEN)
    names = product.kernel_names()
    for p in [planter.vphi(ring, 41, -1)] + ([planter.e(ring, 129)] if ideal else []):
        st = {k: v.copy() for k, v in base.items()}
        p.apply(st)
        planted = CP.condition_cfl(d0, g, st)
        b = planted.binding()
        assert b[:3] == p.bind and b[3] == p.term and b[1] == ring, f"{p.name}: meant {p.bind} {p.term}, binds {b}"
        assert planted.dt <= 0.75 * res.dt, f"{p.name}: dt only {planted.dt / res.dt:.3f} of the base dt"
        fields = tuple(st[k] for k in ("sigma", "vrad", "vazi", "energy"))

        def run(lib, mode, fold=None):
            ctx = driver.make_context(lib, d0, fields=fields, radii=radii)
            try:
                S = driver.SlabSet([ctx])
                S.prepare()
                dts = []
                if mode == "host":
                    for k in range(3):
                        if lib is oracle:   # where does this step's dt come from?
                            r = CP.condition_cfl(d0, g, _grids(ctx, d0))
                            bk = r.binding()
                            assert bk[0] == "cell" and bk[1] == ring and bk[3] == p.term, \
                                f"{p.name}, step {k}: dt no longer comes from ring {ring} through {p.term}: {bk}"
                        dts.append(S.step())
                        if lib is oracle:
                            assert abs(dts[-1] - r.dt) <= 1e-13 * r.dt, (p.name, k, dts[-1], r.dt)
                else:
                    ctx.set_option("graph_steps", 0)
                    ctx.set_option("bc_in_cfl", 2)
                    ctx.set_option("cfl_fold_in_source", fold)
                    ctx.profile_start([names.index("k_cfl_rings_bc"), names.index("k_cfl_final")], max_launches=32)
                    assert ctx.run_steps(3) == 3
                    prof = ctx.profile_stop()
                    assert prof.get("k_cfl_rings_bc", (0, 0))[1] == 2, prof   # steps 2 and 3 carry the call of the step before
                    folds = prof.get("k_cfl_final", (0, 0))[1]
                    assert (folds < 3) if fold else (folds >= 3), (fold, prof)   # (on: the source kernel folds)
                return ctx.state(), ctx.clock.time, dts
            finally:
                ctx.close()

        ref = run(oracle, "host")
        host = run(product, "host")
        for k, (x, y) in enumerate(zip(host[2], ref[2])):
            assert abs(x - y) <= TOL_DT * y, f"{p.name}, step {k}: dt {x!r} (HIP) vs {y!r} (oracle), {abs(x - y) / y:.2e}"
        for fold in (1, 0):
            got = run(product, "merged", fold)
            assert got[1] == host[1], f"{p.name}, fold {fold}: clock {got[1]!r} vs {host[1]!r}"
            for k in host[0]:
                assert np.array_equal(got[0][k], host[0][k]), f"{p.name}, fold {fold}: {k} differs from the host loop's"
