"""The last stage of the CFL reduction (cfl_fold_value, kernels/cfl.h) at the ends of its strided loops.

A thread of the folding workgroup takes the partial maxima n = thread, thread + NT, ... and the ring pairs (n, n + 1)
of the shear limit the same way; k_cfl_final folds with NT = 1024 threads, the prologue of the marching source kernel
(option cfl_fold_in_source) with NT = 256.  What can go wrong is an element dropped or read twice where the strides
end: so the ring counts are 20 (most threads idle), 255 / 256 / 257 (a thread count and its neighbours), 600 (ragged:
the last threads hold fewer elements than the first) and 2049 (one ring above eight strides of 256 and two of 1024),
at Nphi = 256.  Planted (tests/cfl_plants.py): the maximum in the last active ring; in the highest ring below it that
the LAST thread of either shape holds; and a v_phi offset that makes the last ring pair the shear limit.  The numpy
restatement says that each plant binds where it is meant to (no GPU needed); cfl() must return its dt, the base dt
must come back bit for bit, and three steps of the device loop must leave the same clock and state whether
k_cfl_final folds or the marching kernel does.

(Written with a batched form of the fold -- every load of a group of elements ahead of the first use -- that gave
these bits too but no measurable step time, profiles/ab_serial_round_trips.txt, and was not kept.)"""
import numpy as np
import pytest

from fargocpt_amd import driver
from tests import cfl_plants as CP

NPHI = 256
NRS = [20, 255, 256, 257, 600, 2049]
FOLD_THREADS = (1024, 256)   # k_cfl_final, the marching kernels
TOL_DT = 1e-12
STEP_CFL = 0.02   # (as MERGED_CFL of tests/test_gpu_cfl_plants.py: the planted jumps are no benign start at 0.5)

_SETUPS = {}


def _last_thread_rings(g):
    """The highest active ring below the last one among the elements of the last thread, for either fold shape."""
    out = set()
    for nt in FOLD_THREADS:
        held = [n for n in range(nt - 1, g.nr, nt) if g.first_active <= n < g.active_size - 1]
        if held:
            out.add(held[-1])
    return sorted(out)


def _setup(product, nr):
    if nr not in _SETUPS:
        d0, radii, g, base = CP.base_state(product, CP.case_desc(product, nr, NPHI))
        d0.first_dt, d0.cfl_max_var = 1.0, 1.0e3   # CalculateTimeStep takes the CFL value at every step
        d0.cfl = STEP_CFL
        res = CP.condition_cfl(d0, g, base)
        planter = CP.Planter(d0, g, base, res)
        plants = [planter.vphi(g.active_size - 1, 41, +1)]
        plants += [planter.vr(i, 129, +1) for i in _last_thread_rings(g)]
        plants.append(planter.shear(CP.shear_pairs(g)[-1]))
        planted = []
        for p in plants:
            p.fields = tuple(sorted({c[0] for c in p.changes}))
            st = {k: v.copy() for k, v in base.items()}
            p.apply(st)
            planted.append(CP.condition_cfl(d0, g, st, base=res, rings=p.rings))
        _SETUPS[nr] = (d0, radii, g, base, res, plants, planted)
    return _SETUPS[nr]


@pytest.mark.parametrize("nr", NRS)
def test_plants_bind_where_they_say(product, nr):
    d0, radii, g, base, res, plants, planted = _setup(product, nr)
    assert g.active_size < nr and CP.shear_pairs(g)[-1] == g.active_size - 1
    if nr in (600, 2049):
        assert len(plants) >= 3, [p.name for p in plants]   # (a last-thread ring of its own)
    for p, r in zip(plants, planted):
        b = r.binding()
        assert b[:3] == p.bind and b[3] == p.term, f"{p.name}: meant {p.bind} {p.term}, binds {b}"
        assert r.dt <= 0.5 * res.dt, f"{p.name}: dt only {r.dt / res.dt:.3f} of the base dt"
    assert plants[0].bind[1] == g.active_size - 1
    assert plants[-1].bind == ("shear", g.active_size - 1, g.active_size)


@pytest.mark.gpu
@pytest.mark.parametrize("nr", NRS)
def test_cfl_of_the_plants(product, nr):
    d0, radii, g, base, res, plants, planted = _setup(product, nr)
    s = CP.Session(product, d0, radii, base)
    try:
        names = product.kernel_names()
        s.ctx.profile_start([names.index("k_cfl_rings"), names.index("k_cfl_final")], max_launches=64)
        dt0 = s.cfl()
        print(f"nr {nr} base: {dt0!r} vs {res.dt!r} ({abs(dt0 - res.dt) / res.dt:.2e})")
        assert abs(dt0 - res.dt) <= TOL_DT * res.dt, (dt0, res.dt)
        for p, r in zip(plants, planted):
            dt = s.cfl(p)
            print(f"nr {nr} {p.name}: {dt!r} vs {r.dt!r} ({abs(dt - r.dt) / r.dt:.2e})")
            assert abs(dt - r.dt) <= TOL_DT * r.dt, (p.name, dt, r.dt)
            assert s.cfl() == dt0, f"the base dt {dt0!r} did not come back after {p.name}"
        prof = s.ctx.profile_stop()
        assert prof.get("k_cfl_rings", (0, 0))[1] > 0 and prof.get("k_cfl_final", (0, 0))[1] > 0, prof
    finally:
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nr", NRS)
def test_fold_in_the_march_leaves_the_bits_of_k_cfl_final(product, nr):
    d0, radii, g, base, res, plants, planted = _setup(product, nr)
    names = product.kernel_names()
    for p in plants:
        st = {k: v.copy() for k, v in base.items()}
        p.apply(st)
        fields = tuple(st[k] for k in ("sigma", "vrad", "vazi", "energy"))
        out = []
        for fold in (1, 0):
            ctx = driver.make_context(product, d0, fields=fields, radii=radii)
            try:
                S = driver.SlabSet([ctx])
                S.prepare()
                ctx.set_option("graph_steps", 0)
                ctx.set_option("cfl_fold_in_source", fold)
                ctx.profile_start([names.index("k_cfl_final")], max_launches=32)
                assert ctx.run_steps(3) == 3
                folds = ctx.profile_stop().get("k_cfl_final", (0, 0))[1]
                assert (folds < 3) if fold else (folds >= 3), (p.name, fold, folds)   # (on: the source kernel folds)
                c = ctx.clock
                out.append((ctx.state(), (c.time, c.last_dt, c.n_hydro_iter)))
            finally:
                ctx.close()
        assert out[0][1] == out[1][1], f"{p.name}: clock {out[0][1]!r} (fold in the march) vs {out[1][1]!r}"
        for k in out[0][0]:
            assert np.array_equal(out[0][0][k], out[1][0][k]), f"{p.name}: {k} differs"
