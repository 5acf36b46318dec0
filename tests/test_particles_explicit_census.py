"""The cases of the GPU tests of the explicit integrator reach the branches they are meant to reach, by count in the
restatement, and the yardstick for timestep and facold is what tests/particles_explicit_cases.py records: the restatement
in float64 against itself in longdouble on the parity case (isothermal initial gas; drag on / off, polar / Cartesian)."""
import numpy as np
import pytest

import fargocpt_amd
from fargocpt_amd import setups

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X


@pytest.fixture(scope="module")
def lib():
    return fargocpt_amd.load()


@pytest.mark.parametrize("drag,cartesian", [(False, False), (False, True), (True, False), (True, True)])
def test_parity_case_reaches_its_branches_and_measures_the_yardstick(lib, drag, cartesian):
    census = {}
    (a, b), (ha, hb), most = xc.restatement_runs(lib, drag, cartesian, census)
    print("drag=%d cartesian=%d: %s; at most %d substeps per particle and call" % (drag, cartesian, census, most))
    assert most * 100 <= X.MAX_ATTEMPTS             # two orders of magnitude below the cap
    assert census["clipped_last"] >= 7000 and census["fac_ge_1_rule"] >= 7000
    assert census["escape_inward"] >= 5 and census["escape_outward"] >= 5
    if drag:
        assert census["drag_skipped_below_rmin"] >= 5 and census["drag_skipped_above_rmax"] >= 5
        assert census["drag_on_rmin"] == 1 and census["drag_on_rmax"] == 1     # r = RMIN and r = RMAX are kicked: r < RMIN skips
        # every regime of calc_tstop: the four branches of the Stokes coefficient (Re <= 1e-3 by the ten particles planted
        # on the gas's own velocity) and both Knudsen regimes (Kn > 1 by the boulders of 10 cm to 1 m)
        assert min(census[k] for k in ("Re<=500", "Re<=1500", "Re>1500", "Kn<1", "Kn>1")) >= 100 and census["Re<=1e-3"] >= 10
    # the two restatements agree on the substep counts of all but 0.2 % of the particles ...
    mism = xc.count_mismatch(ha, hb)
    assert mism.mean() <= xc.COUNT_MISMATCH_RESTATEMENTS, int(mism.sum())
    # ... and on timestep and facold of the others within the recorded yardsticks
    both = a["alive"] & b["alive"] & ~mism
    ts = xc.relative_difference(a["timestep"][both], b["timestep"][both])
    fo = xc.relative_difference(a["facold"][both], b["facold"][both])
    print("float64 against longdouble: timestep %.3e, facold %.3e, %d count mismatches" % (ts, fo, mism.sum()))
    assert ts <= xc.YARDSTICK_TIMESTEP * 1.05 and fo <= xc.YARDSTICK_FACOLD * 1.05
    # r_ddot and phi_ddot are well conditioned in this case (they are not where a controlled step size splits a call)
    both_alive = a["alive"] & b["alive"]
    for k in ("r_ddot", "phi_ddot"):
        x, y = np.asarray(a[k][both_alive], dtype=np.float64), np.asarray(b[k][both_alive], dtype=np.float64)
        gap = float(np.abs(x - y).max() / np.abs(y).max())
        print("%s of the two restatements: %.3e" % (k, gap))
        assert gap <= xc.ACCELERATION_CONDITIONING, (k, gap)
    # the state itself is well conditioned
    la, lb = X.live(a), X.live(b)
    diff = X.worst_difference_cartesian(la, lb) if cartesian else R.worst_difference(la, lb)
    assert max(diff.values()) <= 1e-12, diff


def test_stiff_grain_trips_guard_10(lib):
    d = cases.parity_desc(lib, 48, 256)
    radii = lib.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    sigma, vrad, vazi, _ = lib.initial_fields(d, radii)
    gas = cases.isothermal_gas(d, g, sigma, vrad, vazi)
    phys = X.physics(d, cases.parity_params(lib, d, False))
    s = xc.explicit_draw(d, radii, n=65)
    s["radius"][40] = xc.STIFF_GRAIN
    s["stokes"] = R.initial_stokes(g, gas, phys, s)
    X.add_adaptive(s)
    bodies = setups.jupiter_bodies(d)
    X.init_timestep(phys, bodies, s)
    before = {k: s[k].copy() for k in X.STATE}
    census = {}
    guards = X.step(g, gas, phys, bodies, s, xc.EXPLICIT_DT, census=census)
    assert guards[40] == X.GUARD_STIFF and np.count_nonzero(guards) == 1 and census["guard_stiff"] == 1
    for k in X.STATE:
        assert s[k][40] == before[k][40], k


def test_encounter_lane_needs_many_times_the_substeps_of_its_wavefront(lib):
    d = cases.parity_desc(lib, 48, 256)
    radii = lib.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    H = d.aspect_ratio * g.rmed ** (1.0 + d.flaring_index)
    fields = {"H": H[:, None] * np.ones((g.nr, g.nphi))}
    phys = X.physics(d, cases.parity_params(lib, d, False))
    bodies = setups.jupiter_bodies(d)
    runs = [xc.encounter_wavefront(d, radii) for _ in range(2)]
    dtypes = (np.float64, np.longdouble)
    for s, dtype in zip(runs, dtypes):
        X.init_timestep(phys, bodies, s, False, dtype)
    worst = 0.0
    for call in range(xc.ENCOUNTER_CALLS):
        for s, dtype in zip(runs, dtypes):
            assert not X.step(g, fields, phys, bodies, s, xc.ENCOUNTER_DT, drag=False, dtype=dtype).any()
        s = runs[0]
        sub = (s["accepted"] + s["rejected"]).astype(int)
        others = np.delete(sub, xc.ENCOUNTER_LANE)
        print("call %d: substeps of the encounter lane: %d, of the others: mean %.1f, max %d" % (call, sub[xc.ENCOUNTER_LANE], others.mean(), others.max()))
        # in every call: many times its neighbours, and two orders of magnitude below the attempt cap
        assert sub[xc.ENCOUNTER_LANE] >= 4 * others.mean() and sub[xc.ENCOUNTER_LANE] > others.max()
        assert sub.max() * 100 <= X.MAX_ATTEMPTS
        worst = max(worst, xc.acceleration_gap(runs[0], runs[1]))
    print("r_ddot, phi_ddot, float64 against longdouble: %.3e" % worst)
    assert worst <= xc.ENCOUNTER_ACCELERATION_YARDSTICK * 1.05
    # conditioning of the state in the encounter: what a parity bar of 1e-10 can tell from an error
    diff = R.worst_difference(X.live(runs[0]), X.live(runs[1]))
    print("float64 against longdouble:", diff)
    assert max(diff.values()) <= 1e-11, diff


@pytest.mark.parametrize("cartesian", [False, True])
def test_planted_step_sizes_reach_rejections_and_acceptances_after_them(lib, cartesian):
    """The sequence of test_the_step_size_persists_between_calls_of_different_dt: the parity case itself rejects nothing."""
    d = cases.parity_desc(lib, 48, 256)
    radii = lib.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    H = d.aspect_ratio * g.rmed ** (1.0 + d.flaring_index)
    fields = {"H": H[:, None] * np.ones((g.nr, g.nphi))}
    phys = X.physics(d, cases.parity_params(lib, d, False))
    bodies = setups.jupiter_bodies(d)
    snaps, most = ([], []), [0]
    for k, dtype in enumerate((np.float64, np.longdouble)):
        def after(s, k=k):
            snaps[k].append({key: np.array(v) for key, v in s.items()})
            most[0] = max(most[0], int((s["accepted"] + s["rejected"])[s["alive"]].max()))
        s, c = xc.step_size_sequence(d, radii, cartesian, lambda s: X.init_timestep(phys, bodies, s, cartesian, dtype),
                                     lambda s, dt, census: X.step(g, fields, phys, bodies, s, dt, drag=False, cartesian=cartesian,
                                                                  census=census, dtype=dtype), after=after)
        if k == 0:
            census = c
    gaps = [xc.acceleration_gap(a, b) for a, b in zip(*snaps)]
    print(census, "at most %d substeps per particle and call; r_ddot, phi_ddot float64 against longdouble per call:" % most[0], gaps)
    assert most[0] * 100 <= X.MAX_ATTEMPTS
    assert max(gaps) <= xc.STEP_SIZE_ACCELERATION_YARDSTICK * 1.05
    assert census["rejection"] >= 200 and census["accepted_after_rejection"] >= 200 and census["clipped_last"] >= 700
