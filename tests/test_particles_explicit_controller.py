"""The step-size controller and init_particle_timestep of tests/particles_explicit_ref.py against values computed by hand:
a scalar Cash-Karp substep written out in this file in plain Python floats, and the controller's formulas applied to its
err one decision at a time, as particles.cpp:1724-2011 writes them -- including the aliasing of :1726 (old_timestep is
the stored step, which holds the new value after :1981, so a rejection divides it twice).

Cartesian state, star only: the right-hand side needs sqrt alone, which is correctly rounded everywhere, so the two
implementations must agree to the last bits (tolerance 1e-15 relative)."""
import math

import numpy as np

import tests.particles_ref as R
import tests.particles_explicit_ref as X

TOL = 1e-15
PRM = {"G": 1.0, "Mc": 1.0, "alpha": 0.0, "thickness_smoothing": 0.0, "omega_frame": 0.0, "escape_radius_min": 0.1,
       "escape_radius_max": 10.0}
BODIES = ([0.0], [0.0], [1.0])
GRID = R.Grid(np.linspace(0.1, 10.0, 34), 33, 16)
FIELDS = {"H": np.full((33, 16), 0.05)}


def rhs(y, gm=1.0, eps_sq=0.0):
    dx, dy = 0.0 - y[0], 0.0 - y[1]
    r2 = dx * dx + dy * dy
    r2 = r2 + eps_sq
    r = math.sqrt(r2)
    factor = gm / (r * r2)
    return [y[2], y[3], 0.0 + factor * dx, 0.0 + factor * dy]


def substep(y, ts):
    """-> (new state, slope of the velocities, err)"""
    k1 = rhs(y)
    k2 = rhs([y[j] + ts * 0.2 * k1[j] for j in range(4)])
    k3 = rhs([y[j] + ts * (0.075 * k1[j] + 0.225 * k2[j]) for j in range(4)])
    k4 = rhs([y[j] + ts * (0.3 * k1[j] - 0.9 * k2[j] + 1.2 * k3[j]) for j in range(4)])
    k5 = rhs([y[j] + ts * (-11.0 / 54.0 * k1[j] + 2.5 * k2[j] - 70.0 / 27.0 * k3[j] + 35.0 / 27.0 * k4[j]) for j in range(4)])
    k6 = rhs([y[j] + ts * (1631.0 / 55296.0 * k1[j] + 175.0 / 512.0 * k2[j] + 575.0 / 13824.0 * k3[j] + 44275.0 / 110592.0 * k4[j] +
                           253.0 / 4096.0 * k5[j]) for j in range(4)])
    slope = [37.0 / 378.0 * k1[j] + 250.0 / 621.0 * k3[j] + 125.0 / 594.0 * k4[j] + 512.0 / 1771.0 * k6[j] for j in range(4)]
    new = [y[j] + ts * slope[j] for j in range(4)]
    e1, e3 = 37.0 / 378.0 - 2825.0 / 27648.0, 250.0 / 621.0 - 18575.0 / 48384.0
    e4, e5, e6 = 125.0 / 594.0 - 13525 / 55296.0, -277.0 / 14336.0, 512.0 / 1771.0 - 1.0 / 4.0
    err = 0.0
    for j in range(4):
        est = ts * (e1 * k1[j] + e3 * k3[j] + e4 * k4[j] + e5 * k5[j] + e6 * k6[j])
        sq = est / (1e-14 + 1e-12 * max(abs(y[j]), abs(new[j])))
        err = err + sq * sq
    return new, slope, math.sqrt(err / 4.0)


def power(x, y):
    """numpy's pow: the controller amplifies a last-bit difference in a step size a millionfold (err is a cancellation), so
    the hand computation must use the same library function as the restatement."""
    return float(np.power(np.float64(x), y))


def by_hand(y, stored, facold, dt):
    """The reference's loop, one decision per pass.  -> (state, stored timestep, facold, log of (kind, clipped, forced))"""
    expo1 = 0.2 - 0.04 * 0.75
    elapsed, last, reject, log = 0.0, False, False, []
    while not last:
        timestep, update = stored, True
        if elapsed + timestep * 1.01 > dt:
            timestep, last, update = dt - elapsed, True, False
        new, _, err = substep(y, timestep)
        fac11 = power(err, expo1)
        fac = fac11 / power(facold, 0.04)
        fac = max(0.1, min(5.0, fac / 0.9))
        forced = (not update) and fac < 1.0
        if not update:
            fac = max(fac, 1.0)
        before = stored
        stored = stored / fac                        # particles[i].timestep = old_timestep / fac: old_timestep is `stored`
        if err <= 1.0:
            facold = max(err, 1.0e-4)
            elapsed += timestep
            y = new
            if reject:
                stored = min(abs(stored), abs(stored))
                assert stored == before / fac          # changes nothing
            log.append(("accepted after rejection" if reject else "accepted", not update, forced))
            reject = False
        else:
            stored = stored / min(5.0, fac11 / 0.9)    # ... so this is the second division
            assert stored == before / fac / min(5.0, fac11 / 0.9)
            reject, last = True, False
            log.append(("rejected", not update, forced))
    return y, stored, facold, log


def _plant(h, facold, dt):
    y0 = [1.0, 0.0, 0.0, 1.0]
    s = R.make_state([3], [y0[0]], [y0[1]], [y0[2]], [y0[3]], [1.0], [1e30])
    X.add_adaptive(s, [h], [facold])
    guards = X.step(GRID, FIELDS, PRM, BODIES, s, dt, drag=False, cartesian=True)
    assert not guards.any()
    y, stored, fo, log = by_hand(y0, h, facold, dt)
    assert abs(s["timestep"][0] - stored) <= TOL * abs(stored), (s["timestep"][0], stored)
    assert abs(s["facold"][0] - fo) <= TOL * abs(fo), (s["facold"][0], fo)
    for k, v in zip(("r", "phi", "r_dot", "phi_dot"), y):
        assert abs(s[k][0] - v) <= TOL * max(abs(v), 1.0), k
    kinds = [entry[0] for entry in log]
    assert int(s["accepted"][0]) == sum(k != "rejected" for k in kinds) and int(s["rejected"][0]) == kinds.count("rejected")
    return s, log


def test_a_rejection_divides_the_stored_step_twice():
    s, log = _plant(0.9, 1e-4, 1.0)
    assert log[0] == ("rejected", False, False)
    # the first decision alone, from the formulas: err of one substep of 0.9 from the start
    _, _, err = substep([1.0, 0.0, 0.0, 1.0], 0.9)
    fac11 = power(err, 0.2 - 0.04 * 0.75)
    fac = max(0.1, min(5.0, fac11 / power(1e-4, 0.04) / 0.9))
    after_one = 0.9 / fac / min(5.0, fac11 / 0.9)
    assert err > 1.0 and fac == 5.0 and after_one == 0.9 / 5.0 / 5.0      # both divisions saturate at facc1 = 5
    # ... and the next attempt is made with that step
    _, _, err2 = substep([1.0, 0.0, 0.0, 1.0], after_one)
    assert ("rejected" if err2 > 1.0 else "accepted after rejection") == log[1][0]


def test_a_rejection_followed_by_an_acceptance():
    _, log = _plant(0.9, 1e-4, 1.0)
    kinds = [entry[0] for entry in log]
    first = kinds.index("accepted after rejection")
    assert first >= 1 and all(k == "rejected" for k in kinds[:first])


def test_the_clipped_last_substep():
    s, log = _plant(0.004, 1e-4, 0.01)
    assert [entry[1] for entry in log] == [False, False, True]       # 0.004, 0.004, then 0.002 clipped by the 1.01 test
    assert all(entry[0] == "accepted" for entry in log)


def test_the_step_does_not_grow_on_a_clipped_substep():
    s, log = _plant(5e-3, 0.5, 1e-3)
    assert log == [("accepted", True, True)]        # err tiny: fac = 0.1 would grow the step tenfold; forced to 1
    assert s["timestep"][0] == 5e-3 and s["facold"][0] == 1.0e-4


def test_dt_zero_terminates_and_moves_nothing():
    s, log = _plant(5e-3, 0.5, 0.0)
    assert log == [("accepted", True, True)]
    assert (s["r"][0], s["phi"][0], s["r_dot"][0], s["phi_dot"][0]) == (1.0, 0.0, 0.0, 1.0) and s["timestep"][0] == 5e-3


def test_attempt_cap_leaves_the_particle_as_it_was():
    for h in (0.9, float("nan"), 0.0):
        s = R.make_state([3], [1.0], [0.0], [0.0], [1.0], [1.0], [1e30])
        X.add_adaptive(s, [h], [0.5])
        before = {k: s[k].copy() for k in X.STATE}
        guards = X.step(GRID, FIELDS, PRM, BODIES, s, 1.0, drag=False, cartesian=True, max_attempts=3)
        assert guards[0] == X.GUARD_ATTEMPTS
        for k in X.STATE:
            assert np.array_equal(s[k], before[k], equal_nan=True), k


# ---- init_particle_timestep --------------------------------------------------------------------------------------------

def _init(y, mass, cartesian=True):
    s = R.make_state([3], [y[0]], [y[1]], [y[2]], [y[3]], [1.0], [1e30])
    X.add_adaptive(s)
    branch = X.init_timestep(PRM, ([0.0], [0.0], [mass]), s, cartesian)
    assert s["facold"][0] == 1.0e-4
    return s["timestep"][0], branch[0]


def test_starting_step_regular_branch():
    y = [1.0, 0.0, 0.0, 1.0]
    got, branch = _init(y, 1.0)
    eps_sq = 0.05 * 0.05
    k1 = rhs(y, 1.0, eps_sq)
    dnf = sum((f / 1e-12) * (f / 1e-12) for f in k1)
    dny = sum((v / 1e-12) * (v / 1e-12) for v in y)
    h = math.sqrt(dny / dnf) * 0.01
    k2 = rhs([y[j] + h * k1[j] for j in range(4)], 1.0, eps_sq)
    der2 = math.sqrt(sum(((k2[j] - k1[j]) / 1e-12) ** 2 for j in range(4))) / h
    der12 = max(abs(der2), math.sqrt(dnf))
    want = min(100.0 * h, (0.01 / der12) ** (1.0 / 5.0))
    assert branch == "regular" and abs(got - want) <= 1e-14 * want, (got, want)
    assert want == (0.01 / der12) ** 0.2        # Hairer's h1 is the smaller one here


def test_starting_step_degenerate_branches():
    # no mass, at rest: dnf = 0 -> 1e-6; der12 = 0 -> h1 = max(1e-6, 1e-9); min(1e-4, 1e-6)
    got, branch = _init([1.0, 0.0, 0.0, 0.0], 0.0)
    assert branch == "dnf+der12" and got == 1.0e-6
    # a mass of 1e-18: |f| = 1e-18, dnf = 1e-12 <= 1e-10 -> 1e-6; der12 = sqrt(dnf) = 1e-6 -> h1 = 1e4^0.2 = 6.3;
    # min(100 x 1e-6, 6.3)
    got, branch = _init([1.0, 0.0, 0.0, 0.0], 1.0e-18)
    assert branch == "dnf" and got == 100.0 * 1.0e-6
    # the polar form of the first case: no centrifugal term at rest
    got, branch = _init([1.0, 0.3, 0.0, 0.0], 0.0, cartesian=False)
    assert branch == "dnf+der12" and got == 1.0e-6
