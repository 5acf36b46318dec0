"""The N-body step of the host library (fcpt_nbody_*): needs no GPU.

The accuracy bar is the reference's own: its test `circ_kepler_orbit` (setup and threshold kept verbatim under
tests/golden/circ_kepler_orbit/) asks for 1e-11 in the planet's position over 20 orbits taken in 2000 steps."""
import os

import numpy as np
import pytest
import yaml

from fargocpt_amd import binding as B

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "circ_kepler_orbit")

# What test 1 measures for the circular orbit: max |r - r_exact| = 1.97e-12 after 20 periods, i.e. 9.9e-14 per period
# (an along-track drift: a relative error of 1.6e-14 in the mean motion).  Rounded to 1e-13 it is the yardstick of the
# eccentric case below.
PER_PERIOD_ERROR = 1e-13


def _two_body(product, m2, e):
    s = product.nbody(1.0)
    s.add(1.0)
    s.add(m2, 1.0, e)
    return s


def test_circular_kepler_orbit_reference_criterion(product):
    """test/circ_kepler_orbit of the reference (nbody_test.yml: star 1, planet 1e-3 at a = 1, e = 0, Nmonitor steps
    of MonitorTimestep; check_results.py: planet against (cos Omega t, sin Omega t), Omega = sqrt(1 + 1e-3), threshold
    of testconfig.yml).  The reference's frame is centred on the star: the position is taken relative to it.
    Measured: 1.97e-12."""
    with open(os.path.join(GOLDEN, "nbody_test.yml")) as f:
        cfg = yaml.safe_load(f)
    with open(os.path.join(GOLDEN, "testconfig.yml")) as f:
        threshold = float(yaml.safe_load(f)["threshold"])
    assert threshold == 1e-11
    star, planet = cfg["nbody"]
    nsteps, dt = int(cfg["Nmonitor"]) * int(cfg["Nsnapshots"]), float(cfg["MonitorTimestep"])
    assert (nsteps, dt) == (2000, 0.06283185307179586)
    m1, m2 = float(star["mass"]), float(planet["mass"])
    assert (m1, m2, float(planet["eccentricity"])) == (1.0, 1e-3, 0.0)
    s = _two_body(product, m2, 0.0)
    om = np.sqrt(1.0 + 1e-3)
    worst = 0.0
    for k in range(1, nsteps + 1):
        s.advance(dt)
        st = s.state
        t = k * dt
        worst = max(worst, abs(st[1, 0] - st[0, 0] - np.cos(om * t)), abs(st[1, 1] - st[0, 1] - np.sin(om * t)))
    print(f"circular orbit, {nsteps} steps: max deviation {worst:.3e} (threshold {threshold:g})")
    assert worst <= threshold


def _kepler_position(t, e, mu):
    M = np.sqrt(mu) * t
    E = M
    for _ in range(60):
        E = E - (E - e * np.sin(E) - M) / (1.0 - e * np.cos(E))
    return np.cos(E) - e, np.sqrt(1.0 - e * e) * np.sin(E)


def test_eccentric_orbit_uneven_steps(product):
    """e = 0.3, 20 periods, step lengths drawn log-uniformly from [1e-3, 0.1] by a seeded generator.  Bound: the
    per-period error of the circular case (PER_PERIOD_ERROR, measured there) x 20 periods x a margin of 10 = 2e-11,
    for the relative energy and angular-momentum errors and for the position against the Kepler-equation solution.
    Measured: energy 2.3e-14, angular momentum 1.2e-14, position 8.3e-13 (5867 steps)."""
    e, m2 = 0.3, 1e-3
    mu = 1.0 + m2
    bound = PER_PERIOD_ERROR * 20 * 10
    s = _two_body(product, m2, e)
    rng = np.random.default_rng(7)
    t_end = 20 * 2 * np.pi / np.sqrt(mu)

    def invariants(st):
        rel, vel = st[1, :2] - st[0, :2], st[1, 2:4] - st[0, 2:4]
        return 0.5 * vel @ vel - mu / np.hypot(*rel), rel[0] * vel[1] - rel[1] * vel[0]

    e0, l0 = invariants(s.state)
    t, nsteps, worst_e, worst_l, worst_x = 0.0, 0, 0.0, 0.0, 0.0
    while t < t_end:
        dt = float(np.exp(rng.uniform(np.log(1e-3), np.log(0.1))))
        s.advance(dt)
        t += dt
        nsteps += 1
        st = s.state
        en, l = invariants(st)
        x, y = _kepler_position(t, e, mu)
        worst_e = max(worst_e, abs(en / e0 - 1.0))
        worst_l = max(worst_l, abs(l / l0 - 1.0))
        worst_x = max(worst_x, abs(st[1, 0] - st[0, 0] - x), abs(st[1, 1] - st[0, 1] - y))
    print(f"eccentric orbit, {nsteps} steps: energy {worst_e:.3e}, angular momentum {worst_l:.3e}, position {worst_x:.3e} "
          f"(bound {bound:g})")
    assert worst_e <= bound and worst_l <= bound and worst_x <= bound


def _three_bodies(product):
    s = product.nbody(1.0)
    s.add(1.0)
    s.add(1e-3, 1.0, 0.1)
    s.add(3e-4, 1.7, 0.05, 0.4, 2.0)
    return s


def test_three_bodies_momentum_and_state(product):
    """Total linear momentum to rounding; the trial advance of centre_delta_v leaves the state bit-identical;
    get/set of the state reproduces a following advance bit for bit; kick adds exactly a dt."""
    s = _three_bodies(product)
    assert len(s) == 3
    st0 = s.state
    p0 = (st0[:, 4:5] * st0[:, 2:4]).sum(axis=0)
    pscale = np.abs(st0[:, 4:5] * st0[:, 2:4]).sum()
    for _ in range(200):
        s.advance(0.05)
    st = s.state
    p1 = (st[:, 4:5] * st[:, 2:4]).sum(axis=0)
    # 200 steps of a few dozen force evaluations each, every one rounding m_i a_i and m_j a_j separately
    assert np.abs(p1 - p0).max() <= 200 * 64 * np.finfo(float).eps * pscale, (p0, p1)

    before = s.state.copy()
    dv = s.centre_delta_v(1, 0.05)
    assert np.array_equal(s.state, before)
    assert np.all(np.isfinite(dv)) and np.abs(dv).max() > 0.0
    assert np.array_equal(s.centre_delta_v(1, 0.05), dv)
    # ... and it is the star's velocity change over the advance
    t = product.nbody(1.0)
    t.state = before
    assert np.array_equal(t.state, before)
    s.advance(0.05)
    t.advance(0.05)
    assert np.array_equal(s.state, t.state)
    assert np.array_equal(s.state[0, 2:4] - before[0, 2:4], dv)

    ax, ay, dt = np.array([1e-5, -2e-3, 0.25]), np.array([0.0, 3e-4, -0.125]), 0.03125
    before = s.state.copy()
    s.kick(ax, ay, dt)
    after = s.state
    assert np.array_equal(after[:, 2], before[:, 2] + ax * dt) and np.array_equal(after[:, 3], before[:, 3] + ay * dt)
    assert np.array_equal(after[:, [0, 1, 4]], before[:, [0, 1, 4]])


def test_placement_shift_and_rotation(product):
    """The first pair sits about its barycentre with the elements between them; shift_to_centre(1) puts the first
    body at rest at the origin; rotate turns positions and velocities alike."""
    s = _two_body(product, 1e-3, 0.3)
    st = s.state
    m = st[:, 4]
    assert np.abs((m[:, None] * st[:, :4]).sum(axis=0)).max() <= 1e-18
    assert np.allclose(st[1, :2] - st[0, :2], [0.7, 0.0], rtol=0, atol=4e-16)          # pericentre a (1 - e)
    assert np.isclose(st[1, 3] - st[0, 3], np.sqrt(1.001 * 1.3 / 0.7), rtol=1e-15)     # vis-viva there
    s.shift_to_centre(1)
    st = s.state
    assert np.array_equal(st[0, :4], np.zeros(4))
    s.rotate(np.pi / 2)
    r = s.state
    assert np.allclose(r[1, :2], [-st[1, 1], st[1, 0]], rtol=0, atol=1e-16)
    assert np.allclose(r[1, 2:4], [-st[1, 3], st[1, 2]], rtol=0, atol=1e-16)
    with pytest.raises(B.FcptError):
        s.shift_to_centre(3)
    with pytest.raises(B.FcptError):
        s.centre_delta_v(0, 0.1)
