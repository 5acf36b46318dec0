"""The restatement of the explicit adaptive integrator on the reference's known-answer test, test/dust_drift: the grains
of cases.drift_case whose initial t_stop is at least 10 DRIFT_DT (the explicit kick's condition, guard 10) drift inward
from 1 au through the frozen power-law disk at Nakagawa's speed within 1 %.  The state is Cartesian, as the reference's
setup has it (CartesianParticles: yes).  The deviations are printed beside the midpoint restatement's golden values for
the same grains and pinned in tests/golden/dust_drift_explicit_restatement.json (FCPT_UPDATE_GOLDEN=1 rewrites it)."""
import json
import os

import numpy as np

import fargocpt_amd

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X
from tests.test_particles_ref_drift import drift_golden, sample_drift

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dust_drift_explicit_restatement.json")


def explicit_drift_case(lib):
    """-> (desc, radii, fields, params, bodies, gas, physics, Cartesian state of the qualifying grains, their indices)"""
    d, radii, fields, prm, bodies, s = cases.drift_case(lib)
    g = R.Grid(radii, d.nr_global, d.nphi)
    gas = cases.isothermal_gas(d, g, fields[0], fields[1], fields[2])
    phys = X.physics(d, prm)
    s["stokes"] = R.initial_stokes(g, gas, phys, s)
    keep = np.flatnonzero(s["stokes"] / R.omega_kepler(phys, s["r"]) >= 10.0 * cases.DRIFT_DT)
    s = {k: v[keep].copy() for k, v in s.items()}
    return d, radii, fields, prm, bodies, g, gas, phys, X.add_adaptive(xc.to_cartesian(s)), keep


def polar_view(p):
    """r and stokes for sample_drift from a Cartesian state."""
    return {"id": p["id"], "r": np.hypot(p["r"], p["phi"]), "stokes": p["stokes"]}


def explicit_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_explicit_drift_speed_matches_nakagawa_within_one_per_cent():
    d, radii, fields, prm, bodies, g, gas, phys, s, keep = explicit_drift_case(fargocpt_amd.load())
    assert keep.size >= 4, keep
    X.init_timestep(phys, bodies, s, True)
    most, calls, stiff = [0], [0], {}

    def advance(nsteps):
        for _ in range(nsteps):
            guards = X.step(g, gas, phys, bodies, s, cases.DRIFT_DT, drag=True, cartesian=True)
            # the condition of guard 10 is held at every step: a grain that drifts into denser gas until t_stop < 10 dt is
            # refused from then on, and its series ends there like that of a grain that leaves the domain
            assert np.all((guards == 0) | (guards == X.GUARD_STIFF)), guards
            for slot in np.flatnonzero(guards):
                stiff.setdefault(int(s["id"][slot]), calls[0])
                s["alive"][slot] = False
            calls[0] += 1
            most[0] = max(most[0], int((s["accepted"] + s["rejected"])[s["alive"]].max(initial=0)))
        return polar_view(X.live(s))

    stokes, dev = cases.drift_deviations(*sample_drift(advance, s["id"].copy(), polar_view(X.live(s))))
    mid = drift_golden()
    print("at most %d substeps per particle and call; grains refused by guard 10 (id: call): %s" % (most[0], stiff))
    done = np.array([int(i) not in stiff for i in s["id"]])
    assert done.sum() >= 4, stiff
    print("Stokes number, deviation of the explicit restatement | of the midpoint restatement")
    for k, st, q in zip(keep, stokes, dev):
        print(f"{st:.6e} {q:+.6e} | {mid['stokes'][k]:.6e} {mid['deviation'][k]:+.6e}")
    assert most[0] * 100 <= X.MAX_ATTEMPTS
    assert np.all(np.abs(dev[done]) < cases.DRIFT_TOLERANCE), dev
    keep, stokes, dev = keep[done], stokes[done], dev[done]      # the recorded grains: those that complete the 100 orbits
    if os.environ.get("FCPT_UPDATE_GOLDEN") == "1":
        with open(GOLDEN, "w") as f:
            json.dump({"comment": "mean Stokes number and deviation from Nakagawa's drift speed of tests/particles_explicit_ref.py "
                                  "(Cartesian state) for the grains of drift_case with t_stop >= 10 dt throughout, 100 orbits at dt = "
                                  "0.628318531 / 16; written by tests/test_particles_explicit_drift.py with FCPT_UPDATE_GOLDEN=1",
                       "grains": [int(k) for k in keep], "stokes": [float(x) for x in stokes],
                       "deviation": [float(x) for x in dev]}, f, indent=1)
    gold = explicit_golden()
    assert gold["grains"] == [int(k) for k in keep]
    assert np.allclose(dev, gold["deviation"], rtol=0.0, atol=1e-9) and np.allclose(stokes, gold["stokes"], rtol=1e-9, atol=0.0)
