"""The numpy restatement of the particle step passes the reference's own known-answer test, test/dust_drift: twelve
grain sizes drifting inward from 1 au through a frozen power-law disk must match Nakagawa's drift speed within 1 %
(calc_deviation.py).  No GPU: the gas comes from fcpt_initial_fields, H and T from the isothermal definitions.

The deviations of the restatement (100 orbits, dt = 0.628318531 / 16) are printed beside the reference's
deviations.txt and recorded in DESIGN.md section 3."""
import json
import os

import numpy as np

import fargocpt_amd

import tests.particles_cases as cases
import tests.particles_ref as R


def sample_drift(advance, ids, first):
    """(t, r, stokes, alive) at every DRIFT_SAMPLE; advance(nsteps) -> the live particles as a dict with "id"."""
    nsamples = int(round(cases.DRIFT_ORBITS * 2.0 * np.pi / cases.DRIFT_SAMPLE))
    t = np.arange(nsamples + 1) * (cases.DRIFT_SUBSTEPS * cases.DRIFT_DT)
    r, st = np.ones((nsamples + 1, ids.size)), np.ones((nsamples + 1, ids.size))
    alive = np.zeros((nsamples + 1, ids.size), dtype=bool)
    now = first
    for k in range(nsamples + 1):
        if k:
            now = advance(cases.DRIFT_SUBSTEPS)
        col = np.searchsorted(ids, now["id"])
        r[k, col], st[k, col], alive[k, col] = now["r"], now["stokes"], True
    return t, r, st, alive


def restatement_drift(lib):
    d, radii, (sigma, vrad, vazi, _), prm, bodies, s = cases.drift_case(lib)
    g = R.Grid(radii, d.nr_global, d.nphi)
    gas = cases.isothermal_gas(d, g, sigma, vrad, vazi)
    phys = R.physics(d, prm)
    s["stokes"] = R.initial_stokes(g, gas, phys, s)

    def advance(nsteps):
        for _ in range(nsteps):
            guards, _ = R.step(g, gas, phys, bodies, s, cases.DRIFT_DT)
            assert not guards.any()
        return R.live(s)

    return sample_drift(advance, s["id"].copy(), R.live(s))


def test_drift_speed_matches_nakagawa_within_one_per_cent():
    stokes, dev = cases.drift_deviations(*restatement_drift(fargocpt_amd.load()))
    print("Stokes number, deviation of the restatement | the reference's deviations.txt")
    for s, q, (s_ref, q_ref) in zip(stokes, dev, cases.DRIFT_REFERENCE_DEVIATIONS):
        print(f"{s:.6e} {q:+.6e} | {s_ref:.6e} {q_ref:+.6e}")
    assert np.all(np.abs(dev) < cases.DRIFT_TOLERANCE), dev
    # the recorded copy that test_gpu_particles_drift.py compares the device with is this run's
    # (FCPT_UPDATE_GOLDEN=1 in the environment rewrites it from this run instead)
    if os.environ.get("FCPT_UPDATE_GOLDEN") == "1":
        with open(GOLDEN, "w") as f:
            json.dump({"comment": "mean Stokes number and deviation from Nakagawa's drift speed of tests/particles_ref.py, 100 orbits "
                                  "at dt = 0.628318531 / 16; written by tests/test_particles_ref_drift.py with FCPT_UPDATE_GOLDEN=1",
                       "stokes": [float(x) for x in stokes], "deviation": [float(x) for x in dev]}, f, indent=1)
    gold = drift_golden()
    assert np.allclose(dev, gold["deviation"], rtol=0.0, atol=1e-9) and np.allclose(stokes, gold["stokes"], rtol=1e-9, atol=0.0)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dust_drift_restatement.json")


def drift_golden():
    with open(GOLDEN) as f:
        return json.load(f)
