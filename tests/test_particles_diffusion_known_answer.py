"""The numpy restatement of the diffusion kick passes the reference's own known-answer test, test/dust_diffusion
(Charnoz et al. 2011): 20 500 grains of 1e-5 cm start at r = 10 au in a frozen power-law disk with the gas drag off, so
that the random walk is their only radial motion; after 1000 monitor intervals the histogram of r in 101 bins,
normalised to unit mass, must lie within 0.1 of the largest value from the reference's curve (check_results.py,
testconfig.yml).  No GPU: the gas comes from fcpt_initial_fields, H, T and c_s from the isothermal definitions.

dt: 11 equal steps per monitor interval -- the number of hydro steps the driver's timestepLogging records per interval
for the GPU run of the same setup (mean dt 0.080780; the last step of an interval is cut to end on it).

The margin to 0.1 is thin (0.063 .. 0.081 over six seeds of a 1-D model of the same kicks) and the reference's checker
itself says a failure "could be statistical": the seed is fixed and must be one for which the restatement gives
<= 0.09 -- a condition on the choice of seed, checked here.  Also held: std(r) within 2 % of sqrt(2 D t) = 0.4553, four
times the 1 / sqrt(2 N) = 0.49 % sampling error.  About four minutes of numpy (11 000 steps of 20 500 particles)."""
import json
import os

import numpy as np
import pytest

import fargocpt_amd

import tests.particles_diffusion_cases as dcases
import tests.particles_diffusion_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dust_diffusion_restatement.json")
REFERENCE = os.path.join(HERE, "golden", "dust_diffusion_reference_data.txt")


def reference_rows():
    return np.loadtxt(REFERENCE)


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def final_state():
    d, g, gas, phys, bodies, s = dcases.known_answer_case(fargocpt_amd.load())
    dt = dcases.KA_MONITOR / dcases.KA_SUBSTEPS
    for k in range(dcases.KA_INTERVALS * dcases.KA_SUBSTEPS):
        guards, _ = D.step(g, gas, phys, bodies, s, dt, gas_drag=False, diffusion=True, seed=dcases.KA_SEED, step_no=k)
        assert not guards.any()
    return s


def test_the_fixtures_are_the_references(final_state):
    assert reference_rows().shape == (1272, 2)
    assert "ParticleDustDiffusion: 'yes'" in open(os.path.join(HERE, "golden", "setups", "dust_diffusion.yml")).read()


def test_restatement_passes_the_references_check(final_state):
    s = final_state
    r = s["r"][s["alive"]]
    value, fullest = dcases.known_answer_criterion(r, reference_rows())
    out = {"criterion": value, "mean": float(r.mean()), "std": float(r.std()), "live": int(r.size), "fullest_bin": fullest}
    print("restatement: criterion %.4f (threshold %.1f, seed condition 0.09), mean r %.4f, std %.4f (sqrt(2 D t) = %.4f), "
          "%d live, fullest bin %d" % (value, dcases.KA_THRESHOLD, out["mean"], out["std"], dcases.KA_STD, r.size, fullest))
    assert value < dcases.KA_THRESHOLD
    assert value <= 0.09, "choose another seed: this one leaves no margin to the threshold"
    assert abs(out["std"] / dcases.KA_STD - 1.0) <= 0.02
    # the recorded copy that test_gpu_driver_dust_diffusion.py compares the device with is this run's
    # (FCPT_UPDATE_GOLDEN=1 in the environment rewrites it from this run instead)
    if os.environ.get("FCPT_UPDATE_GOLDEN") == "1":
        with open(GOLDEN, "w") as f:
            json.dump(dict(out, comment="test/dust_diffusion on tests/particles_diffusion_ref.py, seed %d, %d steps of "
                                        "MonitorTimestep / %d; written by tests/test_particles_diffusion_known_answer.py with "
                                        "FCPT_UPDATE_GOLDEN=1" % (dcases.KA_SEED, dcases.KA_INTERVALS * dcases.KA_SUBSTEPS,
                                                                  dcases.KA_SUBSTEPS)), f, indent=1, sort_keys=True)
            f.write("\n")
    gold = golden()
    assert out["live"] == gold["live"] and out["fullest_bin"] == gold["fullest_bin"]
    for k in ("criterion", "mean", "std"):
        assert abs(out[k] - gold[k]) <= 1e-9 * abs(gold[k]), k
