"""The draw of the GPU parity test, held to its purpose with the numpy restatement alone (no GPU): every branch of the
drag law and every special case of the interpolation is met by particles that the parity test then compares."""
import numpy as np
import pytest

import fargocpt_amd
from fargocpt_amd import setups

import tests.particles_cases as cases
import tests.particles_ref as R


@pytest.fixture(scope="module")
def census():
    lib = fargocpt_amd.load()
    d = cases.parity_desc(lib)
    radii = lib.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    sigma, vrad, vazi, _ = lib.initial_fields(d.copy(), radii)
    gas = cases.isothermal_gas(d, g, sigma, vrad, vazi)
    prm = R.physics(d, cases.parity_params(lib, d, cartesian=False))
    bodies = setups.jupiter_bodies(d)
    s0 = cases.census_draw(d, radii)
    s0["stokes"] = R.initial_stokes(g, gas, prm, s0)

    def run(s):
        s = R.copy_state(s)
        seen = {"re": [], "kn": [], "r_in": [], "phi": [], "slots": [], "guards": 0}
        for _ in range(cases.PARITY_STEPS):
            slots = np.flatnonzero(s["alive"])
            guards, diag = R.step(g, gas, prm, bodies, s, cases.PARITY_DT, cases.PARITY_INDIRECT, d.omega_frame * cases.PARITY_DT)
            still = s["alive"][slots]          # compared by the parity test after this step
            seen["guards"] += int((guards != 0).sum())
            seen["re"].append(diag["Re"][still]); seen["kn"].append(diag["Kn"][still])
            seen["r_in"].append(diag["r_in"][still]); seen["phi"].append(diag["phi"][still])
        return s, {k: (np.concatenate(v) if isinstance(v, list) and v else v) for k, v in seen.items()}

    s1, seen = run(s0)
    return dict(d=d, g=g, s0=s0, s1=s1, seen=seen, run=run)


def test_every_reynolds_branch_is_taken(census):
    re, n = census["seen"]["re"], census["seen"]["re"].size
    shares = [np.mean(re <= 1e-3), np.mean((re > 1e-3) & (re <= 500.0)), np.mean((re > 500.0) & (re <= 1500.0)), np.mean(re > 1500.0)]
    print("shares of the four Re branches:", shares, "of", n)
    assert min(shares) >= 0.01, shares


def test_both_knudsen_regimes_occur(census):
    kn = census["seen"]["kn"]
    assert (kn < 0.1).any() and (kn > 10.0).any()


def test_edges_of_the_interpolation_are_met(census):
    g, seen = census["g"], census["seen"]
    r, phi = seen["r_in"], seen["phi"]
    counts = {"first half cell": int((r < g.rmed[0]).sum()), "last half cell": int((r > g.rmed[-1]).sum()),
              "first half column": int(((phi < 0.5 * g.dphi) & (phi < np.pi)).sum()),
              "last half column": int(((phi > 2.0 * np.pi - 0.5 * g.dphi) & (phi > np.pi)).sum())}
    print(counts)
    assert min(counts.values()) >= 1, counts


def test_escapes_and_survivors(census):
    d, s0, s1 = census["d"], census["s0"], census["s1"]
    gone = ~s1["alive"]
    inner, outer = int((gone & (s1["r"] < 1.0)).sum()), int((gone & (s1["r"] > 1.0)).sum())
    print("left through the inner / outer escape radius:", inner, outer, "survivors:", int(s1["alive"].sum()))
    assert inner >= 5 and outer >= 5
    assert s1["alive"].mean() >= 0.8
    assert census["seen"]["guards"] == 0


def test_the_run_is_not_sensitive_to_rounding(census):
    """A perturbation of 1e-15 relative in the state must stay below 1e-12 by the parity measure: what the GPU may differ
    by at the start of the run is not amplified beyond the parity bar's reach."""
    s0 = census["s0"]
    rng = np.random.default_rng(7)
    p = R.copy_state(s0)
    for k in ("r", "phi", "r_dot", "phi_dot", "stokes"):
        p[k] = p[k] * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], p[k].size))
    a, _ = census["run"](p)
    worst = R.worst_difference(R.live(a), R.live(census["s1"]))
    print(worst)
    assert max(worst.values()) < 1e-12, worst
