"""The draw of the GPU diffusion parity test, held to its purpose with the numpy restatement alone (no GPU): the kicks
of compared particles meet the rows without a density derivative, the seam column, both signs of the drift term and
both ends of the Schmidt number, and a kick decides an escape."""
import numpy as np
import pytest

import fargocpt_amd
from fargocpt_amd import setups

import tests.particles_cases as cases
import tests.particles_diffusion_cases as dcases
import tests.particles_diffusion_ref as D
import tests.particles_ref as R


@pytest.fixture(scope="module")
def census():
    lib = fargocpt_amd.load()
    d = cases.parity_desc(lib)
    d.viscous_alpha = dcases.PARITY_ALPHA
    radii = lib.radii(d)
    g = R.Grid(radii, d.nr_global, d.nphi)
    sigma, vrad, vazi, _ = lib.initial_fields(d.copy(), radii)
    sigma = sigma * dcases.ring_bump(g)[:, None]
    gas = dcases.with_sound_speed(d, cases.isothermal_gas(d, g, sigma, vrad, vazi))
    prm = R.physics(d, cases.parity_params(lib, d, cartesian=False))
    bodies = setups.jupiter_bodies(d)
    s0 = dcases.diffusion_draw(d, radii)
    s0["stokes"] = R.initial_stokes(g, gas, prm, s0)

    def run(s, gas_drag=True):
        s = R.copy_state(s)
        keys = ("row", "column", "mean", "stokes", "sigma")
        seen = {k: [] for k in keys}
        seen.update(guards=0, left_by_kick=0, kept_by_kick=0)
        for k in range(cases.PARITY_STEPS):
            guards, diag = D.step(g, gas, prm, bodies, s, cases.PARITY_DT, cases.PARITY_INDIRECT, d.omega_frame * cases.PARITY_DT,
                                  gas_drag=gas_drag, diffusion=True, seed=dcases.PARITY_SEED, step_no=dcases.PARITY_FIRST_STEP + k)
            seen["guards"] += int((guards != 0).sum())
            seen["left_by_kick"] += int((diag["gone"] & ~diag["gone_before_kick"]).sum())
            seen["kept_by_kick"] += int((~diag["gone"] & diag["gone_before_kick"]).sum())
            kept = ~diag["gone"]            # compared by the parity test after this step
            for q in keys:
                seen[q].append(diag[q][kept])
        return s, {k: (np.concatenate(v) if isinstance(v, list) else v) for k, v in seen.items()}

    out = {"d": d, "g": g, "s0": s0, "run": run}
    for name, drag in (("drag", True), ("nodrag", False)):
        out[name] = run(s0, drag)
    return out


def test_ids_are_distinct_and_spread_above_2_to_32(census):
    ids = census["s0"]["id"]
    assert np.unique(ids).size == ids.size
    assert (ids > 2 ** 32).sum() >= ids.size - 1 and int(ids.max()) > 2 ** 42


@pytest.mark.parametrize("name", ["drag", "nodrag"])
def test_the_kicks_meet_every_case(census, name):
    g, (s1, seen) = census["g"], census[name]
    rows = {"row 0": int((seen["row"] == 0).sum()), "row Nr-1": int((seen["row"] == g.nr - 1).sum()),
            "interior": int(((seen["row"] > 0) & (seen["row"] < g.nr - 1)).sum()),
            "first column": int((seen["column"] == 0).sum()), "last column": int((seen["column"] == g.nphi - 1).sum()),
            "mean > 0": int((seen["mean"] > 0).sum()), "mean < 0": int((seen["mean"] < 0).sum()),
            "St < 0.1": int((seen["stokes"] < 0.1).sum()), "St > 10": int((seen["stokes"] > 10.0).sum())}
    print(name, rows, "left only because of the kick:", seen["left_by_kick"], "kept by it:", seen["kept_by_kick"], "live:", int(s1["alive"].sum()))
    assert min(rows.values()) >= 1, rows
    assert (seen["mean"][(seen["row"] == 0) | (seen["row"] == g.nr - 1)] == 0.0).all()
    assert (seen["sigma"] > 0).all()
    assert seen["left_by_kick"] >= 1 and seen["kept_by_kick"] >= 1
    assert seen["guards"] == 0


@pytest.mark.parametrize("name,drag", [("drag", True), ("nodrag", False)])
def test_the_run_is_not_sensitive_to_rounding(census, name, drag):
    """A perturbation of 1e-15 relative in the state stays below 1e-12 by the parity measure after the 20 steps (the
    kick reads its cell without interpolation: a particle would have to lie within rounding of a cell's edge)."""
    s0 = census["s0"]
    rng = np.random.default_rng(7)
    p = R.copy_state(s0)
    for k in ("r", "phi", "r_dot", "phi_dot", "stokes"):
        p[k] = p[k] * (1.0 + 1e-15 * rng.choice([-1.0, 1.0], p[k].size))
    a, _ = census["run"](p, drag)
    worst = R.worst_difference(R.live(a), R.live(census[name][0]))
    print(worst)
    assert max(worst.values()) < 1e-12, worst
