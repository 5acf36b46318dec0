"""fcpt_particles_slab_window, which needs no GPU: for 1, 2 and 3 slabs and the three radial spacings the ownership windows
tile the real line, shared edges carry the same bits and are Rinf of local row FCPT_OVERLAP / nr - FCPT_OVERLAP, and the
ends are infinite.  And the draws of tests/particles_slab_cases.py hold what they are for: on the numpy restatement
(tests/particles_ref.py, tests/particles_explicit_ref.py; the gas of t = 0) every planted crosser changes the side of its
edge within the run, the ones that turn back do so twice, and the particle on an edge starts on it."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, setups

import tests.particles_cases as cases
import tests.particles_ref as R
import tests.particles_explicit_cases as xc
import tests.particles_explicit_ref as X
import tests.particles_slab_cases as sc


@pytest.mark.parametrize("spacing", [B.SPACING_LOGARITHMIC, B.SPACING_ARITHMETIC, B.SPACING_EXPONENTIAL])
@pytest.mark.parametrize("nslabs", [1, 2, 3])
def test_windows_tile_the_real_line(product, spacing, nslabs):
    d = cases.parity_desc(product, 48, 256, spacing=spacing)
    d.exponential_cell_size_factor = 2.0      # (the default has no root on this grid, see test_gpu_particles_parity.py)
    radii = product.radii(d)
    assert np.all(np.isfinite(radii))
    win = sc.slab_windows(product, d, radii, nslabs)
    assert win[0][0] == -np.inf and win[-1][1] == np.inf
    for rank, dk in enumerate(sc.slab_descs(d, nslabs)):
        s = product.split_domain(dk)
        lo, hi = win[rank]
        assert lo < hi
        if rank > 0:
            assert lo == radii[s.imin + B.OVERLAP]
            assert np.float64(lo).tobytes() == np.float64(win[rank - 1][1]).tobytes()
        if rank < nslabs - 1:
            assert hi == radii[s.imin + s.nr - B.OVERLAP]
    # every radius has exactly one owner under the rule of fcpt_particles_set: r_lo^2 <= r^2 < r_hi^2
    probe = np.concatenate([np.linspace(0.5 * d.rmin, 1.5 * d.rmax, 999), [w[1] for w in win[:-1]]])
    owners = sum(((np.square(lo) <= probe * probe) | (lo == -np.inf)) & (probe * probe < np.square(hi)) for lo, hi in win)
    assert np.all(owners == 1)


def test_window_refuses_a_bad_split(product):
    d = cases.parity_desc(product, 48, 256)
    radii = product.radii(d)
    d.rank, d.nranks = 5, 3
    with pytest.raises(B.FcptError):
        product.particles_slab_window(d, radii)


def _initial_gas(product, d, radii):
    g = R.Grid(radii, d.nr_global, d.nphi)
    sigma, vrad, vazi, _ = product.initial_fields(d.copy(), radii)
    return g, cases.isothermal_gas(d, g, sigma, vrad, vazi)


def _check(plants, slots, history, steps):
    history = np.asarray(history)          # [steps + 1, planted]
    for col, k in enumerate(slots):
        edge, sign, kind = plants[int(k)]
        n = sc.crossings(history[:, col], edge)
        if kind == "on":
            assert history[0, col] == edge
        elif kind == "back":
            assert n >= 2, (k, kind, sign, n)
        else:
            assert n >= 1, (k, kind, sign, n)
            first = (history[:, col] >= edge) != (history[0, col] >= edge)
            assert first[1:steps].any(), "the crosser should cross before the last step"


def test_planted_crossers_cross_midpoint(product):
    d = cases.parity_desc(product, 48, 256)
    radii = product.radii(d)
    g, gas = _initial_gas(product, d, radii)
    prm = cases.parity_params(product, d, False)
    phys = R.physics(d, prm)
    bodies = setups.jupiter_bodies(d)
    s, plants = sc.slab_draw(product, d, radii)
    assert len(sc.interior_edges(product, d, radii)) == 3
    kinds = [p[2] for p in plants.values()]
    assert set(kinds) == {"bulk", "twin", "first", "last", "back", "on"}
    assert kinds.count("on") == 3 and kinds.count("back") == 6 and kinds.count("twin") >= 6 and kinds.count("first") == 4
    s["stokes"] = R.initial_stokes(g, gas, phys, s)
    p, slots = sc.subset(s, plants)
    history = [p["r"].copy()]
    for _ in range(cases.PARITY_STEPS):
        guards, _ = R.step(g, gas, phys, bodies, p, cases.PARITY_DT, cases.PARITY_INDIRECT, d.omega_frame * cases.PARITY_DT)
        assert not guards.any() and p["alive"].all()
        history.append(p["r"].copy())
    _check(plants, slots, history, cases.PARITY_STEPS)
    # a step is a small part of a ring width: nobody outruns the overlap
    assert np.abs(np.diff(np.asarray(history), axis=0)).max() < 0.05 * np.diff(g.rinf).min()


@pytest.mark.parametrize("cartesian", [False, True])
def test_planted_crossers_cross_explicit(product, cartesian):
    d = cases.parity_desc(product, 48, 256)
    radii = product.radii(d)
    g, gas = _initial_gas(product, d, radii)
    prm = cases.parity_params(product, d, False)
    phys = X.physics(d, prm)
    bodies = setups.jupiter_bodies(d)
    s, plants = sc.explicit_slab_state(product, d, radii, g, gas, phys, cartesian)
    p, slots = sc.subset(s, plants)
    X.init_timestep(phys, bodies, p, cartesian)
    radius = lambda q: np.hypot(q["r"], q["phi"]) if cartesian else q["r"].copy()
    history = [radius(p)]
    for _ in range(xc.EXPLICIT_CALLS):
        guards = X.step(g, gas, phys, bodies, p, xc.EXPLICIT_DT, cases.PARITY_INDIRECT, d.omega_frame * xc.EXPLICIT_DT,
                        drag=True, cartesian=cartesian)
        assert not guards.any() and p["alive"].all()
        history.append(radius(p))
    if cartesian:       # x = -r, and x^2 + y^2 = r^2 to the bit for the particle on an edge
        for col, k in enumerate(slots):
            if plants[int(k)][2] == "on":
                edge = plants[int(k)][0]
                assert s["r"][k] == -edge and s["r"][k] * s["r"][k] + s["phi"][k] * s["phi"][k] == edge * edge
    _check(plants, slots, history, xc.EXPLICIT_CALLS)
