"""Inputs shared by the dust-particle tests: the reference's dust_drift setup and the draw of the parity test."""
from __future__ import annotations

import numpy as np

from fargocpt_amd import binding as B, setups

import tests.particles_ref as R

CM = 1.0 / 1.495978707e13   # code length per centimetre (L0 = 1 au)


def isothermal_gas(d: B.Desc, grid: R.Grid, sigma, vrad, vazi):
    """H and T of the locally isothermal disk from their definitions (SourceEuler.cpp:1080-1088,1224-1245,1475-1505):
    c_s = h r^f sqrt(G M / r), H = c_s / Omega_K, T = mu / R c_s^2, constant along a ring."""
    rm = grid.rmed
    cs = d.aspect_ratio * rm ** d.flaring_index * np.sqrt(d.G * d.hydro_center_mass / rm)
    H = cs / np.sqrt(d.G * d.hydro_center_mass / rm ** 3)
    T = d.mu / d.Rgas * cs * cs
    ones = np.ones((grid.nr, grid.nphi))
    return R.gas_fields(sigma, H[:, None] * ones, T[:, None] * ones, vrad, vazi, d.density_factor)


# ---- test/dust_drift/dust_drift.yml -----------------------------------------------------------------------------

DRIFT_ORBITS = 100
DRIFT_SAMPLE = 0.628318531      # MonitorTimestep: a tenth of an orbit at 1 au
# the reference steps with the gas CFL limit, 0.5 dr / c_s = 0.045 at 1 au on this grid and less further in;
# a sixteenth of the sampling interval (0.039) is of that size and keeps the samples on step boundaries
DRIFT_SUBSTEPS = 16
DRIFT_DT = DRIFT_SAMPLE / DRIFT_SUBSTEPS
DRIFT_TOLERANCE = 0.01          # calc_deviation.py
# test/dust_drift/deviations.txt of the reference: (Stokes number, deviation)
DRIFT_REFERENCE_DEVIATIONS = [
    (4.683726604682566534e-08, -7.348145725160071251e-04), (4.683720962574184852e-07, -7.377129417704963998e-04),
    (4.683664544513871032e-06, -7.371790203062333902e-04), (4.683100668051964189e-05, -7.304395257574647360e-04),
    (4.677491665688776655e-04, -4.033583456609646234e-04), (4.621202310717473921e-03, -8.352614235371813578e-04),
    (4.080741561634874254e-02, -1.504087451596136660e-03), (2.957282737789268534e-01, -7.987193068873854607e-03),
    (7.061075539002357182e+00, -4.622702992709393222e-03), (2.688071256153982063e+02, -7.147527820816623745e-05),
    (1.366233324943743901e+04, -9.926063461251910525e-05), (4.533387882471327321e+05, 1.174770404370750754e-04)]


def drift_desc(lib: B.Library) -> B.Desc:
    d = lib.desc_default()
    d.nr_global, d.nphi = 400, 1403
    d.rmin, d.rmax, d.radial_spacing = 0.5, 3.0, B.SPACING_LOGARITHMIC
    d.sigma0, d.sigma_slope, d.sigma_floor = 88.87231453905 / setups.SIGMA_CGS, 1.0, 1e-7
    d.aspect_ratio, d.flaring_index = 0.05, 0.0
    d.viscous_alpha, d.constant_viscosity = 0.0, 0.0
    d.eos, d.adiabatic_index, d.mu = B.EOS_ISOTHERMAL, 1.4, 2.35
    d.thickness_smoothing = 0.0
    d.omega_frame = 0.0
    d.damping = 0
    d.first_dt = 1e-1
    d.artificial_viscosity = B.ARTVISC_NONE
    return d


def drift_case(lib: B.Library):
    """-> (desc, radii, gas grids (sigma, vrad, vazi, energy), params, bodies, initial state without Stokes numbers)."""
    d = drift_desc(lib)
    radii = lib.radii(d)
    fields = lib.initial_fields(d, radii)
    prm = lib.particle_params_default(d)
    prm.gravity_cartesian = 1         # CartesianParticles: yes with the midpoint integrator (parameters.cpp:927-932)
    prm.escape_radius_min, prm.escape_radius_max = 0.5, 3.0
    n = 12
    radius = 1e-8 * 100.0 * CM * 10.0 ** np.arange(n)        # ParticleRadius: 1e-8 m, factor 10, 12 species
    mass = 4.0 / 3.0 * np.pi * radius ** 3 * prm.particle_density
    a = 1.0
    v = np.sqrt(d.G * (d.hydro_center_mass + mass) / a)      # insert_particle (:426-475), e = 0
    phi = (np.arange(n) + 0.37) * (2.0 * np.pi / n)          # the reference draws the angle; spread over the ring here
    state = R.make_state(np.arange(n), np.full(n, a), phi, np.zeros(n), v / a, radius, np.zeros(n))
    bodies = ([0.0], [0.0], [d.hydro_center_mass])
    return d, radii, fields, prm, bodies, state


def drift_deviations(t, r, stokes, alive, h=0.05):
    """calc_deviation.py per particle: the mean over the last tenth of its time series of (dr/dt) / v_theo, minus 1, with
    v_theo = eta v_K / (St + 1/St) and eta = -2 h^2 (drift_theo.py: Sigma and T slopes 1; G M = 1).  A particle that leaves
    the domain has a series that ends there, as in the reference's output (its St = 0.3 grain does, after 40 orbits).
    t: [m]; r, stokes, alive: [m, n].  -> (mean Stokes numbers, deviations)."""
    st_avg, dev = np.zeros(r.shape[1]), np.zeros(r.shape[1])
    for k in range(r.shape[1]):
        m = int(alive[:, k].sum())            # alive is monotonic: the first m samples
        rk, sk, tk = r[:m, k], stokes[:m, k], t[:m]
        rdot = (rk[1:] - rk[:-1]) / (tk[1:] - tk[:-1])
        vtheo = -2.0 * h * h * np.sqrt(1.0 / rk) / (sk + 1.0 / sk)
        navg = rdot.size // 10
        dev[k] = np.mean(rdot[-navg:] / vtheo[-navg:]) - 1.0
        st_avg[k] = np.mean(sk[-navg:])
    return st_avg, dev


# ---- the draw of the parity test ----------------------------------------------------------------------------------

PARITY_DT = 4.0e-3      # below the CFL step of every parity grid after its 8 gas steps
PARITY_STEPS = 20
PARITY_INDIRECT = (3.0e-4, -2.0e-4)


def parity_desc(lib: B.Library, nr=48, nphi=256, adiabatic=False, spacing=B.SPACING_LOGARITHMIC, smoothing=0.6, omega_frame=1.0):
    d = setups.planet_disk(lib, nr, nphi, adiabatic=adiabatic)
    d.radial_spacing = spacing
    d.thickness_smoothing = smoothing
    d.omega_frame = omega_frame
    return d


def parity_params(lib: B.Library, d: B.Desc, cartesian: bool):
    prm = lib.particle_params_default(d)
    prm.gravity_cartesian = 1 if cartesian else 0
    return prm


def census_draw(d: B.Desc, radii, n=1000, seed=20240611, dt=PARITY_DT):
    """n particles for the grid of `d`: a bulk on perturbed Kepler orbits with grain radii from 1e-5 cm to 100 m
    (every branch of the drag law, both Knudsen regimes), boulders on eccentric orbits (large Reynolds numbers), particles
    in the first and last half column of the ring, slow leavers next to both escape radii, and fast particles that enter
    the domain through the outermost half cells, where the cell-centred grids are extrapolated."""
    rng = np.random.default_rng(seed)
    nr, nphi = d.nr_global, d.nphi
    g = R.Grid(radii, nr, nphi)
    vk = lambda r: np.sqrt(d.G * d.hydro_center_mass / r)
    r = np.exp(rng.uniform(np.log(d.rmin * 1.06), np.log(d.rmax * 0.95), n))
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    radius = CM * 10.0 ** rng.uniform(-5.0, 4.0, n)
    r_dot = vk(r) * rng.normal(0.0, 0.01, n)
    # (phi_dot is the angular velocity in the inertial frame: the gas speed it is compared with gets r OmegaFrame added)
    v_phi = vk(r) * (1.0 + rng.normal(0.0, 0.01, n))
    k = np.arange(n)
    if n >= 200:
        # boulders, metres to 100 m across, a fifth of the Kepler speed off the gas
        m = (k % 10) == 3
        radius[m] = CM * 10.0 ** rng.uniform(2.0, 4.0, m.sum())
        r_dot[m] = vk(r[m]) * rng.uniform(0.1, 0.3, m.sum()) * rng.choice([-1.0, 1.0], m.sum())
        # pebbles in the Reynolds range 500 .. 1500 and above it
        m = (k % 10) == 7
        radius[m] = CM * 10.0 ** rng.uniform(0.5, 2.0, m.sum())
        r_dot[m] = vk(r[m]) * rng.uniform(0.02, 0.3, m.sum())
        # the seam of the ring
        phi[k % 50 == 1] = rng.uniform(0.02, 0.45, (k % 50 == 1).sum()) * g.dphi
        phi[k % 50 == 2] = 2.0 * np.pi - rng.uniform(0.02, 0.45, (k % 50 == 2).sum()) * g.dphi
        # nobody starts next to the planet at (1, 0): a close encounter amplifies rounding differences beyond what a
        # parity bar can tell from an error (test_particles_ref_census.py measures the amplification)
        near = (np.abs(r - 1.0) < 0.12) & (np.abs(np.mod(phi + np.pi, 2.0 * np.pi) - np.pi) < 0.15)
        r[near] *= 1.25
        v_phi[near] = vk(r[near])
        # leavers: a few step lengths inside an escape radius, moving out at a tenth of the Kepler speed
        for sel, edge, sign in ((k % 100 == 11, d.rmin, -1.0), (k % 100 == 12, d.rmax, 1.0)):
            c = sel.sum()
            v = 0.1 * vk(edge)
            r[sel] = edge - sign * v * dt * rng.uniform(0.5, PARITY_STEPS - 1.0, c)
            r_dot[sel] = sign * v
            radius[sel] = CM * 10.0 ** rng.uniform(1.0, 3.0, c)
            v_phi[sel] = vk(r[sel])
        # enterers: from outside the grid through its outermost half cell in one step (the half drift ends below
        # Rmed[0] / above Rmed[nr-1], the full step inside the escape radii), heavy enough to keep their speed
        for sel, lo, hi, sign in ((k % 100 == 13, g.rinf[0], g.rinf[1], 1.0), (k % 100 == 14, g.rinf[nr], g.rinf[nr - 1], -1.0)):
            c = sel.sum()
            w = abs(hi - lo)
            a = rng.uniform(0.1, 0.3, c)            # start this many cell widths outside the grid
            s = 1.0 + 1.5 * a                       # cell widths per step: -a + s/2 < 1/2 and 1 < -a + s
            r[sel] = lo - sign * a * w
            r_dot[sel] = sign * s * w / dt
            radius[sel] = CM * 10.0 ** rng.uniform(3.0, 4.0, c)
            v_phi[sel] = vk(r[sel])
    return R.make_state(k + 1000, r, phi, r_dot, v_phi / r, radius, np.zeros(n))
