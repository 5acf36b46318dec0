"""The disk's force on all bodies in one pass (fcpt_disk_on_bodies_begin / _end, k_disk_on_bodies) and its sum over
the slabs (fcpt_allreduce_sum): against the oracle's ComputeDiskOnPlanetAccel, against the product's own single-body
call (bit for bit: the batched kernel keeps that kernel's reduction tree), in the point-mass limit, and over slabs."""
import threading

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups

pytestmark = pytest.mark.gpu


def _placements(bodies):
    """The 27 bodies of test_gpu_parity.test_disk_on_body_accel: (x, y, r_object, smoothing_fixed, cubic radius)."""
    hill = (bodies[2][1] / 3.0) ** (1.0 / 3.0)
    p = [(1.0, 0.0, 1.0, -1.0, 0.0),                      # H-based smoothing per cell
         (1.0, 0.0, 1.0, 0.6 * 0.05, 0.5 * hill),        # planet-location + cubic smoothing
         (0.0, 0.0, 0.0, 0.0, 0.0)]                      # the star, no smoothing
    rng = np.random.default_rng(11)   # bodies anywhere: inside the inner hole, between rings, beyond the disk
    for _ in range(24):
        r, ph = rng.uniform(0.05, 3.5), rng.uniform(0.0, 2 * np.pi)
        fixed = float(rng.choice([-1.0, 0.0, 0.03]))
        p.append((r * np.cos(ph), r * np.sin(ph), r, fixed, float(rng.choice([0.0, 0.4 * hill]))))
    return p


def _batches(n_total, size):
    """Windows of `size` consecutive placements covering all of them (the last one wraps round)."""
    return [[(k + i) % n_total for i in range(size)] for k in range(0, n_total, size)]


def _scale(sig):
    return float(np.abs(sig).sum()) * 2 * np.pi * 2.5 ** 2 / sig.size  # ~ G M_disk with G = 1, d ~ 1


@pytest.mark.parametrize("adiabatic", [False, True])
def test_batched_force_matches_oracle_and_single_body_call(product, oracle, adiabatic):
    """Configuration and bar of test_disk_on_body_accel (planet_disk 48x256, 8 steps, 1e-10 max|oracle| + 1e-12 scale);
    the 27 placements go through the batched call in batches of 1, 2, 5 and 8 whose members mix the smoothing modes.
    Against the product's single-body call the comparison is bit for bit: k_disk_on_bodies keeps its thread-to-cell
    map, ring order, shuffle tree, block fold and final stage.  Two identical calls: bit-identical."""
    d = setups.planet_disk(product, 48, 256, adiabatic=adiabatic)
    bodies = setups.jupiter_bodies(d)
    place = _placements(bodies)
    modes = {(p[3] < 0, p[3] == 0, p[4] > 0) for p in place}
    assert len(modes) >= 5  # cell-wise, zero and fixed smoothing, with and without the cubic term

    ctx = driver.make_context(oracle, d, bodies=bodies)
    S = driver.SlabSet([ctx])
    S.prepare()
    S.run(8)
    want = np.array([ctx.disk_on_body_accel(*p) for p in place])
    ctx.close()

    ctx = driver.make_context(product, d, bodies=bodies)
    S = driver.SlabSet([ctx])
    S.prepare()
    S.run(8)
    single = np.array([ctx.disk_on_body_accel(*p) for p in place])
    scale = _scale(ctx.download(B.F_SIGMA))
    worst = 0.0
    for size in (1, 2, 5, 8):
        for idx in _batches(len(place), size):
            args = [np.array([place[k][c] for k in idx]) for c in range(5)]
            got = ctx.disk_on_bodies(*args)
            assert got.shape == (size, 4)
            again = ctx.disk_on_bodies(*args)
            assert np.array_equal(got, again), "two identical calls differ"
            for row, k in zip(got, idx):
                assert np.abs(want[k]).max() > 0
                bar = 1e-10 * np.abs(want[k]).max() + 1e-12 * scale
                worst = max(worst, float(np.abs(row - want[k]).max() / bar))
                assert np.all(np.abs(row - want[k]) <= bar), (size, k, row, want[k])
                assert np.array_equal(row, single[k]), (size, k, row, single[k])
    print(f"batched force vs oracle: worst difference {worst:.3e} of the bar")
    ctx.close()


def test_batched_force_argument_errors(product):
    d = setups.planet_disk(product, 48, 256)
    ctx = driver.make_context(product, d)
    with pytest.raises(B.FcptError):
        ctx.disk_on_bodies_end()                       # no pass pending
    z = np.zeros(B.MAX_BODIES + 1)
    with pytest.raises(B.FcptError):
        ctx.disk_on_bodies_begin(z, z, z, z, z)        # more than FCPT_MAX_BODIES
    e = np.zeros(0)
    with pytest.raises(B.FcptError):
        ctx.disk_on_bodies_begin(e, e, e, e, e)
    one = np.ones(1)
    ctx.disk_on_bodies_begin(one, 0 * one, one, -one, 0 * one)
    assert ctx.disk_on_bodies_end().shape == (1, 4)
    with pytest.raises(B.FcptError):
        ctx.disk_on_bodies_end()                       # consumed
    ctx.close()


def test_point_mass_limit(product):
    """The idea of the reference's planet_orbiting_disk test at kernel level: a uniform ring between 1e-7 and 2e-7
    (28 x 56 cells, the grid of its euler.yml) of total mass M pulls a body at distance d = 1 with G M / d^2 towards
    the origin.  The first correction is the quadrupole's, of order (r / d)^2 = 4e-14: bar 1e-12 relative, and the
    transverse component below 1e-12 of the radial one."""
    d = setups.planet_disk(product, 28, 56, damping=False)
    d.rmin, d.rmax, d.radial_spacing = 1e-7, 2e-7, B.SPACING_LOGARITHMIC
    ctx = driver.make_context(product, d)
    radii = product.radii(d)
    s = ctx.split
    lo, hi = s.radial_first_active, s.radial_active_size
    area = np.pi * (radii[hi] ** 2 - radii[lo] ** 2)      # the rings the force sums over
    M = 1.0
    ctx.upload(B.F_SIGMA, np.full((ctx.nr, ctx.nphi), M / area))
    for ang in (0.0, 0.7, 2.9):
        x, y = np.cos(ang), np.sin(ang)
        a = ctx.disk_on_bodies([x], [y], [1.0], [0.0], [0.0])[0]
        assert a[2] == 0.0 and a[3] == 0.0                # every ring is inside the body's orbit
        radial = a[0] * x + a[1] * y
        transverse = -a[0] * y + a[1] * x
        want = -d.G * M / 1.0 ** 2
        print(f"point-mass limit at {ang}: radial {radial / want - 1.0:.3e} relative, transverse {abs(transverse / want):.3e}")
        assert abs(radial / want - 1.0) <= 1e-12
        assert abs(transverse) <= 1e-12 * abs(want)
    ctx.close()


def _in_threads(fns):
    out, err = [None] * len(fns), []

    def run(k):
        try:
            out[k] = fns[k]()
        except Exception as e:  # noqa: BLE001 -- reported below
            err.append((k, e))

    ts = [threading.Thread(target=run, args=(k,)) for k in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(180)
    assert not err, err
    assert not any(t.is_alive() for t in ts)
    return out


@pytest.mark.parametrize("adiabatic", [False, True])
def test_sum_over_slabs(product, oracle, adiabatic, tmp_path):
    """One slab against three slabs of the same global state (host link): the rank-ordered sum of the slabs' sums
    meets the one-slab sums at the oracle bar of the test above and carries the same bits on all three ranks."""
    nslabs = 3
    d = setups.planet_disk(product, 96, 256, adiabatic=adiabatic)
    bodies = setups.jupiter_bodies(d)
    place = _placements(bodies)[:8]
    args = [np.array([p[c] for p in place]) for c in range(5)]

    one = driver.make_context(product, d, bodies=bodies)
    S = driver.SlabSet([one])
    S.prepare()
    S.run(8)
    want = one.disk_on_bodies(*args)
    assert np.array_equal(one.allreduce_sum(want), want)   # no communicator: the input
    scale = _scale(one.download(B.F_SIGMA))
    one.close()

    ctxs = []
    for k in range(nslabs):
        dk = d.copy()
        dk.rank, dk.nranks = k, nslabs
        ctxs.append(driver.make_context(product, dk, bodies=bodies))
    S = driver.SlabSet(ctxs)
    S.prepare()
    S.run(8)
    link = str(tmp_path / "hostlink")
    _in_threads([lambda c=c: c.comm_init_host(link) for c in ctxs])
    local = [c.disk_on_bodies(*args) for c in ctxs]
    total = _in_threads([lambda c=c, v=v: c.allreduce_sum(v) for c, v in zip(ctxs, local)])
    rank_order = (local[0] + local[1]) + local[2]
    for t in total:
        assert np.array_equal(t, total[0])
        assert np.array_equal(t, rank_order)
    for row, ref in zip(total[0], want):
        assert np.all(np.abs(row - ref) <= 1e-10 * np.abs(ref).max() + 1e-12 * scale), (row, ref)
    _in_threads([lambda c=c: c.comm_barrier() for c in ctxs])
    for c in reversed(ctxs):
        c.comm_destroy()
        c.close()


# ---- the driver: fargocpt_hip --bodies free ----------------------------------------------------------------------------
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fargocpt_amd", "bin", "fargocpt_hip")
SETUPS = os.path.join(ROOT, "tests", "golden", "setups")


def _drive(tmp_path, setup, outname, extra=(), edits=None, ranks=1, mode=("start",)):
    out = tmp_path / outname
    text = open(os.path.join(SETUPS, setup)).read().splitlines()
    text = [("OutputDir: " + str(out)) if l.startswith("OutputDir") else l for l in text]
    for key, val in (edits or {}).items():
        assert any(l.split(":")[0].strip() == key for l in text), key
        text = [(f"{key}: {val}") if l.split(":")[0].strip() == key else l for l in text]
    cfg = tmp_path / f"config_{outname}_{mode[0]}.yml"
    cfg.write_text("\n".join(text) + "\n")
    cmd = [BIN, "-q"] + (["--ranks", str(ranks)] if ranks > 1 else []) + list(extra) + list(mode) + [str(cfg)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    return str(out) + "/"


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# max relative difference of the gas fields of the last snapshot between --bodies free and --bodies circular for
# cold_disk_planet.yml, as measured (profiles/free_bodies_cold_disk_planet.txt)
COLD_DISK_PLANET_FREE_VS_CIRCULAR = {"Sigma": 1.4e-11, "vrad": 3.1e-10, "vazi": 5.7e-13}


def test_driver_free_bodies_without_feedback(tmp_path):
    """cold_disk_planet.yml (planet of 2e-5 on a circular orbit, DiskFeedback: no, 100 orbits) with --bodies free
    against --bodies circular.  The planet stays on its circle: monitor/nbody1.dat against a (cos wt, sin wt) within the
    reference's circ_kepler_orbit criterion carried from 20 to 100 orbits (5e-11); measured 1.5e-11.  The gas fields of
    the last snapshot differ by the integrator's error and by how the indirect term is averaged over a step (a
    velocity difference of the star over the step against the closed-form average): measured max relative
    differences Sigma 1.4e-11, vrad 3.0e-10, vazi 5.7e-13 (of max|field|), asserted with a margin of 10.  The setup's
    known-answer threshold (temperature profile within 0.1, calc_deviation.py) holds in free mode too."""
    circ = _drive(tmp_path, "cold_disk_planet.yml", "circ")
    free = _drive(tmp_path, "cold_disk_planet.yml", "free", extra=("--bodies", "free"))
    Nr, Naz = np.genfromtxt(free + "dimensions.dat", usecols=(4, 5), unpack=True, dtype=int)
    t, x, y, vx, vy, m = np.genfromtxt(free + "monitor/nbody1.dat", usecols=(7, 2, 3, 4, 5, 6), unpack=True)
    assert t.size == 1001 and t[0] == 0.0 and np.all(m == 2e-5)
    om = np.sqrt(1.0 + 2e-5)
    circle = max(np.abs(x - np.cos(om * t)).max(), np.abs(y - np.sin(om * t)).max())
    print(f"free planet against its circle over {t[-1] / (2 * np.pi):.1f} orbits: {circle:.3e}")
    assert circle <= 1e-11 * 100 / 20
    star = np.genfromtxt(free + "monitor/nbody0.dat", usecols=(2, 3, 4, 5))
    assert np.all(star == 0.0)                                    # HydroFrameCenter: primary
    for name, rows in (("Sigma", Nr), ("vrad", Nr + 1), ("vazi", Nr)):
        a = np.fromfile(free + f"snapshots/10/{name}.dat")
        b = np.fromfile(circ + f"snapshots/10/{name}.dat")
        assert a.size == b.size == rows * Naz
        print(f"free vs circular, snapshot 10, {name}: {_rel(a, b):.3e}")
        assert _rel(a, b) <= 10 * COLD_DISK_PLANET_FREE_VS_CIRCULAR[name], (name, _rel(a, b))
    import yaml
    tempunit = yaml.safe_load(open(free + "units.yml"))["temperature"]["cgs value"]
    prof = {n: (tempunit * np.fromfile(free + f"snapshots/{n}/Temperature.dat").reshape(Nr, Naz)).mean(axis=1) for n in (0, 10)}
    assert np.max(np.abs(prof[10] / prof[0] - 1)) < 0.1


@pytest.mark.parametrize("ranks", [3])
def test_driver_free_bodies_with_feedback_over_slabs(tmp_path, ranks):
    """mpi_simple.yml (DiskFeedback: yes) with --bodies free, 1 process against 3 (host transport): the same number of
    steps, snapshot fields to 1e-12 of max|field| (the bar of test_n_rank_driver_matches_one_rank; measured 1.4e-14,
    2.8e-14, 2.5e-15), the rows of nbody1.dat to 1e-12 of the largest entry of their column -- position and velocity as
    vectors: in the frame that rotates with the planet its y is 3e-4 of its x."""
    one = _drive(tmp_path, "mpi_simple.yml", "one", extra=("--bodies", "free"))
    many = _drive(tmp_path, "mpi_simple.yml", "many", extra=("--bodies", "free"), ranks=ranks)
    assert open(many + "snapshots/list.txt").read().split() == ["0", "1"]
    for name, rows in (("Sigma", 128), ("vrad", 129), ("vazi", 128)):
        a, b = np.fromfile(many + f"snapshots/1/{name}.dat"), np.fromfile(one + f"snapshots/1/{name}.dat")
        assert a.size == b.size == rows * 384
        print(f"feedback on, {ranks} ranks vs 1, {name}: {_rel(a, b):.3e}")
        assert _rel(a, b) <= 1e-12, (name, _rel(a, b))
    a, b = np.genfromtxt(many + "monitor/nbody1.dat"), np.genfromtxt(one + "monitor/nbody1.dat")
    assert a.shape == b.shape == (2, 22)
    for c in range(22):
        scale = np.abs(b[:, c]).max()
        if c in (2, 3, 4, 5):
            lo = 2 if c < 4 else 4
            scale = np.hypot(b[:, lo], b[:, lo + 1]).max()
        if scale > 0:
            print(f"feedback on, {ranks} ranks vs 1, nbody1.dat column {c}: {np.abs(a[:, c] - b[:, c]).max() / scale:.3e}")
            assert np.abs(a[:, c] - b[:, c]).max() <= 1e-12 * scale, c
    circ = _drive(tmp_path, "mpi_simple.yml", "circ")
    assert not np.array_equal(np.fromfile(circ + "snapshots/1/Sigma.dat"), np.fromfile(one + "snapshots/1/Sigma.dat"))


def test_driver_feedback_moves_the_planet_and_restarts_bitwise(tmp_path):
    """mpi_simple.yml over 4 monitor steps.  With DiskFeedback: yes the planet's angular momentum about the star (column
    11 of nbody1.dat) changes from row to row by (torque + indirect torque) x MonitorTimestep (columns 18 and 20: the
    step-by-step sums of m r x a of the disk's force on the planet and of minus its force on the star, over
    MonitorTimestep) -- the sum is the exact record of the kicks, so the difference is rounding, asserted at 1e-12 |L|;
    its semi-major axis moves (measured: da/dt = -7.9e-6 per time unit, |dL - sum| = 1.6e-18 at |dL| = 4.9e-9), while with DiskFeedback: no it stays within
    the integrator's error (1e-11; measured 4.4e-15).  A restart from snapshot 1 reproduces the later snapshots and the rows of
    nbody1.dat bit for bit."""
    edits = {"Nsnapshots": "4"}
    yes = _drive(tmp_path, "mpi_simple.yml", "yes", extra=("--bodies", "free"), edits=edits)
    no = _drive(tmp_path, "mpi_simple.yml", "no", extra=("--bodies", "free"), edits={**edits, "DiskFeedback": "no"})
    ry, rn = np.genfromtxt(yes + "monitor/nbody1.dat"), np.genfromtxt(no + "monitor/nbody1.dat")
    assert ry.shape == rn.shape == (5, 22)
    dt_mon = 0.628
    L, tq = ry[:, 11], ry[:, 18] + ry[:, 20]
    worst = np.abs(np.diff(L) - tq[1:] * dt_mon).max()
    print(f"angular momentum: |dL - sum(torque dt)| = {worst:.3e}, |dL| = {np.abs(np.diff(L)).max():.3e}, L = {L[0]:.3e}")
    assert np.abs(np.diff(L)).max() > 1e6 * worst
    assert worst <= 1e-12 * np.abs(L).max()
    dadt = (ry[-1, 12] - ry[0, 12]) / (ry[-1, 7] - ry[0, 7])
    print(f"da/dt with feedback: {dadt:.3e}; without: max |a/a0 - 1| = {np.abs(rn[:, 12] / rn[0, 12] - 1).max():.3e}")
    assert np.abs(rn[:, 12] / rn[0, 12] - 1).max() <= 1e-11
    assert np.abs(ry[-1, 12] / ry[0, 12] - 1) > 1e-9
    assert np.all(rn[:, 18] == 0.0) and np.all(rn[:, 20] == 0.0)

    part = _drive(tmp_path, "mpi_simple.yml", "part", extra=("--bodies", "free"), edits={"Nsnapshots": "1"})
    _drive(tmp_path, "mpi_simple.yml", "part", extra=("--bodies", "free"), edits=edits, mode=("restart", "1"))
    for snap in ("2", "4"):
        for name in ("Sigma", "vrad", "vazi", "nbody"):
            ext = ".bin" if name == "nbody" else ".dat"
            assert np.array_equal(np.fromfile(part + f"snapshots/{snap}/{name}{ext}", dtype=np.uint8),
                                  np.fromfile(yes + f"snapshots/{snap}/{name}{ext}", dtype=np.uint8)), (snap, name)
    assert open(part + "monitor/nbody1.dat").read() == open(yes + "monitor/nbody1.dat").read()
    assert open(part + "monitor/nbody0.dat").read() == open(yes + "monitor/nbody0.dat").read()


def test_driver_circular_says_that_feedback_is_not_applied(tmp_path):
    out = tmp_path / "note"
    text = open(os.path.join(SETUPS, "mpi_simple.yml")).read().splitlines()
    text = [("OutputDir: " + str(out)) if l.startswith("OutputDir") else l for l in text]
    cfg = tmp_path / "config_note.yml"
    cfg.write_text("\n".join(text) + "\n")
    r = subprocess.run([BIN, "-N", "2", "start", str(cfg)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr.count("DiskFeedback: yes is not applied with --bodies circular") == 1
    r = subprocess.run([BIN, "-q", "-N", "2", "start", str(cfg)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "DiskFeedback" not in r.stderr
