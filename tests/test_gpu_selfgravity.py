"""Self-gravity of the gas on the GPU.  Every number the solver produces is held to tests/selfgravity_ref.py's `sg_direct`, a
plain double sum that contains no FFT; the transform alone to numpy.fft with the a-priori bound of the Cooley-Tukey
recursion; the kick to the reference's expression cell by cell; the in-step kick, the device loop and the switch back to
"off" to bit equality with the paths that exist without it."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups

from tests import rough_states
from tests import selfgravity_ref as R

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SHAPES = [(16, 24), (20, 30)]          # transform lengths 32, 24 (radices 2, 3, 4) and 40, 30 (radix 5 too)
MODES = [(B.SG_BASIC, "basic"), (B.SG_SYMMETRIC, "symmetric")]
H, TSS = 0.05, 0.6


def five_smooth(n):
    for p in (2, 3, 5):
        while n % p == 0:
            n //= p
    return n == 1


FFT_LENGTHS = [n for n in range(1, 65) if five_smooth(n)] + [96, 125, 243, 384, 1000, 1536, 4096, 6144, 8192]


def rel_l2(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb > 0 else np.linalg.norm(a - b)


@pytest.fixture(scope="module")
def fft_cases():
    """Seeded complex noise (3 rows per length) and numpy's transforms of it, computed once."""
    rng = np.random.default_rng(20261021)
    out = {}
    for n in FFT_LENGTHS:
        x = rng.standard_normal((3, n)) + 1j * rng.standard_normal((3, n))
        out[n] = (x, np.fft.fft(x, axis=1), np.fft.ifft(x, axis=1) * n)
    return out


@pytest.mark.parametrize("n", FFT_LENGTHS)
def test_fft_against_numpy(product, fft_cases, n):
    """|X - numpy|_2 / |numpy|_2 <= 16 eps log2 n: the classical a-priori bound of the Cooley-Tukey recursion, about
    8 eps log2 n, doubled because numpy's own float64 result carries the same error.  Forward, inverse (unnormalised), and
    forward then inverse = n x."""
    x, fwd, inv = fft_cases[n]
    bar = 16 * EPS * np.log2(n)
    got_f = product.selftest_fft(x)
    got_i = product.selftest_fft(x, inverse=True)
    back = product.selftest_fft(got_f, inverse=True)
    for row in range(3):
        errs = (rel_l2(got_f[row], fwd[row]), rel_l2(got_i[row], inv[row]), rel_l2(back[row], n * x[row]))
        print(f"n = {n} row {row}: forward {errs[0]:.3e} inverse {errs[1]:.3e} round trip {errs[2]:.3e} (bar {bar:.3e})")
        assert max(errs) <= bar


def sg_context(product, nr, nphi, sigma=None, fields=None, d=None, prepare=False):
    d = setups.planet_disk(product, nr, nphi) if d is None else d
    radii = product.radii(d)
    if fields is None:
        fields = [f.copy() for f in product.initial_fields(d.copy(), radii)]
    if sigma is not None:
        fields[0] = sigma
    ctx = driver.make_context(product, d, fields=fields, radii=radii)
    if sigma is not None:
        ctx.upload(B.F_SIGMA, sigma)   # again: init_physics' boundary call has rewritten the two ghost rings
    if prepare:
        driver.SlabSet([ctx]).prepare()
    return ctx, d, radii


def accel(ctx):
    return ctx.download(B.F_SG_ACCEL_RAD), ctx.download(B.F_SG_ACCEL_AZI)


@pytest.fixture(scope="module")
def direct_cases(product):
    """Random Sigma in [0.5, 1.5] and the plain sum over it, once per (shape, mode)."""
    out = {}
    for nr, nphi in SHAPES:
        d = setups.planet_disk(product, nr, nphi)
        radii = product.radii(d)
        sigma = np.random.default_rng(100 * nr + nphi).uniform(0.5, 1.5, size=(nr, nphi))
        for mode, _ in MODES:
            out[nr, nphi, mode] = (sigma, R.sg_direct(sigma, radii, mode, H, TSS, G=d.G))
    return out


@pytest.mark.parametrize("mode,name", MODES)
@pytest.mark.parametrize("nr,nphi", SHAPES)
def test_solver_against_direct_sum(product, direct_cases, nr, nphi, mode, name):
    sigma, ref = direct_cases[nr, nphi, mode]
    ctx, d, radii = sg_context(product, nr, nphi, sigma=sigma)
    ctx.selfgravity(mode, H, TSS, in_step=False)
    p = ctx.selfgravity_get()
    assert (p.mode, p.in_step, p.aspect_ratio, p.thickness_smoothing_sg) == (mode, 0, H, TSS)
    ctx.selfgravity_compute()
    got = accel(ctx)
    ctx.close()
    for g, r, what in zip(got, ref, ("g_r", "g_phi")):
        err = np.abs(g - r).max() / np.abs(r).max()
        print(f"{nr}x{nphi} {name} {what}: {err:.3e} of max|g_ref|")
        assert err <= 1e-12


@pytest.mark.parametrize("mode,name", MODES)
@pytest.mark.parametrize("nr,nphi", SHAPES)
def test_planted_deltas(product, nr, nphi, mode, name):
    """Sigma zero but for one cell: g is the kernel table read off around that cell, with the two weights.  With the
    delta in the last ring, ring 0 must feel the far-field value K(u = -log(r_last / r_0)) -- without the zero padding
    the periodic transform would wrap the last ring round to sit next to ring 0."""
    ctx, d, radii = sg_context(product, nr, nphi)
    ctx.selfgravity(mode, H, TSS, in_step=False)
    cells = [(0, 0), (0, nphi - 1), (nr - 1, 0), (nr - 1, nphi - 1), (nr // 2 - 1, nphi // 3)]
    for i0, j0 in cells:
        sigma = np.zeros((nr, nphi))
        sigma[i0, j0] = 1.25
        ctx.upload(B.F_SIGMA, sigma)
        ctx.selfgravity_compute()
        got = accel(ctx)
        ref = R.weighted_kernel(radii, nr, nphi, mode, H, TSS, i0, j0, 1.25, G=d.G)
        for g, r, what in zip(got, ref, ("g_r", "g_phi")):
            err = np.abs(g - r).max() / np.abs(r).max()
            print(f"{nr}x{nphi} {name} delta at ({i0}, {j0}) {what}: {err:.3e}")
            assert err <= 1e-12
        if i0 == nr - 1:
            near = R.weighted_kernel(radii, nr, nphi, mode, H, TSS, 1, j0, 1.25, G=d.G)[0]   # a source one ring away
            far = abs(ref[0][0, j0])
            assert far < 0.05 * abs(near[0, j0]), "the far-field value is far below a neighbour's pull"
            assert abs(got[0][0, j0] - ref[0][0, j0]) <= 1e-12 * np.abs(ref[0]).max()
    ctx.close()


@pytest.mark.parametrize("nr,nphi", [(20, 30), (32, 128)])
def test_kick_alone(product, nr, nphi):
    """fcpt_selfgravity_kick(dt) on a rough state against update_velocities in numpy, fed with the accelerations the
    library itself computed (the solver has its own tests): cell-wise within 2 eps (|v| + dt |g|); v_r rows 0 and Nr
    keep their bits."""
    d0, radii, fields = rough_states.noisy(product, rough_states.case_desc(product, nr, nphi), seed=3)
    ctx, d, _ = sg_context(product, nr, nphi, fields=fields, d=d0)
    ctx.selfgravity(B.SG_SYMMETRIC, H, in_step=False)
    vr0, va0 = ctx.download(B.F_VRAD), ctx.download(B.F_VAZI)
    dt = 0.0123
    ctx.selfgravity_kick(dt)
    vr1, va1 = ctx.download(B.F_VRAD), ctx.download(B.F_VAZI)
    g_r, g_t = accel(ctx)
    ctx.close()
    assert np.abs(g_r).max() > 0 and np.abs(g_t).max() > 0
    ref_r, ref_a = R.kick(vr0, va0, g_r, g_t, radii, dt)
    assert np.array_equal(vr1[0], vr0[0]) and np.array_equal(vr1[nr], vr0[nr])
    gmax_r = np.zeros_like(vr0)
    gmax_r[1:nr] = np.maximum(np.abs(g_r[1:]), np.abs(g_r[:-1]))
    gmax_a = np.maximum(np.abs(g_t), np.abs(np.roll(g_t, 1, axis=1)))
    for got, ref, old, gm, what in ((vr1, ref_r, vr0, gmax_r, "v_r"), (va1, ref_a, va0, gmax_a, "v_phi")):
        excess = np.abs(got - ref) - 2 * EPS * (np.abs(ref) + dt * gm)
        print(f"{nr}x{nphi} {what}: max |got - ref| {np.abs(got - ref).max():.3e}, moved by {np.abs(got - old).max():.3e}")
        assert excess.max() <= 0
        assert np.abs(got - old).max() > 0


def stepped_pair(product, nr, nphi, leapfrog=False, graph=-1):
    """Two prepared contexts from one rough state."""
    d0, radii, fields = rough_states.noisy(product, rough_states.case_desc(product, nr, nphi, leapfrog=leapfrog), seed=5)
    out = []
    for _ in range(2):
        ctx, _, _ = sg_context(product, nr, nphi, fields=[f.copy() for f in fields], d=d0, prepare=True)
        ctx.set_option("graph_steps", graph)
        out.append(ctx)
    return out, d0


def assert_same_state(a, b):
    sa, sb = a.state(), b.state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    ca, cb = a.clock, b.clock
    assert (ca.time, ca.last_dt, ca.n_hydro_iter) == (cb.time, cb.last_dt, cb.n_hydro_iter)


def host_step(ctx, pre=None):
    dt = ctx.calculate_timestep(ctx.cfl())
    if pre is not None:
        pre(dt)
    ctx.step(dt)
    ctx.post(dt)
    return dt


@pytest.mark.parametrize("nr,nphi", [(32, 128), (16, 24)])   # marching source path, narrow-ring path
def test_in_step_order(product, nr, nphi):
    """in_step = 1 and fcpt_step(dt) against in_step = 0 and fcpt_selfgravity_kick(dt) followed by fcpt_step(dt): the same
    bits in Sigma, v_r, v_phi (the kick is the first thing the step does); and not vacuously: a run without self-gravity
    differs by more than 1e-8 in v_r."""
    (a, b), d = stepped_pair(product, nr, nphi)
    (off, _), _ = stepped_pair(product, nr, nphi)
    a.selfgravity(B.SG_SYMMETRIC, H, in_step=True)
    b.selfgravity(B.SG_SYMMETRIC, H, in_step=False)
    for _ in range(2):
        dt_a = host_step(a)
        dt_b = host_step(b, pre=b.selfgravity_kick)
        dt_off = host_step(off)
        assert dt_a == dt_b
    assert_same_state(a, b)
    vr_on, vr_off = a.download(B.F_VRAD), off.download(B.F_VRAD)
    diff = np.abs(vr_on - vr_off).max() / np.abs(vr_off).max()
    print(f"{nr}x{nphi}: v_r with self-gravity differs from the run without by {diff:.3e} (dt {dt_a:.3e}, {dt_off:.3e})")
    assert diff > 1e-8
    for c in (a, b, off):
        c.close()


@pytest.mark.parametrize("leapfrog", [False, True], ids=["euler", "leapfrog"])
def test_kick_length_of_one_step(product, leapfrog):
    """The self-gravity of ONE step adds dt g in all: Euler one kick with dt, leapfrog two with dt / 2
    (simulation.cpp:324, 379).  D = v(with) - v(without) after one fcpt_step(dt) is projected on K = the numpy kick of
    zero velocities over dt with the accelerations the library left: <D, K> / <K, K> is 1 for the right lengths, 2 if
    both leapfrog kicks ran with the full dt, 1/2 if one was lost.  The bound 0.25 is reasoning, not measurement: g is
    smooth on the scale of a cell (gravity of a disk with 10-30 % noise), so what the other terms of one step at CFL
    0.5 make of a perturbation dt g is smaller than it by the ratio of a cell to the scale of g, a few per cent, and g
    itself moves by the relative change of Sigma in one step; 0.25 separates 1 from 2 and 1/2 with room on both sides."""
    nr, nphi = 32, 128
    (on, off), d = stepped_pair(product, nr, nphi, leapfrog=leapfrog)
    on.selfgravity(B.SG_SYMMETRIC, H, in_step=True)
    dt = on.calculate_timestep(on.cfl())
    assert off.calculate_timestep(off.cfl()) == dt
    for c in (on, off):
        c.step(dt)
        c.post(dt)
    radii = product.radii(d)
    g_r, g_t = accel(on)
    k_r, k_a = R.kick(np.zeros((nr + 1, nphi)), np.zeros((nr, nphi)), g_r, g_t, radii, dt)
    d_r, d_a = on.download(B.F_VRAD) - off.download(B.F_VRAD), on.download(B.F_VAZI) - off.download(B.F_VAZI)
    on.close(), off.close()
    rows = slice(3, nr - 3)   # away from the ghost rings and the damping's strongest rings
    for diff, k, what in ((d_r, k_r, "v_r"), (d_a, k_a, "v_phi")):
        ratio = float((diff[rows] * k[rows]).sum() / (k[rows] * k[rows]).sum())
        print(f"{'leapfrog' if leapfrog else 'euler'} {what}: <D, K> / <K, K> = {ratio:.4f}")
        assert abs(ratio - 1.0) < 0.25


@pytest.mark.parametrize("leapfrog", [False, True], ids=["euler", "leapfrog"])
@pytest.mark.parametrize("nr,nphi,graph", [(32, 128, 1), (32, 128, 0), (16, 24, 1)], ids=["graph", "plain", "narrow-graph"])
def test_device_loop(product, nr, nphi, graph, leapfrog):
    """fcpt_run_steps(5) against five host-stepped steps with self-gravity in the step: the same bits in the state and the
    clock, the same smallest and largest step.  fcpt_run_steps captures a graph only in calls of 8 steps and more, so the
    cases that replay go on with 12 steps more on both sides, assert graph_replays > 0 and compare again."""
    (host, dev), d = stepped_pair(product, nr, nphi, leapfrog=leapfrog, graph=graph)
    for c in (host, dev):
        c.selfgravity(B.SG_SYMMETRIC, H, in_step=True)
        c.dt_statistics(reset=True)
    for _ in range(5):
        host_step(host)
    assert dev.run_steps(5) == 5
    assert_same_state(host, dev)
    assert host.dt_statistics() == dev.dt_statistics()
    if graph:
        for _ in range(12):
            host_step(host)
        assert dev.run_steps(12) == 12
        assert dev.get_option("graph_replays") > 0
        assert_same_state(host, dev)
        assert host.dt_statistics() == dev.dt_statistics()
    else:
        assert dev.get_option("graph_replays") == 0
    g_host, g_dev = accel(host), accel(dev)
    assert np.array_equal(g_host[0], g_dev[0]) and np.array_equal(g_host[1], g_dev[1])
    host.close(), dev.close()


def test_off_is_off(product):
    """Switched on, then off with mode 0: the steps have the bits of a context that never had it, host-stepped and in the
    replayed graph; the two grids are gone."""
    (never, was), d = stepped_pair(product, 32, 128, graph=1)
    was.selfgravity(B.SG_BASIC, H, TSS, in_step=True)
    host_step(was), host_step(never)
    assert not np.array_equal(was.download(B.F_VRAD), never.download(B.F_VRAD))
    for c in (never, was):   # the same state again
        c.close()
    (never, was), d = stepped_pair(product, 32, 128, graph=1)
    was.selfgravity(B.SG_BASIC, H, TSS, in_step=True)
    was.selfgravity_compute()
    was.selfgravity(B.SG_OFF)
    assert was.selfgravity_get().mode == B.SG_OFF
    with pytest.raises(B.FcptError):
        was.download(B.F_SG_ACCEL_RAD)
    with pytest.raises(B.FcptError):
        was.selfgravity_kick(0.1)
    for c in (never, was):
        for _ in range(3):
            host_step(c)
        assert c.run_steps(12) == 12
    assert was.get_option("graph_replays") > 0
    assert_same_state(never, was)
    never.close(), was.close()


def test_refusals_on_a_context(product):
    ctx, d, radii = sg_context(product, 16, 28)   # 28 = 4 * 7
    with pytest.raises(B.FcptError, match="28"):
        ctx.selfgravity(B.SG_BASIC, H, TSS)
    assert ctx.selfgravity_get().mode == B.SG_OFF
    with pytest.raises(B.FcptError):
        ctx.selfgravity_compute()
    ctx.close()
