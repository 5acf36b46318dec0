"""The particle step inside fcpt_run_steps (fcpt_particles_follow_run_steps) against the host-stepped loop.  Wall time per
step between two synchronisations, pairs in one process, three of each, every figure printed with its pair.

 (a) 2048 x 4096 isothermal + Jupiter, 1e6 particles spread as Sigma, in random and in (ring, column)-sorted upload order:
     the host-stepped loop with particles, fcpt_run_steps with follow, fcpt_run_steps without particles.
 (b) 128 x 384 isothermal + Jupiter (launch-bound: the hipGraph is replayed by default), 1e4 particles: the same rows.
 (c) with --parent PATH (a library built from the parent commit): fcpt_run_steps without particles and the host-argument
     k_particles_step launch (HIP events) of this build and of the parent's, interleaved; --parent-first measures the
     parent's first in every pair (the first timed stretch of a process is slow), --only-c skips (a) and (b).

Prints the lines recorded in profiles/ab_particles_in_loop.txt (python profiles/ab_particles_in_loop.py [--parent PATH])."""
import ctypes, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fargocpt_amd
from fargocpt_amd import binding as B, driver, setups
import tests.particles_ref as R
from tests.particles_cases import CM

PAIRS = 3
lib = fargocpt_amd.load()
parent = None
if "--parent" in sys.argv:
    parent = B.Library(ctypes.CDLL(sys.argv[sys.argv.index("--parent") + 1]), "fcpt_")


def context(L, nr, nphi, warm):
    d = setups.planet_disk(L, nr, nphi)
    radii = L.radii(d)
    ctx = driver.make_context(L, d, radii=radii, bodies=setups.jupiter_bodies(d))
    S = driver.SlabSet([ctx]); S.prepare(); S.run(warm)
    return d, radii, ctx


def draw(d, radii, n, seed=5):
    g = R.Grid(radii, d.nr_global, d.nphi)
    rng = np.random.default_rng(seed)
    lo, hi = d.rmin * 1.02, d.rmax * 0.98
    r = (rng.uniform(lo ** 1.5, hi ** 1.5, n)) ** (1 / 1.5)          # dN/dr ~ Sigma r ~ r^(1/2)
    phi = rng.uniform(0, 2 * np.pi, n)
    radius = CM * 10.0 ** rng.uniform(-4, 2, n)
    state = dict(r=r, phi=phi, r_dot=np.zeros(n), phi_dot=np.sqrt(1.0 / r) / r, radius=radius, stokes=np.full(n, 1e-2))
    ring = np.searchsorted(g.rinf, r, side="right") - 1
    col = np.floor(phi / g.dphi).astype(np.int64)
    return state, {"random": np.arange(n), "sorted": np.lexsort((col, ring))}


def host_loop(ctx, d, nsteps, particles):
    ctx.synchronize(); t0 = time.perf_counter()
    for _ in range(nsteps):
        dt = ctx.calculate_timestep(ctx.cfl())
        if particles:
            ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
        ctx.step(dt); ctx.post(dt)
    ctx.synchronize()
    return (time.perf_counter() - t0) / nsteps * 1e3


def device_loop(ctx, nsteps):
    ctx.synchronize(); t0 = time.perf_counter()
    assert ctx.run_steps(nsteps) == nsteps
    ctx.synchronize()
    return (time.perf_counter() - t0) / nsteps * 1e3


def upload(ctx, prm, state, order):
    n = order.size
    ctx.particles_set(prm, np.arange(n)[order], *(state[k][order] for k in R.FIELDS))


def clear(ctx, prm):
    ctx.particles_set(prm, np.zeros(0, dtype=np.uint64), *(np.zeros(0),) * 6)


def three_rows(tag, nr, nphi, n, steps, warm):
    d, radii, ctx = context(lib, nr, nphi, warm)
    prm = lib.particle_params_default(d)
    state, orders = draw(d, radii, n)
    ctx.particles_follow_run_steps(True)
    for name, o in orders.items():
        for pair in range(PAIRS):
            upload(ctx, prm, state, o)
            host_loop(ctx, d, 4, True); device_loop(ctx, 8)              # warm-up, graph capture
            replays = ctx.get_option("graph_replays")
            host = host_loop(ctx, d, steps, True)
            follow = device_loop(ctx, steps)
            replays = ctx.get_option("graph_replays") - replays
            try:
                alive = ctx.particles_count()
            except B.FcptError:                      # a guard report (once): the count is what the call after it returns
                alive = ctx.particles_count()
            clear(ctx, prm)
            device_loop(ctx, 8)
            bare = device_loop(ctx, steps)
            print("%s  %d x %d, %d particles (%s), pair %d, %d steps: host-stepped loop with particles %.4f ms per step, "
                  "run_steps with follow %.4f (%d graph replays), run_steps without particles %.4f; %d live"
                  % (tag, nr, nphi, n, name, pair, steps, host, follow, replays, bare, alive), flush=True)
    ctx.close()


def regression(nr, nphi, n, steps, warm):
    """this build and the parent's, interleaved: run_steps without particles, and the host-argument particle launch"""
    ctxs = {}
    builds = (("this build", lib), ("parent", parent))
    for name, L in builds[::-1] if "--parent-first" in sys.argv else builds:      # (the first timed stretch of a process is slow)
        d, radii, ctx = context(L, nr, nphi, warm)
        ctxs[name] = (L, d, radii, ctx)
    for pair in range(PAIRS):
        for name, (L, d, radii, ctx) in ctxs.items():
            device_loop(ctx, 8)
            print("(c)  %d x %d, pair %d, %-10s run_steps without particles, %d steps: %.4f ms per step"
                  % (nr, nphi, pair, name, steps, device_loop(ctx, steps)), flush=True)
    for name, (L, d, radii, ctx) in ctxs.items():
        state, orders = draw(d, radii, n)
        upload(ctx, L.particle_params_default(d), state, orders["sorted"])
    for pair in range(PAIRS):
        for name, (L, d, radii, ctx) in ctxs.items():
            kid = L.kernel_names().index("k_particles_step")
            host_loop(ctx, d, 4, True)
            ctx.profile_start([kid], 256)
            host_loop(ctx, d, 20, True)
            ms, cnt = ctx.profile_stop()["k_particles_step"]
            print("(c)  %d x %d, %d particles (sorted), pair %d, %-10s host-argument k_particles_step: %.4f ms per launch (%d launches)"
                  % (nr, nphi, n, pair, name, ms / cnt, cnt), flush=True)
    for _, _, _, ctx in ctxs.values():
        ctx.close()


if "--only-c" not in sys.argv:
    three_rows("(a)", 2048, 4096, 1_000_000, 30, 30)
    three_rows("(b)", 128, 384, 10_000, 200, 30)
if parent is not None:
    regression(2048, 4096, 1_000_000, 30, 30)
