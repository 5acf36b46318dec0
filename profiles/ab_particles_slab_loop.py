"""Particles inside fcpt_run_steps on several slabs against the host-stepped sequence.  One MI355X, 2 slabs as two processes
over the host-staged transport (fcpt_comm_init_host), wall time per step between two barriers, alternating pairs, three of
each, every figure printed with its pair by slab 0.

 (a) 2048 x 4096 isothermal + Jupiter with 1e6 particles in (ring, column)-sorted order, and 128 x 384 with 1e4: the
     host-stepped sequence (cfl_allreduce, calculate_timestep, particles_step, particles_migrate, step, exchange, post),
     run_steps with follow, run_steps without follow (the particles stay where they are).
 (b) the particle share of run_steps with follow, split: a run of its own under fcpt_profile_start with the five particle
     kernels selected; what the wall-time difference of (a) holds beyond them is the neighbour exchange of the migration.
 (c) with --parent PATH (a library built from the parent commit): run_steps on the same 2 slabs without particles, this
     build and the parent's, alternating; --parent-first measures the parent's first in every pair, --only-c skips (a), (b).
     --c-build this|parent keeps one of the two: one context per process, so that neither build's figures depend on a
     second context in the same process; run it once per build, alternating.

The host link blocks the host in every transfer: (a) measures the rehearsal transport, not xGMI.  The RCCL path between
several GPUs is not measured here, and has never been executed.

Prints the lines recorded in profiles/ab_particles_slab_loop.txt (python profiles/ab_particles_slab_loop.py [--parent PATH])."""
import ctypes, os, subprocess, sys, tempfile, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS, NSLABS = 3, 2
PARTICLE_KERNELS = ("k_particles_step", "k_particles_emigrate_count", "k_particles_emigrate_finish", "k_particles_emigrate",
                    "k_particles_immigrate")


def launcher():
    """one fresh process per slab; the first that fails or overstays ends the run"""
    with tempfile.TemporaryDirectory() as links:
        args = [a for a in sys.argv[1:]]
        procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), "--links", links] + args)
                 for r in range(NSLABS)]
        t_end = time.monotonic() + 900.0
        rc = 0
        for p in procs:
            try:
                rc = rc or p.wait(max(1.0, t_end - time.monotonic()))
            except subprocess.TimeoutExpired:
                rc = 124
        for p in procs:
            if p.poll() is None:
                p.kill()
        sys.exit(rc)


if "--rank" not in sys.argv:
    launcher()

os.environ.setdefault("FCPT_HOSTLINK_TIMEOUT", "120")
import fargocpt_amd
from fargocpt_amd import binding as B, driver, setups
import tests.particles_ref as R
import tests.particles_slab_cases as sc
from tests.particles_cases import CM

rank = int(sys.argv[sys.argv.index("--rank") + 1])
links = sys.argv[sys.argv.index("--links") + 1]
lib = fargocpt_amd.load()
parent = None
if "--parent" in sys.argv:
    parent = B.Library(ctypes.CDLL(os.path.abspath(sys.argv[sys.argv.index("--parent") + 1])), "fcpt_")


def say(text):
    if rank == 0:
        print(text, flush=True)


def slab(L, nr, nphi, warm, tag):
    """this process's slab of the 2-slab split, on a host link of its own, after sim::init and `warm` steps"""
    d = setups.planet_disk(L, nr, nphi)
    radii = L.radii(d)
    fields = L.initial_fields(d.copy(), radii)
    dk = sc.slab_descs(d, NSLABS)[rank]
    ctx = driver.make_context(L, dk, fields=sc.cut_fields(L, dk, fields), radii=radii, bodies=setups.jupiter_bodies(d))
    ctx.comm_init_host(os.path.join(links, "%s_%dx%d" % (tag, nr, nphi)))
    ctx.calculate_timestep(ctx.cfl_allreduce())         # main() and sim::init
    ctx.exchange()
    ctx.apply_boundary(0.0, False)
    ctx.calculate_timestep(ctx.cfl_allreduce())
    ctx.exchange()
    assert ctx.run_steps(warm) == warm
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
    order = np.lexsort((col, ring))
    return {k: v[order] for k, v in state.items()}


def host_loop(ctx, d, nsteps):
    ctx.comm_barrier(); t0 = time.perf_counter()
    for _ in range(nsteps):
        dt = ctx.calculate_timestep(ctx.cfl_allreduce())
        ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
        ctx.particles_migrate()
        ctx.step(dt); ctx.exchange(); ctx.post(dt)
    ctx.comm_barrier()
    return (time.perf_counter() - t0) / nsteps * 1e3


def device_loop(ctx, nsteps, follow=False):
    ctx.particles_follow_run_steps(follow)
    ctx.comm_barrier(); t0 = time.perf_counter()
    assert ctx.run_steps(nsteps) == nsteps
    ctx.comm_barrier()
    return (time.perf_counter() - t0) / nsteps * 1e3


def live(ctx):
    try:
        return ctx.particles_count()
    except B.FcptError:                      # a guard report (once): the count is what the call after it returns
        return ctx.particles_count()


def rows(nr, nphi, n, steps, warm):
    d, radii, ctx = slab(lib, nr, nphi, warm, "ab")
    prm = lib.particle_params_default(d)
    s = draw(d, radii, n)
    ctx.particles_slabs(True)
    ctx.particles_set(prm, np.arange(n), *(s[k] for k in R.FIELDS))
    host_loop(ctx, d, 4); device_loop(ctx, 8, True)                  # warm-up
    for pair in range(PAIRS):
        host = host_loop(ctx, d, steps)
        follow = device_loop(ctx, steps, True)
        bare = device_loop(ctx, steps, False)
        t = ctx.particles_slabs_get()
        say("(a)  %d x %d on %d slabs, %d particles (sorted), pair %d, %d steps: host-stepped sequence %.4f ms per step, run_steps "
            "with follow %.4f, run_steps without follow %.4f; slab 0: %d live, %d sent, %d received"
            % (nr, nphi, NSLABS, n, pair, steps, host, follow, bare, live(ctx), t.sent_inner + t.sent_outer, t.received))
    # (b) a run of its own: HIP events around the particle launches of run_steps with follow
    names = lib.kernel_names()
    for pair in range(PAIRS):
        device_loop(ctx, 4, True)
        ctx.profile_start([names.index(k) for k in PARTICLE_KERNELS], 1024)
        wall = device_loop(ctx, steps, True)
        prof = ctx.profile_stop()
        parts = ", ".join("%s %.4f" % (k, prof[k][0] / steps) for k in PARTICLE_KERNELS if k in prof)
        say("(b)  %d x %d on %d slabs, %d particles, pair %d, slab 0, ms per step under the profiler (wall %.4f): %s; kernels "
            "together %.4f" % (nr, nphi, NSLABS, n, pair, wall, parts, sum(v[0] for v in prof.values()) / steps))
    ctx.comm_barrier(); ctx.comm_destroy(); ctx.close()


def regression(nr, nphi, steps, warm):
    """(c) this build and the parent's on the same 2 slabs, no particles, alternating"""
    builds = (("this build", lib, "this"), ("parent", parent, "parent"))
    if "--parent-first" in sys.argv:         # (the first timed stretch of a process is slow)
        builds = builds[::-1]
    if "--c-build" in sys.argv:
        builds = tuple(b for b in builds if b[2] == sys.argv[sys.argv.index("--c-build") + 1])
    ctxs = {name: slab(L, nr, nphi, warm, tag)[2] for name, L, tag in builds}
    for pair in range(PAIRS):
        for name, ctx in ctxs.items():
            device_loop(ctx, 8)
            say("(c)  %d x %d on %d slabs, pair %d, %-10s run_steps without particles, %d steps: %.4f ms per step"
                % (nr, nphi, NSLABS, pair, name, steps, device_loop(ctx, steps)))
    for ctx in ctxs.values():
        ctx.comm_barrier(); ctx.comm_destroy(); ctx.close()


if "--only-c" not in sys.argv:
    rows(2048, 4096, 1_000_000, 30, 30)
    rows(128, 384, 10_000, 200, 30)
if parent is not None:
    regression(2048, 4096, 30, 30)
    regression(128, 384, 200, 30)
