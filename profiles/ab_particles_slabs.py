"""Particles on several slabs (fcpt_particles_slabs): what the opt-in costs the default path, and what the slab path costs.
2048 x 4096 isothermal + Jupiter, 1e6 particles spread as Sigma (the draw of profiles/ab_particles_in_loop.py), one MI355X,
one process, three pairs of each, every figure printed with its pair.

 (a) with --parent PATH (a library built from the parent commit): the host-argument k_particles_step launch (HIP events of
     the library's profiler) of this build and of the parent's, interleaved, sorted and random upload order.
 (b) two slabs sharing the GPU in this process, sorted upload order, per step and slab: k_particles_step on the slab (HIP
     events); k_particles_emigrate + _finish + k_particles_immigrate with the messages left in device memory (wall time
     between two synchronisations over both slabs, halved); the same hand-over staged through host arrays as
     SlabSet.migrate_particles does it, i.e. plus the two fixed-length message copies per slab; the share of lanes that
     leave on a dead slot.  The transfer between GPUs (RCCL over xGMI) is not measured here: it needs two devices.

Prints the lines recorded in profiles/ab_particles_slabs.txt (python profiles/ab_particles_slabs.py [--parent PATH])."""
import ctypes, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fargocpt_amd
from fargocpt_amd import binding as B, driver, setups
import tests.particles_ref as R
from tests.particles_cases import CM

PAIRS, NR, NPHI, N = 3, 2048, 4096, 1_000_000
lib = fargocpt_amd.load()
parent = None
if "--parent" in sys.argv:
    parent = B.Library(ctypes.CDLL(sys.argv[sys.argv.index("--parent") + 1]), "fcpt_")


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
    return state, {"sorted": np.lexsort((col, ring)), "random": np.arange(n)}


def upload(ctx, prm, state, order):
    ctx.particles_set(prm, np.arange(order.size)[order], *(state[k][order] for k in R.FIELDS))


def step_launch(L, ctx, d, dt, launches):
    """ms per k_particles_step launch, from the profiler's events"""
    kid = L.kernel_names().index("k_particles_step")
    for _ in range(4):
        ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
    ctx.profile_start([kid], 256)
    for _ in range(launches):
        ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
    ms, cnt = ctx.profile_stop()["k_particles_step"]
    return ms / cnt, cnt


def default_path():
    ctxs = {}
    for name, L in (("this build", lib), ("parent", parent)):
        d = setups.planet_disk(L, NR, NPHI)
        radii = L.radii(d)
        ctx = driver.make_context(L, d, radii=radii, bodies=setups.jupiter_bodies(d))
        S = driver.SlabSet([ctx]); S.prepare(); S.run(8)
        ctxs[name] = (L, d, radii, ctx, ctx.calculate_timestep(ctx.cfl()))
    for order in ("sorted", "random"):
        for name, (L, d, radii, ctx, dt) in ctxs.items():
            state, orders = draw(d, radii, N)
            upload(ctx, L.particle_params_default(d), state, orders[order])
        for pair in range(PAIRS):
            for name, (L, d, radii, ctx, dt) in ctxs.items():
                ms, cnt = step_launch(L, ctx, d, dt, 20)
                print("(a)  %d x %d, %d particles (%s), pair %d, %-10s host-argument k_particles_step: %.4f ms per launch (%d launches)"
                      % (NR, NPHI, N, order, pair, name, ms, cnt), flush=True)
    for _, _, _, ctx, _ in ctxs.values():
        ctx.close()


def device_doubles(count):
    """The address of `count` doubles of device memory, zeroed (hipMalloc of the runtime the library has loaded)."""
    hip = ctypes.CDLL("libamdhip64.so")
    p = ctypes.c_void_p()
    assert hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(8 * count)) == 0
    assert hip.hipMemset(p, 0, ctypes.c_size_t(8 * count)) == 0
    return p.value


def slab_path(nslabs=2, rounds=20):
    d = setups.planet_disk(lib, NR, NPHI)
    radii = lib.radii(d)
    ctxs = []
    for rank in range(nslabs):
        dk = d.copy()
        dk.rank, dk.nranks = rank, nslabs
        ctxs.append(driver.make_context(lib, dk, radii=radii, bodies=setups.jupiter_bodies(dk)))
    S = driver.SlabSet(ctxs); S.prepare(); S.run(8)
    dt = S.calculate_timestep()
    state, orders = draw(d, radii, N)
    prm = lib.particle_params_default(d)
    for c in ctxs:
        c.particles_slabs(True)
        upload(c, prm, state, orders["sorted"])
    cnt = ctxs[0].particles_migrate_count()
    dev = [(device_doubles(cnt), device_doubles(cnt)) for _ in ctxs]
    ptr = lambda address: address

    def device_hand_over():
        for k, c in enumerate(ctxs):
            c.particles_migrate_pack(ptr(dev[k][0]) if k > 0 else None, ptr(dev[k][1]) if k < nslabs - 1 else None)
        for c in ctxs:
            c.synchronize()         # (the neighbour's stream reads the message)
        for k, c in enumerate(ctxs):
            c.particles_migrate_unpack(ptr(dev[k - 1][1]) if k > 0 else None, ptr(dev[k + 1][0]) if k < nslabs - 1 else None)
        for c in ctxs:
            c.synchronize()

    def timed(f):
        for _ in range(3):
            f()
        t0 = time.perf_counter()
        for _ in range(rounds):
            f()
        return (time.perf_counter() - t0) / rounds / nslabs * 1e3

    owned = [c.particles_count() for c in ctxs]
    for pair in range(PAIRS):
        step = [step_launch(lib, c, d, dt, 20)[0] for c in ctxs]
        kernels = timed(device_hand_over)
        staged = timed(S.migrate_particles)
        tot = [c.particles_slabs_get() for c in ctxs]
        print("(b)  %d x %d in %d slabs, %d particles (sorted), pair %d: k_particles_step on a slab %s ms per launch; "
              "emigrate + immigrate, messages on the device %.4f ms per slab and step; staged through host arrays (plus two "
              "copies of %d doubles each way) %.4f; lanes on a dead slot %s; %d records sent so far"
              % (NR, NPHI, nslabs, N, pair, " / ".join("%.4f" % s for s in step), kernels, cnt, staged,
                 " / ".join("%.3f" % (1.0 - o / N) for o in owned), sum(t.sent_inner + t.sent_outer for t in tot)), flush=True)
    for c in ctxs:
        c.close()


if parent is not None:
    default_path()
slab_path()
