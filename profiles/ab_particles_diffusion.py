"""k_particles_step after drag and diffusion became template arguments, on the protocol of profiles/ab_particles.py
(2048 x 4096 isothermal, 1e6 particles spread as Sigma, random and sorted upload order, HIP events around each launch):
  A/B  the default kernel <ADI, true, false> of this build against a build of the parent commit (its
       libfargocpt_hip.so in FCPT_PARENT_LIB), three alternating pairs in one process;
  the (drag, diffusion) = (on, on) and (off, on) kernels of this build beside it.
Prints the lines recorded in profiles/ab_particles_diffusion.txt.
Usage: FCPT_PARENT_LIB=/path/to/parent/libfargocpt_hip.so python profiles/ab_particles_diffusion.py"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fargocpt_amd
from fargocpt_amd import binding as B, driver, setups
import tests.particles_ref as R
from tests.particles_cases import CM

this = fargocpt_amd.load()
libs = {"this build": this}
if os.environ.get("FCPT_PARENT_LIB"):
    libs = {"parent": B.Library(ctypes.CDLL(os.environ["FCPT_PARENT_LIB"]), "fcpt_"), "this build": this}
d = setups.planet_disk(this, 2048, 4096)
d.viscous_alpha = 0.01
radii = this.radii(d)
g = R.Grid(radii, d.nr_global, d.nphi)
bodies = setups.jupiter_bodies(d)
n = 1_000_000
rng = np.random.default_rng(5)
lo, hi = d.rmin * 1.02, d.rmax * 0.98
r = (rng.uniform(lo ** 1.5, hi ** 1.5, n)) ** (1 / 1.5)          # dN/dr ~ Sigma r ~ r^(1/2)
phi = rng.uniform(0, 2 * np.pi, n)
radius = CM * 10.0 ** rng.uniform(-4, 2, n)
vk = np.sqrt(1.0 / r)
state = dict(r=r, phi=phi, r_dot=np.zeros(n), phi_dot=vk / r, radius=radius, stokes=np.full(n, 1e-2))
ring = np.searchsorted(g.rinf, r, side="right") - 1
col = np.floor(phi / g.dphi).astype(np.int64)
orders = {"random": np.arange(n), "sorted by (ring, column)": np.lexsort((col, ring))}
ctxs = {}
for name, lib in libs.items():
    ctx = driver.make_context(lib, d, radii=radii, bodies=bodies)
    S = driver.SlabSet([ctx]); S.prepare(); S.run(30)
    ctxs[name] = ctx
prm = this.particle_params_default(d)


def measure(name, order, switches=None):
    """ms per launch of k_particles_step over 20 launches after 5 warm-up steps; the gas does not move in between"""
    lib, ctx = libs[name], ctxs[name]
    o = orders[order]
    if switches is not None:
        ctx.particles_diffusion(switches[0], switches[1], 12345, 0)
    ctx.particles_set(prm, np.arange(n, dtype=np.uint64)[o], *(state[k][o] for k in R.FIELDS))
    dt = ctx.calculate_timestep(ctx.cfl())
    for _ in range(5):
        ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
    kid = lib.kernel_names().index("k_particles_step")
    ctx.profile_start([kid], 256)
    for _ in range(20):
        ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
    ms, cnt = ctx.profile_stop()["k_particles_step"]
    return ms / cnt, ctx.particles_count()


for rep in range(3):
    for order in orders:
        for name in libs:
            ms, alive = measure(name, order, (True, False) if name == "this build" else None)
            print("pair %d  %-26s %-10s default kernel %.4f ms per launch (%d of %d live)" % (rep, order, name, ms, alive, n), flush=True)
for rep in range(3):
    for order in orders:
        for label, sw in (("(on, on)", (True, True)), ("(off, on)", (False, True)), ("(off, off)", (False, False))):
            ms, alive = measure("this build", order, sw)
            print("run %d   %-26s (drag, diffusion) = %-10s %.4f ms per launch (%d of %d live)" % (rep, order, label, ms, alive, n), flush=True)
for ctx in ctxs.values():
    ctx.close()
