"""The explicit adaptive particle integrator on the protocol of profiles/ab_particles.py (2048 x 4096 isothermal, 1e6
particles spread as Sigma, random and sorted upload order, HIP events around each launch):
  (a) the midpoint kernel k_particles_step<ADI, true, false> of this build against a build of the parent commit (its
      libfargocpt_hip.so in FCPT_PARENT_LIB), three alternating pairs in one process: the explicit kernel must not have
      leaked into the default path;
  (b) k_particles_step_explicit at the hydro step of the CFL size, drag on / off, polar / Cartesian state: ms per launch,
      mean and maximum substeps per particle, and the mean over wavefronts of (maximum substeps in the wave) / (mean
      substeps in the wave), the price of divergence.  Bodies of 10 m to 1 km (t_stop >= 10 dt).
Prints the lines recorded in profiles/ab_particles_explicit.txt.
Usage: FCPT_PARENT_LIB=/path/to/parent/libfargocpt_hip.so [FCPT_MIDPOINT_PAIRS=3] [FCPT_EXPLICIT_RUNS=3]
       python profiles/ab_particles_explicit.py"""
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
vk = np.sqrt(1.0 / r)
ring = np.searchsorted(g.rinf, r, side="right") - 1
col = np.floor(phi / g.dphi).astype(np.int64)
orders = {"random": np.arange(n), "sorted by (ring, column)": np.lexsort((col, ring))}
small = dict(r=r, phi=phi, r_dot=np.zeros(n), phi_dot=vk / r, radius=CM * 10.0 ** rng.uniform(-4, 2, n), stokes=np.full(n, 1e-2))
# nobody of the explicit runs starts within 0.1 of the planet at (1, 0): with St = 1e3 the softening length is 1e-4, and a
# body that starts 1e-3 from the planet needs more than 10000 substeps per call (guard 9 reports it)
near = (np.abs(r - 1.0) < 0.1) & (np.abs(np.mod(phi + np.pi, 2 * np.pi) - np.pi) < 0.1)
large = dict(small, phi=np.where(near, phi + 0.5, phi), radius=CM * 10.0 ** rng.uniform(3, 5, n), stokes=np.full(n, 1e3))
ctxs = {}
for name, lib in libs.items():
    ctx = driver.make_context(lib, d, radii=radii, bodies=bodies)
    S = driver.SlabSet([ctx]); S.prepare(); S.run(30)
    ctxs[name] = ctx
prm = this.particle_params_default(d)
ids = np.arange(n, dtype=np.uint64)


def midpoint(name, order):
    """ms per launch of k_particles_step over 20 launches after 5 warm-up steps; the gas does not move in between"""
    lib, ctx = libs[name], ctxs[name]
    o = orders[order]
    ctx.particles_set(prm, ids[o], *(small[k][o] for k in R.FIELDS))
    dt = ctx.calculate_timestep(ctx.cfl())
    for _ in range(5):
        ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
    ctx.profile_start([lib.kernel_names().index("k_particles_step")], 256)
    for _ in range(20):
        ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
    ms, cnt = ctx.profile_stop()["k_particles_step"]
    return ms / cnt, ctx.particles_count()


def explicit(order, drag, cartesian):
    ctx = ctxs["this build"]
    o = orders[order]
    s = {k: large[k][o] for k in R.FIELDS}
    if cartesian:
        c, sn = np.cos(s["phi"]), np.sin(s["phi"])
        x, y = s["r"] * c, s["r"] * sn
        vx, vy = -s["r"] * s["phi_dot"] * sn, s["r"] * s["phi_dot"] * c
        s.update(r=x, phi=y, r_dot=vx, phi_dot=vy)
    ctx.particles_integrator(kind=B.INTEGRATOR_EXPLICIT, cartesian=cartesian)
    ctx.particles_diffusion(gas_drag=drag)
    ctx.particles_set(prm, ids[o], *(s[k] for k in R.FIELDS))
    ctx.particles_timestep_init()
    dt = ctx.calculate_timestep(ctx.cfl())
    for _ in range(5):
        ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
    ctx.profile_start([this.kernel_names().index("k_particles_step_explicit")], 256)
    for _ in range(20):
        ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
    ms, cnt = ctx.profile_stop()["k_particles_step_explicit"]
    alive = ctx.particles_count()
    ad = ctx.particles_adaptive_get()
    ctx.particles_integrator(kind=B.INTEGRATOR_MIDPOINT)
    sub = (ad["accepted"] + ad["rejected"]).astype(np.float64)
    divergence = float("nan")
    if alive == n:      # slots = lanes only while nobody has left
        w = sub.reshape(-1, 64)
        divergence = float(np.mean(w.max(axis=1) / w.mean(axis=1)))
    return ms / cnt, alive, dt, sub.mean(), sub.max(), divergence


for rep in range(int(os.environ.get("FCPT_MIDPOINT_PAIRS", "3"))):
    for order in orders:
        for name in libs:
            ms, alive = midpoint(name, order)
            print("pair %d  %-26s %-10s midpoint kernel %.4f ms per launch (%d of %d live)" % (rep, order, name, ms, alive, n), flush=True)
for rep in range(int(os.environ.get("FCPT_EXPLICIT_RUNS", "3"))):
    for order in orders:
        for drag in (True, False):
            for cartesian in (False, True):
                ms, alive, dt, mean, most, div = explicit(order, drag, cartesian)
                print("run %d   %-26s explicit drag=%d cartesian=%d dt=%.3e  %.4f ms per launch, substeps mean %.3f max %d, "
                      "wave max/mean %.3f (%d of %d live)" % (rep, order, drag, cartesian, dt, ms, mean, most, div, alive, n), flush=True)
for ctx in ctxs.values():
    ctx.close()
