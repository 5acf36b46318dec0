"""k_particles_step at the headline grid (2048 x 4096 isothermal) with 1e6 particles spread as Sigma: time per launch
(HIP events, fcpt_profile_start/stop) in random upload order and sorted by (ring, column), and the host-stepped loop
with and without particles.  Prints the lines recorded in profiles/ab_particles.txt (run from anywhere: python profiles/ab_particles.py)."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fargocpt_amd
from fargocpt_amd import driver, setups
import tests.particles_ref as R
from tests.particles_cases import CM

lib = fargocpt_amd.load()
d = setups.planet_disk(lib, 2048, 4096)
radii = lib.radii(d)
g = R.Grid(radii, d.nr_global, d.nphi)
bodies = setups.jupiter_bodies(d)
ctx = driver.make_context(lib, d, radii=radii, bodies=bodies)
S = driver.SlabSet([ctx]); S.prepare(); S.run(30)
prm = lib.particle_params_default(d)
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
kid = lib.kernel_names().index("k_particles_step")
out = []
def loop(nsteps, particles):
    ctx.synchronize(); t0 = time.perf_counter()
    for _ in range(nsteps):
        dt = ctx.calculate_timestep(ctx.cfl())
        if particles:
            ctx.particles_step(dt, (0.0, 0.0), d.omega_frame * dt)
        ctx.step(dt); ctx.post(dt)
    ctx.synchronize()
    return (time.perf_counter() - t0) / nsteps * 1e3
for rep in range(3):
    for name, o in orders.items():
        ctx.particles_set(prm, np.arange(n)[o], *(state[k][o] for k in R.FIELDS))
        loop(5, True)                                   # warm-up
        ctx.profile_start([kid], 256)
        loop(20, True)
        ms, cnt = ctx.profile_stop()["k_particles_step"]
        alive = ctx.particles_count()
        out.append("pair %d  %-26s k_particles_step %.4f ms per launch (%d launches, %d of %d live)" % (rep, name, ms / cnt, cnt, alive, n))
        print(out[-1], flush=True)
    with_p = loop(30, True)
    ctx.particles_set(prm, np.zeros(0, dtype=np.uint64), *(np.zeros(0),) * 6)
    without = loop(30, False)
    out.append("pair %d  host-stepped loop (cfl, timestep, [particles,] step, post), 30 steps: %.4f ms per step with the sorted particles, %.4f without" % (rep, with_p, without))
    print(out[-1], flush=True)
ctx.close()
