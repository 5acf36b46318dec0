"""Cost of the self-gravity of the gas: ms per step of fcpt_run_steps with self-gravity off and on (symmetric mode,
locally isothermal, logarithmic grid) at 128 x 384, 512 x 1536 and 2048 x 4096, and the share of the solver's kernels
from fcpt_profile_start / fcpt_profile_stop.  Prints one line per grid; run on a GPU:

    python profiles/tools/ab_selfgravity.py [out.txt]

The timed stretches are wall time around run_steps + synchronize after a warm-up (measuring-on-mi355x: warm clocks,
several repetitions, the median); the profile is a separate run of 10 steps (profiling serialises the launches with
events and switches the graph replay off, so its per-kernel times say how the solver's time divides, not what a step
costs)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import fargocpt_amd
from fargocpt_amd import binding as B, driver, setups

GRIDS = [(128, 384, 200), (512, 1536, 100), (2048, 4096, 30)]   # nr, nphi, steps per timed stretch
REPEATS = 5


def timed(ctx, steps):
    ctx.run_steps(20)
    ctx.synchronize()
    ms = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        ctx.run_steps(steps)
        ctx.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0) / steps)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def main():
    lib = fargocpt_amd.load()
    lines = ["# nr nphi | off: median (min-max) ms/step | on: median (min-max) ms/step | profiled ms per compute+kick: fft transpose "
             "multiply kick | setup s"]
    for nr, nphi, steps in GRIDS:
        d = setups.planet_disk(lib, nr, nphi)
        ctx = driver.make_context(lib, d, bodies=setups.jupiter_bodies(d))
        driver.SlabSet([ctx]).prepare()
        off = timed(ctx, steps)
        t0 = time.perf_counter()
        ctx.selfgravity(B.SG_SYMMETRIC, d.aspect_ratio, in_step=True)
        setup_s = time.perf_counter() - t0
        on = timed(ctx, steps)
        ctx.profile_start(None, 4096)
        ctx.run_steps(10)
        prof = ctx.profile_stop()
        per = {k: prof.get(k, (0.0, 0))[0] / 10 for k in ("k_sg_fft_rows", "k_sg_transpose", "k_sg_multiply", "k_sg_kick")}
        total = sum(v[0] for v in prof.values()) / 10
        ctx.close()
        lines.append(f"{nr} x {nphi} | off {off[0]:.4f} ({off[1]:.4f}-{off[2]:.4f}) | on {on[0]:.4f} ({on[1]:.4f}-{on[2]:.4f}) | "
                     f"fft {per['k_sg_fft_rows']:.4f} transpose {per['k_sg_transpose']:.4f} multiply {per['k_sg_multiply']:.4f} "
                     f"kick {per['k_sg_kick']:.4f} of {total:.4f} profiled ms/step | setup {setup_s:.2f} s")
        print(lines[-1], flush=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
