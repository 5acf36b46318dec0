#!/usr/bin/env python3
"""Times the batched disk force (fcpt_disk_on_bodies_begin/_end, k_disk_on_bodies + its final stage) on the bench grid
beside the single-body call (fcpt_disk_on_body_accel, k_disk_on_body: untouched by the batched path, so its figure is
the parent commit's), both as device time from fcpt_profile_start/stop, 7 repetitions of 50 calls each; then the
host-stepped loop of the driver, ms per step, --bodies circular against --bodies free with DiskFeedback: yes
(mpi_simple.yml at 2048 x 4096, 400 steps, 5 runs each)."""
import os, re, statistics, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa: F401  (HIP runtime first)
import fargocpt_amd
from fargocpt_amd import driver, setups

lib = fargocpt_amd.load()
names = lib.kernel_names()
K1, KN = names.index("k_disk_on_body"), names.index("k_disk_on_bodies")


def spread(v):
    return f"median {statistics.median(v):7.2f} us  min {min(v):7.2f}  max {max(v):7.2f}"


for adi in (False, True):
    d = setups.planet_disk(lib, 2048, 4096, adiabatic=adi)
    ctx = driver.make_context(lib, d, bodies=setups.jupiter_bodies(d))
    ctx.run_steps(3, snap=False)
    ctx.synchronize()
    eos = "ideal" if adi else "isothermal"
    for mode, sm in (("H per cell", -1.0), ("fixed", 0.03)):
        reps = []
        for _ in range(8):
            ctx.profile_start([K1], 256)
            for _ in range(50):
                ctx.disk_on_body_accel(1.0, 0.0, 1.0, sm)
            reps.append(ctx.profile_stop()["k_disk_on_body"][0] * 1e3 / 50)
        print(f"{eos} 2048x4096, smoothing {mode}, single-body call (both stages): {spread(reps[1:])}")
        for n in (1, 2, 4, 8):
            ang = np.linspace(0.0, 2.0, n)
            r = np.linspace(1.0, 1.6, n)
            args = (r * np.cos(ang), r * np.sin(ang), r, np.full(n, sm), np.zeros(n))
            reps = []
            for _ in range(8):
                ctx.profile_start([KN], 256)
                for _ in range(50):
                    ctx.disk_on_bodies(*args)
                reps.append(ctx.profile_stop()["k_disk_on_bodies"][0] * 1e3 / 50)
            print(f"{eos} 2048x4096, smoothing {mode}, batched n = {n} (both stages):        {spread(reps[1:])}")
    ctx.close()

BIN = os.path.join(ROOT, "fargocpt_amd", "bin", "fargocpt_hip")
text = open(os.path.join(ROOT, "tests", "golden", "setups", "mpi_simple.yml")).read().splitlines()
with tempfile.TemporaryDirectory() as tmp:
    edits = {"Nrad": "2048", "Naz": "4096", "OutputDir": os.path.join(tmp, "out"), "Nsnapshots": "100"}
    text = [f"{l.split(':')[0].strip()}: {edits[l.split(':')[0].strip()]}" if l.split(":")[0].strip() in edits else l for l in text]
    cfg = os.path.join(tmp, "config.yml")
    open(cfg, "w").write("\n".join(text) + "\n")
    for mode in ("circular", "free"):
        ms = []
        for _ in range(5):
            r = subprocess.run([BIN, "-N", "400", "--bodies", mode, "start", cfg], capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            ms.append(float(re.search(r"Time per Step: ([0-9.]+) milliseconds", r.stdout).group(1)))
        print(f"driver, mpi_simple.yml at 2048x4096 (isothermal + Jupiter), 400 host-stepped steps, --bodies {mode}: "
              f"median {statistics.median(ms):.3f} ms per step  min {min(ms):.3f}  max {max(ms):.3f}  (5 runs, wall clock incl. snapshot 0)")
