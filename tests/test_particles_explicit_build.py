"""Every variant of k_particles_step_explicit and k_particles_timestep_init compiles for gfx950 without scratch memory:
the 24 stage values of the Cash-Karp substep stay in registers.  Cross-compiles fcpt_kernels.hip with
-Rpass-analysis=kernel-resource-usage as test_hot_kernel_occupancy_budget does; the VGPR counts and occupancies are
printed and recorded in DESIGN.md section 4, and carry no bar."""
import os
import re
import shutil
import subprocess

import pytest


def test_explicit_particle_kernels_use_no_scratch():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fargocpt_amd", "csrc", "fcpt_kernels.hip")
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-c", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+): (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    step = sorted(k for k in usage if "25k_particles_step_explicitILb" in k)
    init = sorted(k for k in usage if "25k_particles_timestep_initILb" in k)
    assert len(step) == 8 and len(init) == 2, (step, init)      # ADI x DRAG x CART, and CART
    for k in step + init:
        u = usage[k]
        print(k, "VGPRs %d, SGPRs %d, occupancy %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy [waves/SIMD]"]))
        assert u["ScratchSize [bytes/lane]"] == 0, (k, u)
