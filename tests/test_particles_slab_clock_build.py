"""The particle kernels of fcpt_run_steps on several slabs exist for gfx950 and use no scratch memory: the eight
instances of k_particles_step_explicit_slab_clock (ADI x DRAG x CART) and the eight of k_particles_step<ADI, DRAG, DIFF, true,
true>.  Cross-compiles fcpt_kernels.hip exactly as test_particles_explicit_build.py does; the VGPR counts and occupancies are
printed and recorded in DESIGN.md section 4, and carry no bar."""
import os
import re
import shutil
import subprocess

import pytest

EXPLICIT = "k_particles_step_explicit_slab_clock"
MIDPOINT = "k_particles_step"


def test_slab_clock_particle_kernels_exist_and_use_no_scratch():
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
    # Itanium mangling: <length><name>I<template arguments>E, a bool argument is Lb0E / Lb1E
    explicit = sorted(k for k in usage if "%d%sILb" % (len(EXPLICIT), EXPLICIT) in k)
    midpoint = sorted(k for k in usage if re.search(r"%d%sI(Lb[01]E){3}Lb1ELb1EE" % (len(MIDPOINT), MIDPOINT), k))
    assert len(explicit) == 8, explicit         # ADI x DRAG x CART
    assert len(midpoint) == 8, midpoint         # ADI x DRAG x DIFF with DEV and SLAB
    for k in explicit + midpoint:
        u = usage[k]
        print(k, "VGPRs %d, SGPRs %d, occupancy %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy [waves/SIMD]"]))
        assert u["ScratchSize [bytes/lane]"] == 0, (k, u)
