"""Every instance of k_particles_step_explicit<ADI, DRAG, CART, DEV, SLAB> and k_particles_timestep_init, and the eight of
k_particles_step<ADI, DRAG, DIFF, true, true> that fcpt_run_steps launches on several slabs, exist for gfx950 and use no scratch
memory: the 24 stage values of the Cash-Karp substep stay in registers.  The explicit kernel is one template: no kernel of a
second name stands beside it.  Reads the remarks of tests/util.py:kernel_resource_usage as test_hot_kernel_occupancy_budget
does; the VGPR counts and occupancies are printed and recorded in DESIGN.md section 4, and carry no bar."""
import re

from tests.util import kernel_resource_usage

# Itanium mangling: <length><name>I<template arguments>E, a bool argument is Lb0E / Lb1E
NAME = "k_particles_step_explicit"
EXPLICIT = "25k_particles_step_explicitILb"


def explicit_instances(usage, dev, slab):
    """The instances of the explicit kernel with these DEV and SLAB ("0" / "1"), over ADI x DRAG x CART"""
    return sorted(k for k in usage if re.search(r"25%sI(Lb[01]E){3}Lb%sELb%sEE" % (NAME, dev, slab), k))


def no_scratch(usage, kernels):
    for k in kernels:
        u = usage[k]
        print(k, "VGPRs %d, SGPRs %d, occupancy %d" % (u["VGPRs"], u["TotalSGPRs"], u["Occupancy [waves/SIMD]"]))
        assert u["ScratchSize [bytes/lane]"] == 0, (k, u)


def test_explicit_particle_kernels_use_no_scratch():
    usage = kernel_resource_usage()
    step = sorted(k for k in usage if EXPLICIT in k)
    init = sorted(k for k in usage if "25k_particles_timestep_initILb" in k)
    assert len(step) == 32 and len(init) == 2, (step, init)      # ADI x DRAG x CART x DEV x SLAB, and CART
    for dev in "01":
        for slab in "01":
            pair = explicit_instances(usage, dev, slab)
            assert len(pair) == 8, (dev, slab, pair)             # ADI x DRAG x CART
    assert not [k for k in usage if re.search(NAME + "_(clock|slab)", k)]       # the names of the four-kernel form
    no_scratch(usage, step + init)


def test_slab_clock_particle_kernels_exist_and_use_no_scratch():
    """The particle kernels of fcpt_run_steps on several slabs: DEV and SLAB together, eight instances of either kernel"""
    usage = kernel_resource_usage()
    explicit = explicit_instances(usage, "1", "1")
    midpoint = sorted(k for k in usage if re.search(r"16k_particles_stepI(Lb[01]E){3}Lb1ELb1EE", k))
    assert len(explicit) == 8, explicit         # ADI x DRAG x CART
    assert len(midpoint) == 8, midpoint         # ADI x DRAG x DIFF with DEV and SLAB
    no_scratch(usage, explicit + midpoint)
