"""What the step loop launches, case by case: per-kernel launch counts, digests of the grids it leaves, the clock and the
counters of the hipGraph replay, for small runs that reach every branch of the host code between the kernels (fcpt_step.hip
and the plans of fcpt_plan.cpp).  tests/test_gpu_launch_census.py compares the library of the working tree with the record
in tests/golden/launch_census.json;

    python -m tests.launch_census --record FILE

writes such a record from whatever library is loaded (FCPT_LIB_PATH: another build).  It runs every case twice: a case
whose digests do not come back the second time is recorded with counts and clock only, and named under "unstable".

Profiling switches the graph replay off, so a case either counts launches (graph_steps 0) or records graph_cycle and
graph_replays.  Every case is planet_disk with Jupiter and a dozen steps at the most, on 32 x 128 cells or fewer -- but for the
"wide" cases on 32 x 256: the fused transport, and with it the gated launch of its fallback, needs rings of 256 cells."""
import hashlib
import json
import sys

import numpy as np

from fargocpt_amd import binding as B, driver, setups

GRIDS = (("sigma", B.F_SIGMA), ("vrad", B.F_VRAD), ("vazi", B.F_VAZI), ("energy", B.F_ENERGY),
         ("qplus", B.F_QPLUS), ("qminus", B.F_QMINUS))
N_PARTICLES = 8
_FIELDS = {}


def _fields(product, d):
    key = (d.nr_global, d.nphi, d.eos, d.rank, d.nranks)
    if key not in _FIELDS:
        radii = product.radii(d)
        _FIELDS[key] = (radii, product.initial_fields(d.copy(), radii))
    return _FIELDS[key]


def _desc(product, nr=32, nphi=128, adiabatic=False, leapfrog=False, mean=False, stab=0, accel=False):
    d = setups.planet_disk(product, nr, nphi, adiabatic=adiabatic)
    d.stabilize_viscosity = stab
    if accel:   # BodyForceFromPotential: no
        d.body_force_from_potential = 0
    if leapfrog:
        d.integrator = B.INTEGRATOR_LEAPFROG
    if mean:   # a mean target: the damping cannot be folded into the transport
        for arr in (d.damp_vrad, d.damp_vaz, d.damp_sigma, d.damp_energy):
            arr[0] = arr[1] = B.DAMP_MEAN
    return d


def _context(product, d, graph=0, options=(), prepare=True):
    radii, fields = _fields(product, d)
    ctx = driver.make_context(product, d, fields=fields, radii=radii, bodies=setups.jupiter_bodies(d))
    ctx.set_option("graph_steps", graph)
    for name, value in options:
        ctx.set_option(name, value)
    if prepare:
        driver.SlabSet([ctx]).prepare()
    return ctx


def _digests(ctx):
    out = {}
    for name, f in GRIDS:
        if f == B.F_ENERGY and ctx.desc.eos != B.EOS_IDEAL:
            continue
        try:
            a = ctx.download(f)
        except B.FcptError:   # a grid this configuration does not have
            continue
        out[name] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    return out


def _clock(ctx):
    c = ctx.clock
    return [float(c.time).hex(), float(c.last_dt).hex(), int(c.n_hydro_iter), int(c.n_monitor), int(c.n_snapshot)]


def _counted(ctx, run, max_launches=1024):
    """run(ctx) between profile_start over all kernels and profile_stop -> the record of the case"""
    ctx.profile_start(None, max_launches=max_launches)
    run(ctx)
    prof = ctx.profile_stop()
    return {"counts": {k: int(v[1]) for k, v in sorted(prof.items())}, "digests": _digests(ctx), "clock": _clock(ctx)}


def _graphed(ctx, run):
    run(ctx)
    return {"graph": [int(ctx.get_option("graph_cycle")), int(ctx.get_option("graph_replays"))], "digests": _digests(ctx),
            "clock": _clock(ctx)}


def _steps(n, snap=False):
    def run(ctx):
        assert ctx.run_steps(n, snap=snap) == n
    return run


def _simple(n=6, snap=False, options=(), **desc):
    def case(product):
        ctx = _context(product, _desc(product, **desc), options=options)
        try:
            return _counted(ctx, _steps(n, snap))
        finally:
            ctx.close()
    return case


def _abi_by_hand(product):
    def run(ctx):
        for _ in range(2):
            dt = ctx.calculate_timestep(ctx.cfl())
            ctx.step(dt)
            ctx.post(dt)
        dt = ctx.calculate_timestep(ctx.cfl())
        ctx.step(0.5 * dt)
        ctx.step(0.5 * dt)   # no post in between: the ghost rings are the transport's, the separate boundary launch
        ctx.post(0.5 * dt)
    ctx = _context(product, _desc(product))
    try:
        return _counted(ctx, run)
    finally:
        ctx.close()


def _upload_between(product):
    def run(ctx):
        assert ctx.run_steps(3) == 3
        ctx.upload(B.F_SIGMA, ctx.download(B.F_SIGMA))   # ghosts_unknown
        assert ctx.run_steps(3) == 3
    ctx = _context(product, _desc(product))
    try:
        return _counted(ctx, run)
    finally:
        ctx.close()


def _leapfrog_mid(adiabatic):
    def case(product):
        d = _desc(product, adiabatic=adiabatic, leapfrog=True)
        ctx = _context(product, d)
        x, y, m = setups.jupiter_bodies(d)
        ctx.set_bodies_midstep([1.0005 * v for v in x], [v + 2.0e-4 for v in y], m)
        try:
            return _counted(ctx, _steps(4))
        finally:
            ctx.close()
    return case


def _graph(first, second=0, between=None, **desc):
    def case(product):
        d = _desc(product, **desc)
        ctx = _context(product, d, graph=1)

        def run(ctx):
            assert ctx.run_steps(first) == first
            if between:
                between(ctx, d)
            if second:
                assert ctx.run_steps(second) == second
        try:
            return _graphed(ctx, run)
        finally:
            ctx.close()
    return case


def _new_bodies(ctx, d):
    x, y, m = setups.jupiter_bodies(d)
    ctx.set_bodies([1.001 * v for v in x], y, m)


def _particles(graph):
    def case(product):
        import tests.particles_cases as cases
        import tests.particles_ref as R
        from tests.test_gpu_particles_run_steps import bulk
        d = cases.parity_desc(product, 32, 128, omega_frame=0.9)
        ctx = _context(product, d, graph=graph, prepare=False)
        ctx.set_bodies(*setups.jupiter_bodies(d), indirect=cases.PARITY_INDIRECT)
        driver.SlabSet([ctx]).prepare()
        ctx.particles_follow_run_steps(True)
        s = bulk(cases.census_draw, d, _fields(product, d)[0], n=N_PARTICLES)
        ctx.particles_set(cases.parity_params(product, d, False), s["id"], *(s[k] for k in R.FIELDS))

        def run(ctx):
            assert ctx.run_steps(12) == 12
        try:
            rec = (_graphed if graph else _counted)(ctx, run)
            got = ctx.particles_get()
            rec["digests"]["particles"] = hashlib.sha256(b"".join(np.ascontiguousarray(got[k]).tobytes() for k in R.FIELDS)).hexdigest()
            return rec
        finally:
            ctx.close()
    return case


def _slab_loopback(product):
    """The middle slab of three as its own neighbour on both sides (option comm_loopback, as tests/test_gpu_distributed.py):
    the loop with neighbours, then its monitor-snapping form."""
    d = _desc(product, 54, 128)
    d.rank, d.nranks = 1, 3
    ctx = _context(product, d, prepare=False)
    ctx.set_option("comm_loopback", 1)
    ctx.comm_init(product.comm_unique_id())
    ctx.calculate_timestep(ctx.cfl_allreduce())   # sim::init's sequence
    ctx.exchange()
    ctx.apply_boundary(0.0, False)
    ctx.calculate_timestep(ctx.cfl_allreduce())
    ctx.exchange()

    def run(ctx):
        assert ctx.run_steps(4) == 4
        assert ctx.run_steps(3, snap=True) == 3
    try:
        return _counted(ctx, run)
    finally:
        ctx.comm_destroy()
        ctx.close()


CASES = {"defaults": _simple()}
for _name, _value in (("bc_in_cfl", 2), ("cfl_fold_in_source", 0), ("gate_in_boundary", 0), ("bc_fold", 0), ("fused_damping", 0),
                      ("march_source", 0), ("cfl_rings", 0)):
    CASES["%s_%d" % (_name, _value)] = _simple(options=((_name, _value),))
CASES.update({
    "ideal": _simple(adiabatic=True),
    "ideal_march_source_adi_0": _simple(adiabatic=True, options=(("march_source_adi", 0),)),   # the derived grids are not lazy
    "ideal_inline_potential_0": _simple(adiabatic=True, options=(("inline_potential", 0),)),
    "leapfrog": _simple(leapfrog=True),
    "leapfrog_ideal": _simple(adiabatic=True, leapfrog=True),
    "leapfrog_mid_bodies": _leapfrog_mid(False),
    "leapfrog_ideal_mid_bodies": _leapfrog_mid(True),
    "narrow_24x64": _simple(nr=24, nphi=64),   # neither the source march nor the ring kernel of the CFL reduction
    # ... per kick k_src_fused, k_av_fused, k_visc_fused; StabilizeViscosity: k_visc_factors ahead of the last;
    # BodyForceFromPotential: no: k_accel_on_gas in k_potential's place.  These two pin LAUNCHES: with alpha = 1e-3 the
    # correction of StabilizeViscosity 1 is exactly 1, so the digests of narrow_24x64_stab1 are those of narrow_24x64 --
    # the arithmetic of k_visc_fused<true,.> is held by the stab1 cases of tests/symmetries.py and test_stabilize_viscosity
    "narrow_24x64_stab1": _simple(nr=24, nphi=64, stab=1),
    "narrow_24x64_accel": _simple(nr=24, nphi=64, accel=True),
    "mean_damping": _simple(mean=True),
    # rings of 256 cells, the narrowest that k_transport_fused takes: only there is there a gated launch of its fallback to
    # merge with the final boundary call (k_transport_theta_gated_boundary), or to queue alone where that call rides
    "wide_32x256": _simple(nphi=256),
    "wide_gate_in_boundary_0": _simple(nphi=256, options=(("gate_in_boundary", 0),)),
    "wide_bc_in_cfl_2": _simple(nphi=256, options=(("bc_in_cfl", 2),)),
    "wide_fused_damping_0": _simple(nphi=256, options=(("fused_damping", 0),)),
    "wide_ideal": _simple(nphi=256, adiabatic=True),
    "host_stepped_snap": _simple(n=4, snap=True),
    "abi_by_hand": _abi_by_hand,
    "upload_between": _upload_between,
    "graph_12_9": _graph(12, 9),
    "graph_set_bodies_between": _graph(12, 9, between=_new_bodies),
    "graph_leapfrog_12": _graph(12, leapfrog=True),
    "graph_wide_12_9": _graph(12, 9, nphi=256),
    "particles": _particles(0),
    "particles_graph": _particles(1),
    "slab_loopback": _slab_loopback,
})


def run_case(product, name):
    return CASES[name](product)


def _try_case(product, name):
    try:
        return run_case(product, name)
    except Exception as e:   # recorded, so that one call shows every case that cannot run; the test refuses such a record
        return {"error": repr(e)}


def record(product):
    first = {name: _try_case(product, name) for name in CASES}
    second = {name: _try_case(product, name) for name in CASES}
    unstable = {}
    for name in CASES:
        a, b = first[name], second[name]
        if "error" in a or "error" in b:
            first[name] = a if "error" in a else b
            continue
        assert {k: v for k, v in a.items() if k != "digests"} == {k: v for k, v in b.items() if k != "digests"}, \
            "%s: counts, graph counters or clock differ between two runs of the same build" % name
        if a["digests"] != b["digests"]:
            unstable[name] = "digests of %s differ between two runs of the recording build" % \
                ", ".join(k for k in a["digests"] if a["digests"][k] != b["digests"].get(k))
            a["digests"] = None
    return {"cases": first, "unstable": unstable}


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", __doc__
    import fargocpt_amd
    rec = record(fargocpt_amd.load())
    with open(sys.argv[2], "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases, unstable: %s" % (len(rec["cases"]), sorted(rec["unstable"]) or "none"))
