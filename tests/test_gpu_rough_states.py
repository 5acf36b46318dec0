"""Parity from rough states, cell by cell: HIP against the oracle from noisy, floored and shocked states
(tests/rough_states.py) over one and two steps, in the host loop and (one slab) in the device loop.

Every grid the step writes is compared cell-wise (tests/util.py:cell_err, 1e-10 against the cell's own value or
the field's local scale), the heating and cooling rates included: before the first step both libraries get the same
non-zero sentinel in Q+ and Q-, so an edge ring that a step never writes cannot pass by holding 0 by luck.  Q+ and
Q- on rings 0 and Nr-1 must equal the oracle's exactly.  Each case also asserts that the kernels it is meant to test
ran (the profiler's launch counts), so that a state which trips a fallback or a changed dispatch cannot pass while
testing something else."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver
from tests import rough_states as R
from tests.util import _tolerance, cell_err, cell_scales, gather_grids

pytestmark = pytest.mark.gpu
TOL = 1e-10
TOL_DT = 1e-12

SOURCE_MARCH = ("k_source_march", "k_source_march_adi", "k_source_march_adi_wide", "k_source_march_adi_acc")
TRANSPORT_FUSED = ("k_transport_fused",)
TRANSPORT_TWO = ("k_transport_radial", "k_transport_radial_means")
CFL_RINGS = ("k_cfl_rings", "k_cfl_rings_bc")


def _sentinel(shape):
    """Q+ = Q- = the same non-zero pattern: Q+ - Q- (what the thermal CFL limit reads) stays 0."""
    nr, nphi = shape
    return 1.0e-3 * (1.0 + 0.25 * np.cos(np.arange(nphi))[None, :] + 0.01 * np.arange(nr)[:, None])


def _run(lib, d0, radii, fields, nslabs, nsteps, loop, noise=0.0, profile=False, dt_scale=1.0):
    """One library from the given global state: (grids, dt history or [time], profile, fell-back flags)."""
    if noise:
        rng = np.random.default_rng(7)
        fields = [f * (1.0 + noise * rng.standard_normal(f.shape)) for f in fields]
    ctxs = []
    for rank in range(nslabs):
        dd = d0.copy()
        dd.rank, dd.nranks = rank, nslabs
        s = lib.split_domain(dd)
        sub = tuple(np.ascontiguousarray(f[s.imin:s.imin + s.nr + (1 if k == 1 else 0)]) for k, f in enumerate(fields))
        ctx = driver.make_context(lib, dd, fields=sub, radii=radii)
        if d0.eos == B.EOS_IDEAL:
            # (this replaces the Q- that init_physics computed for the cooling cases: with Q+ = Q- the first step's
            # thermal CFL term is 0 on both sides, so the init-time Q- is not what these states compare)
            q = _sentinel((s.nr, d0.nphi))
            ctx.upload(B.F_QPLUS, q)
            ctx.upload(B.F_QMINUS, q)
        ctxs.append(ctx)
    S = driver.SlabSet(ctxs)
    S.dt_scale = dt_scale
    S.prepare()
    prof, fell = {}, []
    if profile:
        ctxs[0].profile_start()
    if loop == "host":
        dts = []
        for _ in range(nsteps):
            dts.append(S.step())
            if profile and lib.has("get_option"):
                fell.append(ctxs[0].get_option("transport_fell_back"))
    else:
        assert ctxs[0].run_steps(nsteps) == nsteps
        dts = [ctxs[0].clock.time]
    if profile:
        prof = ctxs[0].profile_stop()
    names = ["sigma", "vrad", "vazi"]
    if d0.eos == B.EOS_IDEAL:
        names += ["energy", "qplus", "qminus"]
    if d0.write_massflow:
        names.append("massflow")
    out = gather_grids(S, names)
    for c in ctxs:
        c.close()
    return out, dts, prof, fell


def _errors(d0, radii, a, b, time):
    scales = cell_scales(d0, radii, b, time)
    return {k: cell_err(a[k], b[k], scales[k]) for k in b}


def _assert_paths(name, opt, prof, fell):
    ran = lambda names: sum(prof.get(n, (0, 0))[1] for n in names)
    if opt["src"] == "march":
        assert ran(SOURCE_MARCH) > 0, f"{name}: no marching source kernel ran: {sorted(prof)}"
    else:
        assert ran(SOURCE_MARCH) == 0, f"{name}: a marching source kernel ran on a per-loop case: {sorted(prof)}"
    if opt["tr"] in ("fused", "fallback"):
        assert ran(TRANSPORT_FUSED) > 0, f"{name}: k_transport_fused did not run: {sorted(prof)}"
        if opt["tr"] == "fused":
            # the fallback's azimuthal launch is queued behind every fused one and returns at once unless the
            # shift-jump stamp is raised: the stamp, not the launch count, says whether it computed the step
            assert ran(TRANSPORT_TWO) == 0 and not any(fell), f"{name}: the transport fell back: {fell} {sorted(prof)}"
        else:
            assert fell and fell[0] == 1, f"{name}: the shift jump did not send the step to the fallback: {fell}"
    else:
        assert ran(TRANSPORT_FUSED) == 0 and ran(TRANSPORT_TWO) > 0, f"{name}: {sorted(prof)}"
    if opt["cfl"] == "rings":
        assert ran(CFL_RINGS) > 0, f"{name}: k_cfl_rings did not run: {sorted(prof)}"
    elif opt["cfl"] == "cells":
        assert ran(CFL_RINGS) == 0 and ran(("k_cfl_cells",)) > 0 and ran(("k_ring_mean",)) > 0, \
            f"{name}: expected k_ring_mean + k_cfl_cells: {sorted(prof)}"


def _compare(name, d0, radii, fields, nslabs, nsteps, loop, product, oracle, opt):
    sc = opt.get("dt_scale", 1.0)
    b, dtb, _, _ = _run(oracle, d0, radii, fields, 1, nsteps, loop, dt_scale=sc)
    a, dta, prof, fell = _run(product, d0, radii, fields, nslabs, nsteps, loop, profile=True, dt_scale=sc)
    _assert_paths(name, opt, prof, fell)
    assert all(np.isfinite(v).all() for v in b.values()), f"{name}: the oracle left the finite range"
    for q in ("qplus", "qminus"):
        if q in b:
            for ring in (0, b[q].shape[0] - 1):
                bad = np.flatnonzero(a[q][ring] != b[q][ring])
                assert bad.size == 0, (f"{name} ({loop}, {nsteps} steps): {q} ring {ring} differs from the oracle's in "
                                       f"{bad.size} cells, e.g. column {bad[0]}: {a[q][ring][bad[0]]!r} vs "
                                       f"{b[q][ring][bad[0]]!r}")
    time = sum(dtb)   # (the device loop's [clock time])
    errs = _errors(d0, radii, a, b, time)
    dterr = max(abs(x - y) / y for x, y in zip(dta, dtb))
    worst = max(e for e, _ in errs.values())
    tol, growth = TOL, 1.0
    if worst > TOL:
        fields_cmp = list(b)
        tol, growth = _tolerance(lambda noise: _run(oracle, d0, radii, fields, 1, nsteps, loop, noise=noise, dt_scale=sc)[0], b,
                                 fields_cmp, worst,
                                 measure=lambda x, y, k: cell_err(x, y, cell_scales(d0, radii, b, time)[k])[0])
        print(f"[rough] {name} {loop} {nsteps} steps: growth-based bar {tol:.1e} (growth {growth:.1e})")
    assert dterr <= TOL_DT, f"{name} ({loop}, {nsteps} steps): dt differs by {dterr:.3e}"
    for k, (e, (i, j)) in errs.items():
        assert e <= tol, (f"{name} ({loop}, {nsteps} steps): {k} at ring {i}, column {j}: {e:.3e} > {tol:.1e} "
                          f"(HIP {a[k][i, j]!r}, oracle {b[k][i, j]!r}, growth {growth:.1e})")


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_rough_state_parity(product, oracle, case):
    name, nr, nphi, physics, kind, opt = case
    d = R.case_desc(product, nr, nphi, physics, kind, av=opt.get("av", "TW"), leapfrog=opt.get("leapfrog", False),
                    massflow=opt.get("massflow", False))
    d0, radii, fields = R.make_state(product, d, kind, nslabs=opt["slabs"])
    loops = ["host"] + (["device"] if opt["slabs"] == 1 and opt["tr"] != "fallback" else [])
    for loop in loops:
        for nsteps in (1, 2):
            _compare(name, d0, radii, fields, opt["slabs"], nsteps, loop, product, oracle, opt)

