"""The runs and comparisons that the state-based parity tests share (tests/test_gpu_rough_states.py,
tests/test_gpu_shift_plants.py) and that their CPU censuses repeat with the oracle alone: one library advanced from a
given global state, with the same non-zero sentinel in Q+ and Q-, and the cell-wise comparison of every grid the step
writes at 1e-10, widened only by tests/util.py:_tolerance."""
from __future__ import annotations

import numpy as np

from fargocpt_amd import binding as B, driver
from tests.util import _tolerance, cell_err, cell_scales, gather_grids

TOL = 1e-10
TOL_DT = 1e-12

SOURCE_MARCH = ("k_source_march", "k_source_march_adi", "k_source_march_adi_wide", "k_source_march_adi_acc")
SOURCE_FUSED = ("k_src_fused", "k_av_fused", "k_visc_fused")
TRANSPORT_FUSED = ("k_transport_fused",)
TRANSPORT_TWO = ("k_transport_radial", "k_transport_radial_means")
CFL_RINGS = ("k_cfl_rings", "k_cfl_rings_bc")


def sentinel(shape):
    """Q+ = Q- = the same non-zero pattern: Q+ - Q- (what the thermal CFL limit reads) stays 0."""
    nr, nphi = shape
    return 1.0e-3 * (1.0 + 0.25 * np.cos(np.arange(nphi))[None, :] + 0.01 * np.arange(nr)[:, None])


def _step_forced(S, step_dt):
    """driver.SlabSet.step with the step length replaced: the CFL reduction and the step policy are still called (in the
    product the CFL launch carries the boundary call that the step loop folds into it), the CFL reduction's own result
    is returned and `step_dt` is what the slabs step with.  The contexts' clocks are then not the run's own: `time`
    advances by `step_dt`, but `last_dt` follows the policy on the CFL results.  Nothing compared from a forced run reads
    the clock (the grids, and `cfl_dts`)."""
    cfl_dt = S.global_cfl()
    for c in S.ctxs:
        c.calculate_timestep(cfl_dt)
    for c in S.ctxs:
        c.step(step_dt)
    S.exchange_local()
    for c in S.ctxs:
        c.post(step_dt)
    return cfl_dt


def run_state(lib, d0, radii, fields, nslabs, nsteps, loop, noise=0.0, profile=False, dt_scale=1.0, chunks=None,
              shifts=None, bodies=None, forced_dts=None, cfl_dts=None, source_chunks=None, sentinel_map=None):
    """One library from the given global state: (grids, dt history or [time], profile, fell-back flags).
    `chunks`: explicit chunk lengths of the fused transport (libraries that have set_transport_chunks), `source_chunks`
    those of the marching source kernel (set_source_chunks).  `shifts`: a list that receives (Nshift, Ntilde) of every
    ring after each step of the host loop (one slab, libraries that export last_nshift and last_ntilde: the oracle).
    `bodies`: (x, y, m, rsm, indirect) for set_bodies before init_physics (None: the star alone, as create leaves it).
    `forced_dts`: the host loop steps with these lengths instead of the CFL step's (_step_forced); `cfl_dts` then
    receives what the CFL reduction of every step returned (before the step policy).  `sentinel_map`: applied to the
    Q+ / Q- sentinel of every slab (tests/symmetries.py: a transformed run starts from the transformed sentinel)."""
    if noise:
        rng = np.random.default_rng(7)
        fields = [f * (1.0 + noise * rng.standard_normal(f.shape)) for f in fields]
    ctxs = []
    for rank in range(nslabs):
        dd = d0.copy()
        dd.rank, dd.nranks = rank, nslabs
        s = lib.split_domain(dd)
        sub = tuple(np.ascontiguousarray(f[s.imin:s.imin + s.nr + (1 if k == 1 else 0)]) for k, f in enumerate(fields))
        ctx = driver.make_context(lib, dd, fields=sub, radii=radii, bodies=bodies)
        if d0.eos == B.EOS_IDEAL:
            # (this replaces the Q- that init_physics computed for the cooling cases: with Q+ = Q- the first step's
            # thermal CFL term is 0 on both sides, so the init-time Q- is not what these states compare)
            q = sentinel((s.nr, d0.nphi))
            if sentinel_map is not None:
                q = np.ascontiguousarray(sentinel_map(q))
            ctx.upload(B.F_QPLUS, q)
            ctx.upload(B.F_QMINUS, q)
        if chunks is not None and lib.has("set_transport_chunks"):
            ctx.set_transport_chunks(chunks)
        if source_chunks is not None and lib.has("set_source_chunks"):
            ctx.set_source_chunks(source_chunks)
        ctxs.append(ctx)
    S = driver.SlabSet(ctxs)
    S.dt_scale = dt_scale
    S.prepare()
    prof, fell = {}, []
    if profile:
        ctxs[0].profile_start()
    if loop == "host":
        dts = []
        for n in range(nsteps):
            if forced_dts is None:
                dts.append(S.step())
            else:
                own = _step_forced(S, forced_dts[n])
                dts.append(forced_dts[n])
                if cfl_dts is not None:
                    cfl_dts.append(own)
            if profile and lib.has("get_option"):
                fell.append(ctxs[0].get_option("transport_fell_back"))
            if shifts is not None:
                assert nslabs == 1
                shifts.append((ctxs[0].last_nshift().astype(np.int64), ctxs[0].last_ntilde()))
    else:
        assert forced_dts is None, "the device loop takes its own step lengths"
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


def errors(d0, radii, a, b, time):
    scales = cell_scales(d0, radii, b, time)
    return {k: cell_err(a[k], b[k], scales[k]) for k in b}


def noise_growth(oracle, d0, radii, fields, nsteps, loop="host", dt_scale=1.0, b=None, **run):
    """By how much the oracle amplifies cell-wise 1e-15 relative noise on its own input over `nsteps`, in the
    measure of `errors` (what _tolerance measures when a comparison misses the plain bar).  `run`: further keyword
    arguments of run_state (bodies, forced_dts: the same step lengths for the noisy run)."""
    noise = 1.0e-15
    if b is None:
        b = run_state(oracle, d0, radii, fields, 1, nsteps, loop, dt_scale=dt_scale, **run)[0]
    b2, dts, _, _ = run_state(oracle, d0, radii, fields, 1, nsteps, loop, noise=noise, dt_scale=dt_scale, **run)
    return max(e for e, _ in errors(d0, radii, b2, b, sum(dts)).values()) / noise


def assert_paths(name, opt, prof, fell):
    ran = lambda names: sum(prof.get(n, (0, 0))[1] for n in names)
    if opt["src"] == "march":
        assert ran(SOURCE_MARCH) > 0, f"{name}: no marching source kernel ran: {sorted(prof)}"
    else:
        assert ran(SOURCE_MARCH) == 0, f"{name}: a marching source kernel ran on narrow rings: {sorted(prof)}"
        for k in SOURCE_FUSED:   # "fused": rings narrower than the march takes -- the three out-of-place kernels
            assert ran((k,)) > 0, f"{name}: {k} did not run: {sorted(prof)}"
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


def compare(name, d0, radii, fields, nslabs, nsteps, loop, product, oracle, opt, tag="rough", run=None, keep=None):
    """Product against oracle from one state; asserts the paths, the dt history and every grid cell-wise; returns
    (worst cell-wise error, bar used).  Of `opt` it reads dt_scale, chunks and source_chunks (explicit chunk lengths for
    the product's set_transport_chunks / set_source_chunks) and what assert_paths reads (src, tr, cfl).  `run`: further keyword arguments of run_state for both libraries (bodies,
    forced_dts, sentinel_map); with forced_dts the dt history compared is what the CFL call of every step returned.
    `keep`: a dictionary that receives both results ("a": the product's grids, "b": the oracle's, "dta", "dtb")."""
    sc = opt.get("dt_scale", 1.0)
    chunks = opt.get("chunks")
    run = dict(run or {})
    cfa, cfb = [], []
    b, dtb, _, _ = run_state(oracle, d0, radii, fields, 1, nsteps, loop, dt_scale=sc, cfl_dts=cfb, **run)
    a, dta, prof, fell = run_state(product, d0, radii, fields, nslabs, nsteps, loop, profile=True, dt_scale=sc, chunks=chunks,
                                   source_chunks=opt.get("source_chunks"), cfl_dts=cfa, **run)
    if run.get("forced_dts") is not None:
        dta, dtb = cfa, cfb
    if keep is not None:
        keep.update(a=a, b=b, dta=dta, dtb=dtb)
    assert_paths(name, opt, prof, fell)
    assert all(np.isfinite(v).all() for v in b.values()), f"{name}: the oracle left the finite range"
    for q in ("qplus", "qminus"):
        if q in b:
            for ring in (0, b[q].shape[0] - 1):
                bad = np.flatnonzero(a[q][ring] != b[q][ring])
                assert bad.size == 0, (f"{name} ({loop}, {nsteps} steps): {q} ring {ring} differs from the oracle's in "
                                       f"{bad.size} cells, e.g. column {bad[0]}: {a[q][ring][bad[0]]!r} vs "
                                       f"{b[q][ring][bad[0]]!r}")
    time = sum(run["forced_dts"][:nsteps]) if run.get("forced_dts") is not None else sum(dtb)   # (the device loop's [clock time])
    errs = errors(d0, radii, a, b, time)
    dterr = max(abs(x - y) / y for x, y in zip(dta, dtb))
    worst = max(e for e, _ in errs.values())
    tol, growth = TOL, 1.0
    if worst > TOL:
        fields_cmp = list(b)
        tol, growth = _tolerance(lambda noise: run_state(oracle, d0, radii, fields, 1, nsteps, loop, noise=noise, dt_scale=sc, **run)[0], b,
                                 fields_cmp, worst,
                                 measure=lambda x, y, k: cell_err(x, y, cell_scales(d0, radii, b, time)[k])[0])
        print(f"[{tag}] {name} {loop} {nsteps} steps: growth-based bar {tol:.1e} (growth {growth:.1e})")
    assert dterr <= TOL_DT, f"{name} ({loop}, {nsteps} steps): dt differs by {dterr:.3e}"
    for k, (e, (i, j)) in errs.items():
        assert e <= tol, (f"{name} ({loop}, {nsteps} steps): {k} at ring {i}, column {j}: {e:.3e} > {tol:.1e} "
                          f"(HIP {a[k][i, j]!r}, oracle {b[k][i, j]!r}, growth {growth:.1e})")
    return worst, tol
