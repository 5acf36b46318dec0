"""Shared helpers of the parity tests."""
from __future__ import annotations

import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver


@functools.lru_cache(maxsize=None)
def kernel_resource_usage() -> dict:
    """{mangled kernel name: {remark: value}} of fcpt_kernels.hip cross-compiled for gfx950 with
    -Rpass-analysis=kernel-resource-usage ("VGPRs", "TotalSGPRs", "Occupancy [waves/SIMD]", "ScratchSize [bytes/lane]",
    "VGPRs Spill", ...).  One compilation per process (a result is cached, a skip is not); skips the calling test where
    hipcc is absent."""
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
    return usage


def rel_err(a: np.ndarray, b: np.ndarray) -> float:
    """max|a-b| / max|b|: v_r has zeros, a pointwise relative error is meaningless
    (SURVEY.md section 8(c))."""
    den = np.abs(b).max()
    return float(np.abs(a - b).max() / (den if den > 0 else 1.0))


def cell_err(a: np.ndarray, b: np.ndarray, scale) -> tuple:
    """max |a-b| / max(|b|, scale) over all cells, and the (ring, column) where it is reached: the measure that sees
    a wrong cell near the floor or where v_r crosses zero, which `rel_err` divides by the field's maximum.  `scale`
    is a number or an array that broadcasts against `b` (a per-cell or per-ring floor of the denominator).  Cells
    where both the denominator and the difference vanish count as exact; a difference over a zero denominator as
    infinite."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    diff = np.abs(a - b)
    den = np.maximum(np.abs(b), np.broadcast_to(np.asarray(scale, dtype=np.float64), b.shape))
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.where(den > 0, diff / np.where(den > 0, den, 1.0), np.where(diff == 0, 0.0, np.inf))
    err = np.where(np.isnan(a) | np.isnan(b), np.inf, err)
    k = int(np.argmax(err))
    pos = np.unravel_index(k, err.shape) if err.ndim == 2 else (k, 0)
    return float(err.flat[k]), (int(pos[0]), int(pos[1]))


def _rmed(d, radii, nrows):
    """Cell-centre radii of the global grid (midpoints of the interfaces: a scale, not the reference's Rmed)."""
    ri = np.asarray(radii[:nrows + 1], dtype=np.float64)
    return 0.5 * (ri[:-1] + ri[1:])


def cell_scales(d, radii, ref, time=None) -> dict:
    """Per-cell floors of the denominator of `cell_err` for the global grids of `ref` (the oracle's state):
    Sigma: the density floor sigma_floor sigma0; e: e_min(Sigma) of the cell; v_r and v_phi: the local sound speed
    (h v_K(r) for the locally isothermal EOS, sqrt(gamma (gamma-1) e / Sigma) of `ref` for the ideal one; an
    interface takes the smaller of its two cells); Q+ and Q-: 1e-7 of the ring's max |Q| (beta cooling towards the
    floor is (e - e_min) Omega / beta: at a cell clamped to e_min one ulp of e is all there is -- 6.8e-27 against 0
    in a ring whose largest |Q-| is 6e-9, which needs a scale of 1.1e-8 of the ring's max to pass at 1e-10);
    MASSFLOW (the mass through a face, summed over the steps: dt dphi R_inf Sigma* v_r, TransportEuler.cpp:609-616):
    what the face would carry in `time` at the local scale of v_r, with the smaller Sigma of its two cells."""
    sigma = ref["sigma"]
    nr = sigma.shape[0]
    out = {"sigma": d.sigma_floor * d.sigma0}
    if d.eos == B.EOS_IDEAL:
        gam = d.adiabatic_index
        out["energy"] = d.minimum_temperature * sigma / d.mu * d.Rgas / (gam - 1.0)
        cs = np.sqrt(np.maximum(gam * (gam - 1.0) * ref["energy"] / sigma, 0.0))
    else:
        r = _rmed(d, radii, nr)
        vk = np.sqrt(d.G * d.hydro_center_mass / r)
        cs = np.broadcast_to((d.aspect_ratio * r ** d.flaring_index * vk)[:, None], sigma.shape)
    out["vazi"] = cs
    iface = np.vstack([cs[:1], np.minimum(cs[:-1], cs[1:]), cs[-1:]])
    out["vrad"] = iface
    for q in ("qplus", "qminus"):
        if q in ref:
            out[q] = 1e-7 * np.abs(ref[q]).max(axis=1, keepdims=True)
    if "massflow" in ref:
        assert time is not None, "the MASSFLOW scale needs the time the flow was summed over"
        sf = np.vstack([sigma[:1], np.minimum(sigma[:-1], sigma[1:]), sigma[-1:]])
        rinf = np.asarray(radii[:nr + 1], dtype=np.float64)[:, None]
        out["massflow"] = time * (2 * np.pi / sigma.shape[1]) * rinf * sf * iface
    return out


GRID_IDS = {"sigma": B.F_SIGMA, "vrad": B.F_VRAD, "vazi": B.F_VAZI, "energy": B.F_ENERGY, "qplus": B.F_QPLUS,
            "qminus": B.F_QMINUS, "massflow": B.F_MASSFLOW, "temperature": B.F_TEMPERATURE}


def gather_grids(slabset, names) -> dict:
    """driver.SlabSet.gather for any grid, the heating and cooling rates included: the global grid of each name
    (a key of GRID_IDS or a field id) with the slabs' overlap rings stripped (write2D, polargrid.cpp:135-180)."""
    out = {}
    for name in names:
        f = GRID_IDS[name] if isinstance(name, str) else int(name)
        parts = []
        for c in slabset.ctxs:
            a = c.download(f)
            s = c.split
            lo = 0 if s.is_first else B.OVERLAP
            hi = a.shape[0] - (0 if s.is_last else B.OVERLAP)
            if f in B.VECTOR_FIELDS and not s.is_last:
                hi -= 1
            parts.append(a[lo:hi])
        out[name] = np.concatenate(parts, axis=0)
    return out


FUZZ_TOL = 1e-10
GROWTH_CAP = 1.0e4   # widened bar at most 1e-13 x 1e4 = 1e-9; a more violent draw is compared over fewer steps instead


def _tolerance(oracle_run, b, fields, worst, measure=rel_err):
    """1e-10, unless the draw is an unstable flow that amplifies rounding by orders of magnitude per step: then
    what the oracle does to cell-wise 1e-15 relative noise on its own input over the same steps (measured only
    when the plain bar is missed), never more than GROWTH_CAP.  `measure(a, b, field) -> float` defaults to
    rel_err of the two grids."""
    if worst <= FUZZ_TOL:
        return FUZZ_TOL, 1.0
    noise = 1.0e-15
    b2 = oracle_run(noise)
    if measure is rel_err:
        growth = max(rel_err(b2[k], b[k]) for k in fields) / noise
    else:
        growth = max(measure(b2[k], b[k], k) for k in fields) / noise
    # the two paths differ by a few 1e-14 before any amplification; one noise realisation
    return max(FUZZ_TOL, 1.0e-13 * min(growth, GROWTH_CAP)), growth


def perturb(fields, d, amp=1e-3):
    """Deterministic non-axisymmetric perturbation 1 + amp sin(3 phi) cos(5 ln r) of Sigma
    (and energy), so limiters, shifts and azimuthal fluxes are exercised
    (SURVEY.md section 8(d))."""
    sigma, vrad, vazi, energy = [f.copy() for f in fields]
    nr, nphi = sigma.shape
    phi = (np.arange(nphi) + 0.5) * 2 * np.pi / nphi
    r = np.geomspace(max(d.rmin, 1e-3), d.rmax, nr)
    f = 1.0 + amp * np.sin(3 * phi)[None, :] * np.cos(5 * np.log(r))[:, None]
    sigma *= f
    energy *= f
    vazi = vazi * (1.0 + 0.1 * amp * np.cos(2 * phi)[None, :])
    return sigma, vrad, vazi, energy


class Runs(list):
    """The [(state, dts), ...] of run_pair, with the descriptor of the global grid and its radii (for cell_scales)."""

    def __init__(self, items=(), desc=None, radii=None):
        super().__init__(items)
        self.desc, self.radii = desc, radii


def check_cells(outs, fields, tol):
    """cell_err of every field of a run_pair result (first against second) at `tol`; asserts and returns the
    errors with their worst cells."""
    (a, _), (b, _) = outs[0], outs[1]
    scales = cell_scales(outs.desc, outs.radii, b)
    errs = {k: cell_err(a[k], b[k], scales[k]) for k in fields}
    for k, (e, (i, j)) in errs.items():
        assert e <= tol, f"{k}: cell-wise {e:.3e} > {tol} at ring {i}, column {j} ({a[k][i, j]!r} vs {b[k][i, j]!r})"
    return errs


def run_pair(lib_a, lib_b, d, nsteps, bodies=None, amp=1e-3, snap=False, nslabs=(1, 1), dt_scale=1.0, noise=0.0,
             irradiation=None, transport_chunks=None, source_chunks=None):
    """Advance the same initial state `nsteps` with two libraries; returns the two global
    states and the two dt histories (a Runs list: with .desc and .radii of the global grid)."""
    outs = Runs()
    dfull = d.copy()
    dfull.rank, dfull.nranks = 0, 1
    radii = lib_a.radii(dfull)
    d0 = dfull.copy()
    fields = lib_a.initial_fields(d0, radii)   # d0.sigma0 possibly rescaled
    outs.desc, outs.radii = d0, radii
    if amp:
        fields = perturb(fields, d0, amp)
    if noise:   # cell-wise relative noise (seeded): how fast does this flow amplify rounding-sized differences?
        rng = np.random.default_rng(7)
        fields = tuple(f * (1.0 + noise * rng.standard_normal(f.shape)) for f in fields)
    for L, ns in zip((lib_a, lib_b), nslabs):
        if ns == 0:   # only one library wanted
            outs.append(None)
            continue
        ctxs = []
        for rank in range(ns):
            dd = d0.copy()
            dd.rank, dd.nranks = rank, ns
            s = L.split_domain(dd)
            sl = slice(s.imin, s.imin + s.nr)
            sub = (fields[0][sl], fields[1][s.imin:s.imin + s.nr + 1], fields[2][sl], fields[3][sl])
            sub = tuple(np.ascontiguousarray(x) for x in sub)
            ctxs.append(driver.make_context(L, dd, fields=sub, radii=radii, bodies=bodies, irradiation=irradiation))
            if transport_chunks is not None and L.has("set_transport_chunks"):   # (the product's marching kernel; the oracle has no chunks)
                ctxs[-1].set_transport_chunks(transport_chunks)
            if source_chunks is not None and L.has("set_source_chunks"):   # (likewise the marching source kernels: the same list for every slab)
                ctxs[-1].set_source_chunks(source_chunks)
        S = driver.SlabSet(ctxs)
        S.dt_scale = dt_scale
        S.prepare()
        dts = S.run(nsteps, snap=snap)
        outs.append((S.gather(), dts))
        for c in ctxs:
            c.close()
    return outs
