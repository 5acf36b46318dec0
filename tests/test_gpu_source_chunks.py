"""The chunk seams of the marching source kernels (kernels/source_march.h), for every instance of them.

A wavefront of k_source_march / _adi / _adi_wide / _adi_acc marches one 59-column segment over a chunk of rings
[k0, k1): it pre-rolls from ring k0 - 3, applies the pre-transport boundary call itself on the edge chunks and may fold
the CFL reduction.  It learns [k0, k1) either from equal chunks of source_rows rings or from a per-wavefront table --
and the built-in choice only takes the table on grids of benchmark size.  fcpt_set_source_chunks puts an explicit,
ragged table under grids of test size: unequal chunks, 3-ring edge chunks (the neighbour's pre-roll then starts on the
ghost ring the folded boundary call rewrites in place), idle padding entries, blockIdx-indexed dispatch.  Every ring of
a segment is computed by exactly one wavefront from the same operands, so ANY seams give the bits of equal chunks."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver, setups
from tests.util import Runs, check_cells, perturb, rel_err, run_pair

pytestmark = pytest.mark.gpu
TOL = 1e-10   # the project's bar against the oracle (tests/test_gpu_parity.py)


def _check(outs, fields, tol=TOL):
    (a, dta), (b, dtb) = outs
    assert np.allclose(dta, dtb, rtol=1e-9, atol=0), "time-step history differs"
    for k in fields:
        e = rel_err(a[k], b[k])
        assert e <= tol, f"{k}: {e:.3e} > {tol}"
    assert isinstance(outs, Runs) and outs.desc is not None
    check_cells(outs, fields, tol)


def _segments(nphi):
    return -(-nphi // 59)


def _check_table(ctx, edges_of_three):
    """The table in force: every (segment, row of v_r) exactly once, whole workgroups, idle entries where the live ones
    do not fill the last workgroup; -> number of chunks."""
    tab = ctx.source_chunks()
    segs, rows = _segments(ctx.nphi), ctx.nr + 1
    assert len(tab) > 0 and len(tab) % 4 == 0
    live = tab[tab[:, 2] > tab[:, 1]]
    assert len(live) % segs == 0
    cover = np.zeros((segs, rows), dtype=np.int32)
    for sg, k0, k1 in live:
        assert 0 <= sg < segs and 0 <= k0 < k1 <= rows and k1 - k0 >= 3
        cover[sg, k0:k1] += 1
    assert (cover == 1).all()
    chunks = len(live) // segs
    if (segs * chunks) % 4 != 0:
        assert len(live) < len(tab), "no idle entry although the live ones do not fill whole workgroups"
    assert len(tab) - len(live) < 4
    for sg in range(segs):
        mine = live[live[:, 0] == sg]
        assert mine[0, 1] == 0 and mine[-1, 2] == rows
        if edges_of_three:
            assert mine[0, 2] - mine[0, 1] == 3 and mine[-1, 2] - mine[-1, 1] == 3
    return chunks


def _bc(d, inner, outer):
    for side, (vrad, vaz, sig) in enumerate((inner, outer)):
        d.bc_vrad[side], d.bc_vaz[side] = vrad, vaz
        d.bc_sigma[side] = d.bc_energy[side] = sig


# (inner, outer) descriptors of (v_r, v_phi, Sigma and e): every kind of every variable at both edges, inner != outer
_VRAD = (B.BC_ZEROGRADIENT, B.BC_REFERENCE, B.BC_REFLECTING, B.BC_OUTFLOW, B.BC_KEPLERIAN)
_VAZ = (B.BC_ZEROGRADIENT, B.BC_REFERENCE, B.BC_KEPLERIAN, B.BC_ZEROSHEAR)
_SIG = (B.BC_ZEROGRADIENT, B.BC_REFERENCE)
BC_MATRIX = [((_VRAD[k % 5], _VAZ[k % 4], _SIG[k % 2]), (_VRAD[(k + 1) % 5], _VAZ[(k + 1) % 4], _SIG[(k + 1) % 2]))
             for k in range(6)]
for _v, _kinds in enumerate((_VRAD, _VAZ, _SIG)):
    for _side in (0, 1):
        assert {pair[_side][_v] for pair in BC_MATRIX} == set(_kinds)
assert all(i != o for pair in BC_MATRIX for i, o in zip(*pair))


def _case(product, case):
    """-> dict(d, bodies, irradiation, lengths, device_loop, kernel, dt_scale, nslabs, edges, options)"""
    c = dict(irradiation=None, device_loop=False, dt_scale=1.0, nslabs=1, edges=False, options={})
    planet = lambda d: setups.jupiter_bodies(d)
    if case == "iso_tw":
        d = setups.planet_disk(product, 44, 320)
        c.update(lengths=[3, 9, 4, 17, 3, 6, 3], device_loop=True, edges=True)
    elif case == "iso_sn_ragged_segment":
        d = setups.planet_disk(product, 45, 130)     # 3 segments, the last one stores 130 - 118 = 12 columns
        d.artificial_viscosity = B.ARTVISC_SN
        c.update(lengths=[5, 3, 30, 8])
    elif case == "iso_noav_constnu_one_chunk":
        d = setups.planet_disk(product, 40, 128)
        d.artificial_viscosity = B.ARTVISC_NONE
        d.viscous_alpha, d.constant_viscosity = 0.0, 1e-5
        c.update(lengths=[64])
    elif case == "iso_stab1":
        d = setups.planet_disk(product, 48, 192)
        d.viscous_alpha, d.constant_viscosity, d.stabilize_viscosity = 0.0, 1.0e-2, 1
        c.update(lengths=[3, 3, 3, 11], dt_scale=3.0)
    elif case == "iso_stab2_leapfrog":
        d = setups.planet_disk(product, 48, 192)
        d.stabilize_viscosity, d.radial_viscosity_factor, d.integrator = 2, 2.5, B.INTEGRATOR_LEAPFROG
        c.update(lengths=[7, 3, 20])
    elif case == "iso_acc_cubic":
        d = setups.planet_disk(product, 48, 288)
        d.body_force_from_potential = 0
        x, y, m = planet(d)   # Klahr & Kley smoothing inside the Hill radius + an indirect term
        c.update(lengths=[4, 4, 25, 3], device_loop=True, bodies=(x, y, m, [0.0, (m[1] / 3.0) ** (1.0 / 3.0)], (1.0e-4, -2.0e-4)))
    elif case == "adi_inline_potential":
        d = setups.planet_disk(product, 44, 320, adiabatic=True)
        c.update(lengths=[3, 10, 3, 3, 20, 3, 3], device_loop=True, edges=True)
    elif case == "adi_sn_leapfrog":
        d = setups.planet_disk(product, 48, 288, adiabatic=True)
        d.artificial_viscosity, d.integrator = B.ARTVISC_SN, B.INTEGRATOR_LEAPFROG
        c.update(lengths=[6, 13, 3])
    elif case == "adi_cool_lin_irradiated":
        d = setups.planet_disk(product, 44, 320, adiabatic=True)
        d.cooling_surface, d.opacity = 1, B.OPACITY_LIN
        x, y, m = planet(d)
        c.update(lengths=[3, 5, 8, 13], device_loop=True, bodies=(x, y, m, [0.0, 0.05]),
                 irradiation=([5800.0 / setups.TEMP0_K, 1500.0 / setups.TEMP0_K], [4.65e-3, 4.7e-4], [0.0, 0.05]))
    elif case == "adi_stab1_beta":
        d = setups.planet_disk(product, 48, 192, adiabatic=True)
        d.viscous_alpha, d.constant_viscosity, d.stabilize_viscosity = 0.0, 1.0e-2, 1
        d.cooling_beta, d.cooling_beta_value, d.cooling_beta_reference = 1, 10.0, B.BETAREF_REFERENCE
        c.update(lengths=[9, 3, 3], dt_scale=3.0)
    elif case == "adi_acc_cool":
        d = setups.planet_disk(product, 40, 256, adiabatic=True)
        d.body_force_from_potential = 0
        d.cooling_surface, d.opacity, d.kappa_const = 1, B.OPACITY_CONST, 1.0e4
        c.update(lengths=[4, 30, 3])
    elif case.startswith("bc_matrix"):
        _, _, eos, k = case.split("_")
        d = setups.planet_disk(product, 40, 263, adiabatic=eos == "adi")
        _bc(d, *BC_MATRIX[int(k)])
        c.update(lengths=[3, 3, 40], device_loop=True, options={"bc_in_cfl": 2, "graph_steps": 0})
    elif case == "three_slabs":
        d = setups.planet_disk(product, 90, 320)     # the middle slab folds neither side, the outer two one side each
        c.update(lengths=[3, 4, 3, 50], nslabs=3)
    else:
        raise AssertionError(case)
    c.setdefault("bodies", planet(d))
    adi = d.eos == B.EOS_IDEAL
    wide = d.stabilize_viscosity or d.cooling_surface or d.cooling_beta
    c["kernel"] = ("k_source_march_adi_acc" if not d.body_force_from_potential else
                   "k_source_march_adi_wide" if wide else "k_source_march_adi") if adi else "k_source_march"
    c["d"] = d
    return c


def _slabs(product, c, fields, radii):
    """The contexts of the case's slabs on the same uploaded state (as run_pair cuts them)."""
    ctxs = []
    for rank in range(c["nslabs"]):
        dd = c["d"].copy()
        dd.rank, dd.nranks = rank, c["nslabs"]
        s = product.split_domain(dd)
        sl = slice(s.imin, s.imin + s.nr)
        sub = tuple(np.ascontiguousarray(x) for x in (fields[0][sl], fields[1][s.imin:s.imin + s.nr + 1], fields[2][sl], fields[3][sl]))
        ctx = driver.make_context(product, dd, fields=sub, radii=radii, bodies=c["bodies"], irradiation=c["irradiation"])
        for name, value in c["options"].items():
            ctx.set_option(name, value)
        ctxs.append(ctx)
    return ctxs


def _snapshot(ctxs, d):
    """Every state grid of every slab (ideal EOS: and Q+, Q-; StabilizeViscosity: and the correction factors), the clocks."""
    out = {}
    for r, ctx in enumerate(ctxs):
        for k, v in ctx.state().items():
            out[f"{k}[{r}]"] = v
        extra = []
        if d.eos == B.EOS_IDEAL:
            extra += [("qplus", B.F_QPLUS), ("qminus", B.F_QMINUS)]
        if d.stabilize_viscosity:
            extra += [("cfac_phi", B.F_VISC_CFAC_PHI), ("cfac_r", B.F_VISC_CFAC_R)]
        for k, f in extra:
            out[f"{k}[{r}]"] = ctx.download(f)
        clk = ctx.clock
        out[f"clock[{r}]"] = np.array([clk.time, clk.last_dt, float(clk.n_hydro_iter)])
    return out


def _same_bits(a, b, when):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), f"{k} differs {when}"


CASES = (["iso_tw", "iso_sn_ragged_segment", "iso_noav_constnu_one_chunk", "iso_stab1", "iso_stab2_leapfrog", "iso_acc_cubic",
          "adi_inline_potential", "adi_sn_leapfrog", "adi_cool_lin_irradiated", "adi_stab1_beta", "adi_acc_cool"] +
         [f"bc_matrix_{eos}_{k}" for eos in ("iso", "adi") for k in range(len(BC_MATRIX))] + ["three_slabs"])


@pytest.mark.parametrize("case", CASES)
def test_source_chunk_seams_never_change_a_result(product, oracle, case):
    """Two product runs from the same uploaded state, one on the built-in equal chunks and one on an explicit ragged
    table: 12 steps (the march kernel of the case profiled: one launch per step, two under leapfrog -- a fallback to the
    out-of-place kernels cannot pass), bits compared; then the explicit context returns to the built-in choice and both run 4
    more, bits compared again.  State grids, Q+ and Q- (ideal EOS), the correction factors (StabilizeViscosity), and
    (time, last_dt, n_hydro_iter).  The device-loop cases take their first 4 steps profiled (plain launches) and the
    other 8 in one call that may replay a captured graph.  And the explicit run against the oracle at 1e-10."""
    c = _case(product, case)
    d = c["d"]
    d0 = d.copy()
    d0.rank, d0.nranks = 0, 1
    radii = product.radii(d0)
    fields = perturb(product.initial_fields(d0, radii), d0, 1e-3)
    frog = d.integrator == B.INTEGRATOR_LEAPFROG
    kid = product.kernel_names().index(c["kernel"])
    snaps = []
    for explicit in (False, True):
        ctxs = _slabs(product, c, fields, radii)
        for ctx in ctxs:
            if explicit:
                ctx.set_source_chunks(c["lengths"])
                _check_table(ctx, c["edges"])
            else:
                assert len(ctx.source_chunks()) == 0
        S = driver.SlabSet(ctxs)
        S.dt_scale = c["dt_scale"]
        S.prepare()
        profiled = 4 if c["device_loop"] else 12
        for ctx in ctxs:
            ctx.profile_start([kid], max_launches=64)
        if c["device_loop"]:
            assert ctxs[0].run_steps(4) == 4
        else:
            S.run(12)
        for ctx in ctxs:
            prof = ctx.profile_stop()
            assert c["kernel"] in prof and prof[c["kernel"]][1] == profiled * (2 if frog else 1), (explicit, prof)
        if c["device_loop"]:
            assert ctxs[0].run_steps(8) == 8
        after12 = _snapshot(ctxs, d)
        if explicit:
            for ctx in ctxs:
                ctx.set_source_chunks([])
                assert len(ctx.source_chunks()) == 0
        if c["device_loop"]:
            assert ctxs[0].run_steps(4) == 4
        else:
            S.run(4)
        snaps.append((after12, _snapshot(ctxs, d)))
        for ctx in ctxs:
            ctx.close()
    _same_bits(snaps[0][0], snaps[1][0], "after 12 steps on the explicit table")
    _same_bits(snaps[0][1], snaps[1][1], "4 steps after the return to the built-in chunks")
    assert int(snaps[1][1]["clock[0]"][2]) == 16
    outs = run_pair(product, oracle, d, 12, bodies=c["bodies"], irradiation=c["irradiation"], dt_scale=c["dt_scale"],
                    nslabs=(c["nslabs"], 1), source_chunks=c["lengths"])
    _check(outs, ("sigma", "vrad", "vazi") + (("energy",) if d.eos == B.EOS_IDEAL else ()))


def test_source_chunks_set_between_graph_replays(product, oracle):
    """40 x 256 with hipGraph replay: 21 steps, the list set, 12 more.  The cycle captured for equal chunks must not be
    replayed for the table (and the table's cycle really is replayed): the bits of the same calls without a graph, and of
    equal chunks throughout."""
    d = setups.planet_disk(product, 40, 256)
    bodies = setups.jupiter_bodies(d)
    lengths = [3, 3, 3, 5]
    out = []
    for graph, explicit in ((1, True), (0, True), (0, False)):
        ctx = driver.make_context(product, d, bodies=bodies)
        ctx.set_option("graph_steps", graph)
        S = driver.SlabSet([ctx])
        S.prepare()
        assert ctx.run_steps(21) == 21
        before = ctx.get_option("graph_replays")
        if explicit:
            ctx.set_source_chunks(lengths)
            _check_table(ctx, False)
        assert ctx.run_steps(12) == 12
        if graph:
            assert before > 0 and ctx.get_option("graph_replays") > before
        else:
            assert ctx.get_option("graph_replays") == 0
        out.append(_snapshot([ctx], d))
        ctx.close()
    _same_bits(out[0], out[1], "between graph replay and plain launches")
    _same_bits(out[1], out[2], "between the explicit table and equal chunks")
    _check(run_pair(product, oracle, d, 12, bodies=bodies, source_chunks=lengths), ("sigma", "vrad", "vazi"))


# ---- equal chunks of any length -------------------------------------------------------------------------------------
ROWS = (1, 2, 3, 5, 14, 22, 43, 45, 64)
NR_EQ, NPHI_EQ = 44, 320


def _last_chunk(rows):
    """(chunks, rings of the first chunk, rings of the last) of equal chunks of `rows` rings over the nr + 1 rows of v_r"""
    total = NR_EQ + 1
    chunks = -(-total // rows)
    return chunks, min(rows, total), total - (chunks - 1) * rows


assert {_last_chunk(r)[2] for r in ROWS} >= {1, 2} and any(_last_chunk(r)[0] == 1 for r in ROWS)
assert _last_chunk(22)[2] == 1 and _last_chunk(43)[2] == 2 and _last_chunk(45)[0] == 1 and _last_chunk(64)[0] == 1

_BUILT_IN = {}


def _equal_chunk_run(product, adiabatic, rows):
    """10 run_steps (1, then 9 with the boundary kernel and the march profiled) -> (snapshot, k_boundary launches, march launches)"""
    d = setups.planet_disk(product, NR_EQ, NPHI_EQ, adiabatic=adiabatic)
    ctx = driver.make_context(product, d, bodies=setups.jupiter_bodies(d))
    if rows is not None:
        ctx.set_option("source_rows", rows)
    assert len(ctx.source_chunks()) == 0
    S = driver.SlabSet([ctx])
    S.prepare()
    # (the first step after an upload never folds the boundary call: the ghost rings are not yet a boundary call's)
    assert ctx.run_steps(1) == 1
    names = product.kernel_names()
    march = "k_source_march_adi" if adiabatic else "k_source_march"
    ctx.profile_start([names.index("k_boundary"), names.index(march)], max_launches=64)
    assert ctx.run_steps(9) == 9
    prof = ctx.profile_stop()
    snap = _snapshot([ctx], d)
    ctx.close()
    return snap, prof.get("k_boundary", (0.0, 0))[1], prof.get(march, (0.0, 0))[1]


@pytest.mark.parametrize("adiabatic", [False, True], ids=["iso", "adi"])
@pytest.mark.parametrize("rows", ROWS)
def test_equal_chunks_of_any_length(product, rows, adiabatic):
    """Option source_rows from a single ring per chunk to a single chunk: the bits of the built-in choice over 10
    run_steps.  Where the first or the last chunk holds fewer than 3 rings the launcher must decline to fold the
    pre-transport boundary call into the march (one more k_boundary launch per step); where both hold 3 it must fold."""
    if adiabatic not in _BUILT_IN:
        _BUILT_IN[adiabatic] = _equal_chunk_run(product, adiabatic, None)
    ref, ref_boundary, ref_march = _BUILT_IN[adiabatic]
    assert ref_march == 9
    snap, boundary, march = _equal_chunk_run(product, adiabatic, rows)
    _, first, last = _last_chunk(rows)
    declined = first < 3 or last < 3
    print(f"source_rows {rows}: first chunk {first}, last {last}, k_boundary {boundary} (built-in {ref_boundary}), march {march}")
    assert march == 9
    assert boundary == ref_boundary + (9 if declined else 0)
    _same_bits(ref, snap, f"with source_rows = {rows}")


def test_source_chunk_argument_errors(product):
    d = setups.planet_disk(product, 44, 320)
    ctx = driver.make_context(product, d, bodies=setups.jupiter_bodies(d))
    try:
        for bad in ([2], [5, 2, 9], [7, 3, 0], [-1]):
            with pytest.raises(B.FcptError, match="FCPT_EINVAL"):
                ctx.set_source_chunks(bad)
            assert len(ctx.source_chunks()) == 0
        ctx.set_source_chunks([5, 3, 17, 4])
        assert _check_table(ctx, False) == 8          # 5 3 17 4 and four more of 4 rings: the last entry repeats
        with pytest.raises(B.FcptError, match="FCPT_EINVAL"):
            ctx.set_source_chunks([4, 2])             # a refused list leaves the one in force alone
        assert _check_table(ctx, False) == 8
        ctx.set_source_chunks([])
        assert len(ctx.source_chunks()) == 0
        ctx.set_source_chunks([5, 3, 17, 4])
        table = ctx.source_chunks()
        ctx.set_option("source_rows", 8)              # equal chunks win over the list ...
        assert len(ctx.source_chunks()) == 0
        ctx.set_option("source_graded", 0)
        ctx.set_option("source_rows", -1)             # ... which is back in force afterwards, whatever source_graded says
        assert np.array_equal(ctx.source_chunks(), table)
        S = driver.SlabSet([ctx])
        S.prepare()
        dt = S.calculate_timestep()
        ctx.step(dt)
        with pytest.raises(B.FcptError, match="FCPT_EINVAL"):
            ctx.set_source_chunks([6])
        ctx.post(dt)
        assert np.array_equal(ctx.source_chunks(), table)
        ctx.set_source_chunks([6])
        assert _check_table(ctx, False) == 8          # 7 x 6 and the 3 rows left
    finally:
        ctx.close()
