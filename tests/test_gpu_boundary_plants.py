"""The ghost-ring conditions and the wave damping of the HIP library against the known answers of
tests/boundary_plants.py, in every kernel that applies them: k_boundary and k_damping on their own
(fcpt_apply_boundary), the edge chunks of the marching source kernels (bc_fold), the next step's CFL launch
(k_cfl_rings_bc, bc_in_cfl), the gated fallback-transport launch (k_theta_march_gated_boundary, gate_in_boundary), the
damping batch of the transport (fused_damping) and the separate damping launches, one and three slabs, Euler and
leapfrog.  tests/test_boundary_plants_oracle.py shows on the CPU that the cases cover every condition on both sides,
that every outflow branch is reached and that the flows amplify rounding by far less than the bars allow.

Every run must (1) leave ghost rings that are `ghost_rings` of its own active rings -- bit for bit for the copying
conditions, the sign of zero included -- (2) agree cell-wise with the oracle to 1e-10, row Nr of v_r included, (3) take
the oracle's time steps to 1e-12, (4) carry the bits of the host loop's state and clock, and (5) have launched the
kernel it was meant to test, or be seen to have declined: the launch counts below follow fcpt_step.hip (a boundary
call rides in the CFL launch or in the gated launch only when it is nothing but the ghost-ring kernel: no separate
damping launches; the fold needs the marching source kernel: rings of 128 cells and more).

A captured graph is replayed only by calls of 8 steps and more, so the two graph modes run GRAPH_NSTEPS = 8 steps
against a host loop and an oracle run of that length (the CPU census bounds the growth over 8 steps as well); all
other runs take 3 steps (4 for GHOST_BINDS_DT).  fcpt_run_steps returns no dt history: its clock after the last step
is held to the host loop's bits, and for GHOST_BINDS_DT the clock after every number of steps.
"""
import numpy as np
import pytest

from fargocpt_amd import binding as B
from tests import boundary_plants as BP
from tests.util import cell_err, cell_scales

pytestmark = pytest.mark.gpu
TOL, TOL_DT = 1e-10, 1e-12
EOS = [False, True]
EOS_IDS = ["iso", "ideal"]
STEP_GRIDS = ((40, 320), (24, 67))
COUNTED = ("k_boundary", "k_damping", "k_cfl_rings_bc", "k_theta_march_gated_boundary", "k_cfl_rings")
CASE_IDS = [c.name for c in BP.CASES]


# ---------------------------------------------------------------------------------------------------------------
# a. direct calls
@pytest.mark.parametrize("ideal", EOS, ids=EOS_IDS)
@pytest.mark.parametrize("case", BP.CASES, ids=CASE_IDS)
def test_direct_calls(product, case, ideal):
    """fcpt_apply_boundary(0, False) and (0.7 tau, True) on the direct-call states: k_boundary and k_damping alone."""
    worst, problems = {}, []
    shapes = [(nr, nphi, 0, 1) for nr, nphi in BP.GRIDS + ((24, 514),)]
    shapes += [(nr, nphi, rank, 3) for nr, nphi in ((24, 67), (40, 320)) for rank in range(3)]
    for nr, nphi, rank, nranks in shapes:
        launches = {}
        bad, w = BP.direct_calls(product, product, case, nr, nphi, ideal, rank, nranks, launches=launches)
        problems += bad
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if launches.get("k_boundary", 0) != 3:
            problems.append(f"{nr}x{nphi} rank {rank}/{nranks}: k_boundary ran {launches.get('k_boundary', 0)} times in three calls")
        if nranks == 1 and (launches.get("k_damping", 0) > 0) != case.damps():
            problems.append(f"{nr}x{nphi}: k_damping ran {launches.get('k_damping', 0)} times, the case damps: {case.damps()}")
    print(f"[gpu boundary plants] direct {case.name} {'ideal' if ideal else 'iso'}: largest deviation in bars {worst}")
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:10])


# ---------------------------------------------------------------------------------------------------------------
# b. every kernel that applies the conditions
def _compare(tag, r, ref, d0, radii, rad, st0, host=None, problems=None):
    """The five assertions of the module docstring but the launch counts, on one run; problems are collected."""
    fields = [k for k in ref.state]
    bad, worst = BP.ghost_mismatch(d0, rad, r.state, st0, fields=fields)
    problems += [f"{tag}: ghost rings: {m}" for m in bad]
    scales = cell_scales(d0, radii, ref.state)
    for k in fields:
        e, (i, j) = cell_err(r.state[k], ref.state[k], scales[k])
        if not e <= TOL:
            problems.append(f"{tag}: {k} differs from the oracle's by {e:.3e} at ring {i}, column {j}")
    if r.dts:
        for n, (x, y) in enumerate(zip(r.dts, ref.dts)):
            if not abs(x - y) <= TOL_DT * y:
                problems.append(f"{tag}: dt of step {n + 1} {x!r} vs the oracle's {y!r} ({abs(x - y) / y:.2e})")
    if not abs(r.time - ref.time) <= TOL_DT * ref.time:
        problems.append(f"{tag}: clock {r.time!r} vs the oracle's {ref.time!r}")
    if host is not None:
        if r.time != host.time:
            problems.append(f"{tag}: clock {r.time!r} is not the host loop's {host.time!r}")
        for k in fields:
            if not np.array_equal(r.state[k], host.state[k]):
                n = int((r.state[k] != host.state[k]).sum())
                problems.append(f"{tag}: {k} differs from the host loop's in {n} cells")
    for k, v in r.options.items():
        if dict(r.asked)[k] != v:
            problems.append(f"{tag}: option {k} reads back {v}")
    return worst


def _expected_launches(case, nr, nphi, opts, n):
    """Launch counts of n Euler steps of fcpt_run_steps on one slab, from fcpt_step.hip (see the module docstring).
    k_boundary: a pair (fewest, most): after the upload of a state the first step's pre-transport call is not folded."""
    o = dict(opts)
    fused_damping = o.get("fused_damping", 1) != 0
    in_step = case.damps() and not case.has_mean() and fused_damping      # the transport's kernels damp
    pure = in_step or not case.damps()                                    # the final call is the ghost-ring kernel alone
    by_rings = nphi % 2 == 0 and 128 <= nphi <= 8192
    rides = o.get("bc_in_cfl", 1) == 2 and by_rings and nr >= 8 and pure
    gate = o.get("gate_in_boundary", 1) == 1 and nphi >= 256 and pure and not rides
    fold = o.get("bc_fold", 1) == 1 and nphi >= 128
    final = 1 if rides else 0 if gate else n
    return {"k_cfl_rings_bc": n - 1 if rides else 0, "k_theta_march_gated_boundary": n if gate else 0,
            "k_boundary": (final, final + 1) if fold else (final + n, final + n),
            "k_damping": None if (case.damps() and not in_step) else 0}


def _check_launches(tag, case, nr, nphi, opts, n, prof, problems):
    want = _expected_launches(case, nr, nphi, opts, n)
    for k, w in want.items():
        got = prof.get(k, 0)
        if w is None:
            ok = got > 0
        elif isinstance(w, tuple):
            ok = w[0] <= got <= w[1]
        else:
            ok = got == w
        if not ok:
            problems.append(f"{tag}: {k} ran {got} times, expected {'some' if w is None else w} (all counts: {prof})")


BASE = (("graph_steps", 0), ("bc_in_cfl", 0), ("gate_in_boundary", 0))
MODES = (
    ("bc_fold0", BASE + (("bc_fold", 0),)),
    ("bc_fold1", BASE + (("bc_fold", 1),)),
    ("bc_in_cfl2", (("graph_steps", 0), ("bc_in_cfl", 2), ("gate_in_boundary", 0))),
    ("gate1", (("graph_steps", 0), ("bc_in_cfl", 0), ("gate_in_boundary", 1))),
    ("fused_damping0", BASE + (("fused_damping", 0),)),
    ("fused_damping0_bc_in_cfl2_gate1", (("graph_steps", 0), ("bc_in_cfl", 2), ("gate_in_boundary", 1), ("fused_damping", 0))),
)
GRAPH_MODES = (
    ("graph", (("graph_steps", 1), ("bc_in_cfl", 0))),
    ("graph_bc_in_cfl2", (("graph_steps", 1), ("bc_in_cfl", 2))),
)


def _device(product, p, nsteps, opts, profile=COUNTED):
    r = BP.run(product, *p, nsteps, mode="device", options=opts, profile=profile)
    r.asked = opts
    return r


@pytest.mark.parametrize("grid", STEP_GRIDS, ids=[f"{a}x{b}" for a, b in STEP_GRIDS])
@pytest.mark.parametrize("ideal", EOS, ids=EOS_IDS)
@pytest.mark.parametrize("case", BP.CASES, ids=CASE_IDS)
def test_every_kernel_that_applies_the_conditions(product, oracle, case, ideal, grid):
    nr, nphi = grid
    n = BP.NSTEPS
    ref = BP.oracle_run(product, oracle, case, nr, nphi, ideal)
    p = d0, radii, st, st0 = ref.planted
    rad = BP.slab_radii(product, d0, radii)
    problems, worst = [], {}

    def merge(w):
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)

    def each(k, S):   # the host loop: the ghost rings after every step
        bad, w = BP.ghost_mismatch(d0, rad, BP.download(S.ctxs[0], ideal), st0)
        problems.extend(f"host loop, step {k + 1}: ghost rings: {m}" for m in bad)
        merge(w)

    host = BP.run(product, *p, n, mode="host", each_step=each, profile=COUNTED)
    host.asked = ()
    merge(_compare("host loop", host, ref, d0, radii, rad, st0, None, problems))
    if host.prof.get("k_boundary", 0) + host.prof.get("k_theta_march_gated_boundary", 0) < n:
        problems.append(f"host loop: the boundary kernels ran {host.prof}")
    for name, opts in MODES:
        if "fused_damping" in dict(opts) and not case.damps():
            continue
        r = _device(product, p, n, opts)
        merge(_compare(name, r, ref, d0, radii, rad, st0, host, problems))
        _check_launches(name, case, nr, nphi, opts, n, r.prof, problems)
    # graph replay: 8 steps, no profiler (a profiled call is not captured)
    n8 = BP.GRAPH_NSTEPS
    ref8 = BP.oracle_run(product, oracle, case, nr, nphi, ideal, nsteps=n8)
    host8 = BP.run(product, *p, n8, mode="host")
    host8.asked = ()
    merge(_compare("host loop, 8 steps", host8, ref8, d0, radii, rad, st0, None, problems))
    for name, opts in GRAPH_MODES:
        r = _device(product, p, n8, opts, profile=None)
        merge(_compare(name, r, ref8, d0, radii, rad, st0, host8, problems))
        if not r.graph_replays > 0:
            problems.append(f"{name}: no graph was replayed")
    print(f"[gpu boundary plants] {case.name} {'ideal' if ideal else 'iso'} {nr}x{nphi}: ghost rings, largest deviation "
          f"in bars (bit rows: wrong cells) {worst}")
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:12])


@pytest.mark.parametrize("ideal", EOS, ids=EOS_IDS)
@pytest.mark.parametrize("name", BP.LEAPFROG_CASES)
def test_leapfrog(product, oracle, name, ideal):
    """Integrator: Leapfrog.  A step makes two boundary calls, as an Euler step does: one without damping between the
    first kick and the transport (folded into the marching source kernel, or its own launch with bc_fold = 0) and the
    final one behind the second kick, whose damping cannot ride in the transport: k_damping runs."""
    case, (nr, nphi), n = BP.CASE_BY_NAME[name], (40, 320), BP.NSTEPS
    ref = BP.oracle_run(product, oracle, case, nr, nphi, ideal, leapfrog=True)
    p = d0, radii, st, st0 = ref.planted
    assert d0.integrator == B.INTEGRATOR_LEAPFROG and case.damps()
    rad = BP.slab_radii(product, d0, radii)
    problems = []
    host = BP.run(product, *p, n, mode="host", profile=COUNTED)
    host.asked = ()
    _compare("host loop", host, ref, d0, radii, rad, st0, None, problems)
    folded = _device(product, p, n, (("graph_steps", 0), ("bc_fold", 1)))
    _compare("run_steps", folded, ref, d0, radii, rad, st0, host, problems)
    unfolded = _device(product, p, n, (("graph_steps", 0), ("bc_fold", 0)))
    _compare("run_steps, bc_fold 0", unfolded, ref, d0, radii, rad, st0, host, problems)
    for tag, prof, lo, hi in (("host loop", host.prof, n, n + 1), ("run_steps", folded.prof, n, n + 1),
                              ("run_steps, bc_fold 0", unfolded.prof, 2 * n, 2 * n)):
        if not lo <= prof.get("k_boundary", 0) <= hi or prof.get("k_damping", 0) == 0 or prof.get("k_cfl_rings_bc", 0):
            problems.append(f"{tag}: launches {prof}, expected k_boundary {lo} .. {hi}, k_damping, no k_cfl_rings_bc")
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:12])


@pytest.mark.parametrize("ideal", EOS, ids=EOS_IDS)
@pytest.mark.parametrize("name", BP.SLAB_CASES)
def test_three_slabs_against_the_one_slab_oracle(product, oracle, name, ideal):
    """Reflecting v_r writes rows 0, 1 and Nr-1, Nr of every slab (no rank guard), outflow only at the disk's edges: the
    gathered state of three slabs is the one-slab oracle's, and its ghost rings are those of its own active rings."""
    case = BP.CASE_BY_NAME[name]
    problems = []
    for nr, nphi in BP.SLAB_GRIDS:
        ref = BP.oracle_run(product, oracle, case, nr, nphi, ideal)
        p = d0, radii, st, st0 = ref.planted
        r = BP.run(product, *p, BP.NSTEPS, mode="host", nslabs=3)
        r.asked = ()
        _compare(f"{nr}x{nphi}, 3 slabs", r, ref, d0, radii, BP.slab_radii(product, d0, radii), st0, None, problems)
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:12])


# ---------------------------------------------------------------------------------------------------------------
# c. a ghost value that sets the time step
def test_ghost_value_binds_dt(product, oracle):
    """GHOST_BINDS_DT: the CFL terms of rings 1 and Nr-2 read rows 1 and Nr-1 of v_r, which only the boundary call
    fills (tests/test_boundary_plants_oracle.py: dt falls to a quarter).  In k_cfl_rings_bc those rings wait for the
    boundary workgroups' stamp; a ring that read the row too early would see the transport's value and return a dt
    several times too large."""
    nr, nphi = BP.BINDS_GRID
    n = 4
    ref = BP.oracle_run(product, oracle, BP.GHOST_BINDS_DT, nr, nphi, False, plant=BP.binds_plant, nsteps=n)
    p = d0, radii, st, st0 = ref.planted
    rad = BP.slab_radii(product, d0, radii)
    problems, clocks = [], []
    host = BP.run(product, *p, n, mode="host", each_step=lambda k, S: clocks.append(S.ctxs[0].clock.time))
    host.asked = ()
    _compare("host loop", host, ref, d0, radii, rad, st0, None, problems)
    opts = (("graph_steps", 0), ("bc_in_cfl", 2))
    for k in range(2, n + 1):   # the clock after k steps, k - 1 of them with the boundary call inside the CFL launch
        r = _device(product, p, k, opts)
        if r.time != clocks[k - 1]:
            problems.append(f"bc_in_cfl = 2, {k} steps: clock {r.time!r}, the host loop's {clocks[k - 1]!r} "
                            f"({abs(r.time - clocks[k - 1]) / clocks[k - 1]:.2e})")
        if r.prof.get("k_cfl_rings_bc", 0) != k - 1:
            problems.append(f"bc_in_cfl = 2, {k} steps: k_cfl_rings_bc ran {r.prof}")
    _compare("bc_in_cfl = 2", r, ref, d0, radii, rad, st0, host, problems)
    n8 = BP.GRAPH_NSTEPS
    ref8 = BP.oracle_run(product, oracle, BP.GHOST_BINDS_DT, nr, nphi, False, plant=BP.binds_plant, nsteps=n8)
    host8 = BP.run(product, *p, n8, mode="host")
    host8.asked = ()
    _compare("host loop, 8 steps", host8, ref8, d0, radii, rad, st0, None, problems)
    g = _device(product, p, n8, (("graph_steps", 1), ("bc_in_cfl", 2)), profile=None)
    _compare("graph, bc_in_cfl = 2", g, ref8, d0, radii, rad, st0, host8, problems)
    if not g.graph_replays > 0:
        problems.append("graph, bc_in_cfl = 2: no graph was replayed")
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:12])
