"""k_transport_fused reads its per-ring scalars from two packed rows per iteration -- TfRow (static, fcpt_tables.cpp) and
ShiftRow, which k_ring_mean completes with every product of the ring's scalars and the step length -- and computes the
bits it computed when every wavefront clamped five table indices and formed those products for itself: SHA-256 of every
state grid and of the dt history after 6 steps of fcpt_run_steps and after 5 host-driven steps, recorded from a build of
the parent commit (tests/golden/make_transport_rows_parent_bits.py).

Grids of 32 x 256 and 40 x 318 cells (a ragged last tile of 53, an Nphi that is no multiple of it): both equations of
state, damping zones on and off, both limiters, planted FARGO shifts (tests/shift_plants.py: ring pairs whose shifts
differ by +1 and by -1, residual velocities of both signs -- both directions of the second azimuthal pass), explicit
chunks of one and two rings, the middle slab of three as its own neighbour (option comm_loopback; 48 x 318: the split
takes no three slabs of fewer rings), and a state whose first host step is 4 x the CFL step, beyond the shear limit, so
that the fallback kernels run from the rows k_ring_mean now writes (the 6 steps of fcpt_run_steps follow its 5 host
steps on the same context: the device loop takes its own step lengths)."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from fargocpt_amd import binding as B, driver
from tests import rough_states as R, shift_plants as P
from tests.parity_runs import run_state
from tests.util import gather_grids

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transport_rows_parent_bits.json")
HOST_STEPS, DEVICE_STEPS = 5, 6


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _names(d0):
    return ["sigma", "vrad", "vazi"] + (["energy"] if d0.eos == B.EOS_IDEAL else [])


def _grid_hashes(grids, d0, dts):
    assert all(np.isfinite(grids[k]).all() for k in _names(d0))
    out = {k: _sha(grids[k]) for k in _names(d0)}
    out["dt"] = _sha(np.asarray(dts, dtype=np.float64))   # (device loop: the clock's time)
    return out


def _rough_state(lib, nr, nphi, physics, kind, limiter, damping):
    d = R.case_desc(lib, nr, nphi, physics, kind)
    d.flux_limiter = B.LIMITER_MC if limiter == "mc" else B.LIMITER_VANLEER
    d.damping = 1 if damping else 0
    return R.make_state(lib, d, kind)


def _both_loops(lib, d0, radii, fields, chunks=None):
    out = {}
    for loop, steps in (("host", HOST_STEPS), ("device", DEVICE_STEPS)):
        grids, dts, prof, _ = run_state(lib, d0, radii, fields, 1, steps, loop, chunks=chunks, profile=True)
        assert prof.get("k_transport_fused", (0, 0))[1] > 0, "k_transport_fused did not run: %s" % sorted(prof)
        out[loop] = _grid_hashes(grids, d0, dts)
    return out


def _rough(nr, nphi, physics, kind, limiter, damping, chunks=None):
    def case(lib, oracle):
        d0, radii, fields = _rough_state(lib, nr, nphi, physics, kind, limiter, damping)
        return _both_loops(lib, d0, radii, fields, chunks)
    return case


# a +1 pair from a jump of the ring mean on the odd grid (the plants of tests/shift_plants.py have none of 318 columns)
_PLANT_318 = P._case("rows_jump_iso_40x318_mc", 40, 318, "iso", ("jump",), ["dsh_plus", "dsh_minus", "dsh_zero"], limiter="mc")
_PLANTED = {}


def _planted_state(lib, oracle, name):
    if name not in _PLANTED:
        if name in P.BY_NAME:
            case, state, rep = P.build(lib, oracle, name)
        else:
            case = _PLANT_318
            for state in P._candidates(lib, oracle, case):
                rep = P.report(oracle, case, state)
                if not P.check(case, rep, P.MARGIN_SEARCH, P.CAP_SEARCH):
                    break
            else:
                raise AssertionError("%s: no candidate state holds the case's conditions" % name)
        first = rep["steps"][0]
        assert {-1, 1} <= set(int(x) for x in first["dsh"]), P.describe(name, rep)
        resid = np.asarray(first["ntilde"]) - np.asarray(first["nshift"])
        assert (resid > 0).any() and (resid < 0).any(), "%s: the residual shifts have one sign" % name
        _PLANTED[name] = state
    return _PLANTED[name]


def _planted(name):
    def case(lib, oracle):
        d0, radii, fields = _planted_state(lib, oracle, name)
        return _both_loops(lib, d0, radii, fields)
    return case


def _fallback(lib, oracle):
    """5 host-driven steps, the first at 4 x the CFL step (beyond the shear limit: the step falls back to the two-kernel
    transport), then 6 steps of fcpt_run_steps on the same context."""
    d = R.case_desc(lib, 32, 256, "iso", "shift_jump")
    d0, radii, fields = R.make_state(lib, d, "shift_jump")
    ctx = driver.make_context(lib, d0, fields=tuple(fields), radii=radii)
    try:
        S = driver.SlabSet([ctx])
        S.prepare()
        dts = []
        for n in range(HOST_STEPS):
            S.dt_scale = 4.0 if n == 0 else 1.0
            dts.append(S.step())
            if n == 0:
                assert ctx.get_option("transport_fell_back") == 1, "the step at 4 x the CFL step did not fall back"
        out = {"host": _grid_hashes(gather_grids(S, _names(d0)), d0, dts)}
        assert ctx.run_steps(DEVICE_STEPS) == DEVICE_STEPS
        out["device"] = _grid_hashes(gather_grids(S, _names(d0)), d0, [ctx.clock.time])
        return out
    finally:
        ctx.close()


def _host_loopback_exchange(ctx):
    cnt = ctx.exchange_count()
    s_in, s_out = np.zeros(cnt), np.zeros(cnt)
    ctx.exchange_pack(s_in, s_out)
    ctx.synchronize()
    ctx.exchange_unpack(s_in, s_out)


def _slab_loopback(lib, oracle):
    """The middle slab of three with itself as both neighbours: 6 steps of fcpt_run_steps through the library's own
    exchange (option comm_loopback), and 5 host-driven steps with the ghost rings staged through the host."""
    d = R.case_desc(lib, 48, 318, "iso", "noisy")
    d0, radii, fields = R.make_state(lib, d, "noisy")
    out = {}
    for loop in ("device", "host"):
        dd = d0.copy()
        dd.rank, dd.nranks = 1, 3
        s = lib.split_domain(dd)
        sub = tuple(np.ascontiguousarray(f[s.imin:s.imin + s.nr + (1 if k == 1 else 0)]) for k, f in enumerate(fields))
        ctx = driver.make_context(lib, dd, fields=sub, radii=radii)
        try:
            if loop == "device":
                ctx.set_option("comm_loopback", 1)
                ctx.comm_init(lib.comm_unique_id())
                xchg = ctx.exchange
                cfl = ctx.cfl_allreduce
            else:
                xchg = lambda: _host_loopback_exchange(ctx)
                cfl = ctx.cfl
            ctx.calculate_timestep(cfl())   # sim::init's sequence
            xchg()
            ctx.apply_boundary(0.0, False)
            ctx.calculate_timestep(cfl())
            xchg()
            if loop == "device":
                assert ctx.run_steps(DEVICE_STEPS) == DEVICE_STEPS
                dts = [ctx.clock.time]
            else:
                dts = []
                for _ in range(HOST_STEPS):
                    dt = ctx.calculate_timestep(ctx.cfl())
                    ctx.step(dt)
                    _host_loopback_exchange(ctx)
                    ctx.post(dt)
                    dts.append(dt)
            st = ctx.state()
            out[loop] = _grid_hashes(st, d0, dts)
        finally:
            if loop == "device":
                ctx.comm_destroy()
            ctx.close()
    return out


CASES = {
    "noisy_iso_32x256_vl_damped": _rough(32, 256, "iso", "noisy", "vl", True),
    "shocked_iso_40x318_mc_undamped": _rough(40, 318, "iso", "shocked", "mc", False),
    "noisy_visc_40x318_vl_damped": _rough(40, 318, "visc", "noisy", "vl", True),
    "floored_visc_32x256_mc_undamped": _rough(32, 256, "visc", "floored", "mc", False),
    "shocked_visc_40x318_mc_damped": _rough(40, 318, "visc", "shocked", "mc", True),
    "planted_shifts_iso_32x256_vl": _planted("jumpwrap_iso_32x256"),
    "planted_shifts_visc_32x256_vl": _planted("jumpwrap_visc_32x256"),
    "planted_shifts_iso_40x318_mc": _planted("rows_jump_iso_40x318_mc"),
    "chunks_of_1_iso_40x318_vl_damped": _rough(40, 318, "iso", "noisy", "vl", True, chunks=[1]),
    "chunks_of_2_1_visc_32x256_vl_damped": _rough(32, 256, "visc", "shocked", "vl", True, chunks=[2, 1, 2, 1, 1, 2]),
    "middle_slab_loopback_iso_48x318": _slab_loopback,
    "fallback_iso_32x256": _fallback,
}


def case_hashes(lib, oracle, name):
    return CASES[name](lib, oracle)


def load_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return B.Library(ctypes.CDLL(os.path.join(root, "oracle", "libfargo_oracle.so")), "orc_")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_record_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(CASES)
    for name, rec in golden["cases"].items():
        assert sorted(rec) == ["device", "host"], name


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_transport_rows_give_the_parent_bits(product, oracle, golden, name):
    assert case_hashes(product, oracle, name) == golden["cases"][name]
