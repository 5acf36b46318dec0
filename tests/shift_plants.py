"""Planted FARGO shifts: initial states whose per-ring integer shifts Nshift[i] at the CFL step fall in named
classes -- ring pairs with Nshift[i] - Nshift[i-1] = +1, 0 and -1, pairs that straddle 0, +Nphi and -Nphi (where
Nshift % Nphi wraps between the two rings), shifts of a whole 64-lane tile and of more than two turns of the ring,
and +-1 pairs on the first ring of a chunk of the fused transport kernel and on the first own ring of a slab.  The
suite's other states never leave Nshift in -5 .. 8 with differences of 0 and -1 (a Keplerian disk shears one way).

Two knobs place the shifts, both searched with the CPU oracle when a case is first asked for (plain numpy and the
oracle, seeded, no GPU; the search is deterministic):

  * OmegaFrame adds the same -Omega dt / dphi to every ring's shift, without shear, and changes the CFL step by less
    than a per cent (the fast-transport CFL uses the residual velocity).  It is tuned by fixed-point iteration on the
    oracle's own dt and unrounded shifts Ntilde until the half-integer that separates two chosen values of Nshift lies
    between the Ntilde of the two rings of a chosen pair (midway, or at another of FRACTIONS).
  * A one-ring jump of the ring-mean v_phi: the inertial v_phi + r Omega times 1 + A from ring k outward, k near the
    inner edge where r dphi / dt is smallest.  Whether the pair at ring k then rounds to +1 depends on the rounding
    phase, so (k, A) are searched and the first pair that holds is kept.

A candidate is kept only if it passes `check` at the search's own bars: the case's intended classes are reached,
max |dsh| (modulo Nphi) stays within 1 in both compared steps (all but the fallback case, where it must exceed 1),
every Ntilde keeps MARGIN_SEARCH from a half-integer, the oracle amplifies 1e-15 noise by less than CAP_SEARCH (0.8 of tests/util.py:GROWTH_CAP), and the CFL step itself
is not set by the shear limit between two large ring means (`dt_rounding`: in a frame that turns once per step the
shear limit cfl dphi / |Omega_i - Omega_i+1| is a difference of two numbers 500 times its size, and the two libraries'
steps then differ by 1e-12 .. 3e-12 -- measured on the GPU with 16 rings -- from the order of the ring sums alone;
with 32 .. 48 rings the sound speed sets the step instead).  tests/test_shift_plants_census.py
holds the result to the (weaker) bars of the census; tests/test_gpu_shift_plants.py compares the HIP library with
the oracle from these states.

Every state carries 1 + 0.03 sin(3 phi) cos(5 ln r) + 1 % cell-wise noise in Sigma (and e): a value taken from the
wrong lane differs from the right one by 1e-3 .. 1e-2 of itself.  Every case starts at first_dt = 1, so both compared
steps run at the CFL step.

Without the FARGO split (fast_transport = 0) the CFL condition sees the whole v_phi, |Ntilde| stays below the CFL
number and every shift is 0: that case reaches `dsh_zero` alone and is here for the path it takes.  (At the CFL number
0.5 the limiting ring has Ntilde = 0.5 (1 - h^2 / 2), 6e-4 from the rounding edge; the case runs at 0.4.)

The census answers the question of the class `plus_across_wrap` (a +1 pair that straddles a multiple of Nphi): the
jump and the frame offset together reach it at an admissible step, towards +Nphi and towards -Nphi -- the cases
jumpwrap_* below.
"""
from __future__ import annotations

import numpy as np

from fargocpt_amd import binding as B
from tests import rough_states as R
from tests.parity_runs import errors, run_state
from tests.util import GROWTH_CAP

TILE = 64              # lanes of one column tile of the fused transport kernel
MARGIN = 1.0e-3        # the census's bar: distance of every Ntilde from a half-integer
MARGIN_SEARCH = 5.0e-3  # the search's own, so that the census's holds with room
CAP_SEARCH = 0.8 * GROWTH_CAP
FRACTIONS = (0.5, 0.35, 0.65)   # where between the two rings' Ntilde the half-integer is put
CLASSES = ("dsh_plus", "dsh_minus", "dsh_zero", "cross_zero", "cross_plus_nphi", "cross_minus_nphi",
           "plus_across_wrap", "tile", "twice_round", "pair_on_chunk_edge", "pair_on_slab_edge")


# ---------------------------------------------------------------------------------------------------------------
# classes of a vector of shifts


def fold(dsh, nphi):
    """Nshift[i] - Nshift[i-1] modulo Nphi, in (-Nphi/2, Nphi/2]: the lane distance the fused kernel couples over."""
    d = np.asarray(dsh, dtype=np.int64) % nphi
    return np.where(d > nphi // 2, d - nphi, d)


def classes_of(nshift, nphi, chunk_firsts=(), slab_firsts=()) -> set:
    """The classes (names of CLASSES) that the shifts of one transport reach.  A pair is (i-1, i), named by its
    upper ring i."""
    n = np.asarray(nshift, dtype=np.int64)
    lo, hi = n[:-1], n[1:]
    d = fold(hi - lo, nphi)
    turn_lo, turn_hi = lo // nphi, hi // nphi        # which turn of the ring a shift lies in (floor)
    wraps = turn_lo != turn_hi
    upper = np.arange(1, n.size)
    out = set()
    if (d == 1).any():
        out.add("dsh_plus")
    if (d == -1).any():
        out.add("dsh_minus")
    if (d == 0).any():
        out.add("dsh_zero")
    if (((lo >= 0) & (hi < 0)) | ((hi >= 0) & (lo < 0))).any():
        out.add("cross_zero")
    if (wraps & (np.maximum(turn_lo, turn_hi) >= 1)).any():
        out.add("cross_plus_nphi")
    if (wraps & (np.minimum(turn_lo, turn_hi) <= -2)).any():
        out.add("cross_minus_nphi")
    if (wraps & (d == 1) & ((np.maximum(turn_lo, turn_hi) >= 1) | (np.minimum(turn_lo, turn_hi) <= -2))).any():
        out.add("plus_across_wrap")
    if (np.abs(n) >= TILE).any() and ((np.abs(n) >= TILE) & (n % TILE == 0)).any():
        out.add("tile")
    if (np.abs(n) >= 2 * nphi).any():
        out.add("twice_round")
    one = np.abs(d) == 1
    if one[np.isin(upper, list(chunk_firsts))].any():
        out.add("pair_on_chunk_edge")
    if one[np.isin(upper, list(slab_firsts))].any():
        out.add("pair_on_slab_edge")
    return out


def half_integer_distance(ntilde) -> float:
    """Smallest distance of any Ntilde from a half-integer (where floor(Ntilde + 0.5) jumps)."""
    x = np.asarray(ntilde, dtype=np.float64)
    return float(np.abs(x - np.floor(x) - 0.5).min())


# ---------------------------------------------------------------------------------------------------------------
# descriptors and states


def case_desc(lib, nr, nphi, physics, opt) -> B.Desc:
    """planet_disk on [1, 2.5] (wide cells: a large CFL step, so that one frame turn per step needs |v_phi| of
    30 .. 130 only) with the physics of a rough-state case, the limiter and the FARGO split of `opt`."""
    d = R.case_desc(lib, nr, nphi, physics, "noisy")
    d.rmin = 1.0
    d.flux_limiter = B.LIMITER_MC if opt["limiter"] == "mc" else B.LIMITER_VANLEER
    d.fast_transport = 1 if opt["fast"] else 0
    d.omega_frame = 0.0
    d.cfl = opt.get("cfl_number", d.cfl)
    d.viscous_alpha = opt.get("alpha", d.viscous_alpha)
    return d


def _rmed(radii, nr):
    ri = np.asarray(radii[:nr + 1])
    return 0.5 * (ri[:-1] + ri[1:])


def make_fields(lib, d, omega, jump=None, seed=0):
    """(descriptor of the global grid, radii, [Sigma, v_r, v_phi, e]) in the frame rotating with `omega`, with the
    non-axisymmetric perturbation of Sigma and e and, for jump = (k, A), the inertial v_phi times 1 + A from ring k
    outward."""
    d = d.copy()
    d.omega_frame = omega
    d0, radii, (sig, vr, va, e) = R.base_state(lib, d)
    nr, nphi = sig.shape
    rng = np.random.default_rng(seed)
    phi = (np.arange(nphi) + 0.5) * 2 * np.pi / nphi
    r = _rmed(radii, nr)
    f = 1.0 + 0.03 * np.sin(3 * phi)[None, :] * np.cos(5 * np.log(r))[:, None] + 0.01 * rng.uniform(-1.0, 1.0, size=sig.shape)
    sig = sig * f
    e = e * f
    if jump is not None:
        k, amp = jump
        ro = (r * omega)[k:, None]
        va = va.copy()
        va[k:] = (va[k:] + ro) * (1.0 + amp) - ro
    fields = [np.ascontiguousarray(x) for x in (sig, vr, va, e)]
    assert fields[0].min() > 0 and all(np.isfinite(x).all() for x in fields)
    return d0, radii, fields


def tune_omega(lib, oracle, d, pair, multiple, jump=None, seed=0, dt_scale=1.0, frac=0.5):
    """OmegaFrame for which the half-integer multiple - 1/2 lies midway between Ntilde[pair - 1] and Ntilde[pair] in
    the first step: Nshift takes the values `multiple` and `multiple - 1` on the two rings (which ring takes which
    depends on the sign of the pair's difference).  dNtilde / dOmega = -dt / dphi, and dt moves by less than a per
    cent with Omega: the iteration converges in three or four rounds."""
    omega = 0.0
    dphi = 2 * np.pi / d.nphi
    for _ in range(8):
        d0, radii, fields = make_fields(lib, d, omega, jump, seed)
        sh = []
        _, dts, _, _ = run_state(oracle, d0, radii, fields, 1, 1, "host", dt_scale=dt_scale, shifts=sh)
        nt = sh[0][1]
        off = (1.0 - frac) * nt[pair - 1] + frac * nt[pair] - (multiple - 0.5)
        if abs(off) < 1.0e-4:
            break
        omega += off * dphi / dts[0]
    return omega


def dt_rounding(d0, radii, vazi, cfl_dt) -> float:
    """Estimate of the relative rounding error of a CFL step that its shear limit sets (cfl.cpp:207-220:
    cfl dphi / |<v_phi>/r of ring i - of ring i+1|).  In a fast frame the two terms are large and nearly equal:
    each ring mean carries the rounding of a sum of Nphi like terms, about sqrt(Nphi) 2^-53 of itself (the two
    libraries sum in different orders), and the difference loses (|a| + |b|) / |a - b| of it.  0 where no ring pair's
    shear limit comes within 2 % of the step: every other limit reads v_phi - <v_phi> against the sound speed, where
    the same error is 1e-13 of the result or less."""
    nr, nphi = vazi.shape
    om = vazi.mean(axis=1) / _rmed(radii, nr)
    diff = np.abs(np.diff(om)) + 1.0e-100
    shear_dt = d0.cfl * (2 * np.pi / nphi) / diff
    binds = shear_dt <= 1.02 * cfl_dt
    if not binds.any():
        return 0.0
    loss = (np.abs(om[:-1]) + np.abs(om[1:])) / diff
    return float(np.sqrt(nphi) * 2.0 ** -53 * loss[binds].max())


def report(oracle, case, state) -> dict:
    """What the oracle does from a state in the two compared steps: per step the shifts, Ntilde, the folded
    differences and the classes; the dt history; whether all grids are finite; the growth of 1e-15 noise."""
    name, nr, nphi, physics, opt = case
    d0, radii, fields = state
    sc = opt.get("dt_scale", 1.0)
    sh = []
    b, dts, _, _ = run_state(oracle, d0, radii, fields, 1, 2, "host", dt_scale=sc, shifts=sh)
    slab_firsts = R.slab_edges(oracle, d0, opt["slabs"]) if opt["slabs"] > 1 else ()
    steps = []
    for n, nt in sh:
        steps.append({"nshift": n, "ntilde": nt, "dsh": fold(np.diff(n), nphi),
                      "classes": classes_of(n, nphi, opt.get("edge_rings", ()), slab_firsts),
                      "margin": half_integer_distance(nt)})
    finite = all(np.isfinite(v).all() for v in b.values())
    growth = np.inf
    if finite:
        b1 = run_state(oracle, d0, radii, fields, 1, 1, "host", dt_scale=sc)[0]
        for s, va, dt in zip(steps, (fields[2], b1["vazi"]), dts):
            s["dt_rounding"] = dt_rounding(d0, radii, va, dt / sc)
        b2, dts2, _, _ = run_state(oracle, d0, radii, fields, 1, 2, "host", noise=1.0e-15, dt_scale=sc)
        growth = max(e for e, _ in errors(d0, radii, b2, b, sum(dts)).values()) / 1.0e-15
    return {"steps": steps, "dts": dts, "finite": finite, "growth": growth, "omega": d0.omega_frame}


DT_ROUNDING = 2.5e-13   # a quarter of the parity tests' bar on dt (1e-12)


def check(case, rep, margin=MARGIN, cap=GROWTH_CAP) -> list:
    """The conditions of the census on a report; returns the list of those that fail (empty: all hold)."""
    name, nr, nphi, physics, opt = case
    bad = []
    reached = set().union(*(s["classes"] for s in rep["steps"]))
    missing = set(opt["classes"]) - reached
    if missing:
        bad.append(f"classes not reached in either step: {sorted(missing)}")
    if "dsh_plus" in opt["classes"] and "dsh_plus" not in rep["steps"][0]["classes"]:
        bad.append("no dsh = +1 pair in the first step")
    if "plus_across_wrap" in opt["classes"] and "plus_across_wrap" not in rep["steps"][0]["classes"]:
        bad.append("no +1 pair across the wrap in the first step")
    worst = [int(np.abs(s["dsh"]).max()) for s in rep["steps"]]
    if opt["tr"] == "fallback":
        if worst[0] <= 1:
            bad.append(f"the fallback case has max |dsh| = {worst[0]} in its first step")
    elif max(worst) > 1:
        bad.append(f"max |dsh| modulo Nphi is {worst} in the two steps")
    m = min(s["margin"] for s in rep["steps"])
    if m < margin:
        bad.append(f"an Ntilde lies {m:.2e} from a half-integer (< {margin:.0e})")
    if not rep["finite"]:
        bad.append("the oracle left the finite range")
    else:
        if rep["growth"] > cap:
            bad.append(f"the oracle amplifies 1e-15 noise by {rep['growth']:.2e} (> {cap:.1e})")
        worst_dt = max(s["dt_rounding"] for s in rep["steps"])
        if worst_dt > DT_ROUNDING:
            bad.append(f"the shear limit sets the step between two large, nearly equal ring means: the step itself is "
                       f"uncertain by about {worst_dt:.1e} (> {DT_ROUNDING:.1e})")
    return bad


# ---------------------------------------------------------------------------------------------------------------
# the cases: (id, nr, nphi, physics, options)
# options: limiter "vl" | "mc"; fast (the FARGO split); plant: how the shifts are placed (below); classes: the
# classes the case is meant to reach; slabs; chunks (explicit chunk lengths of the fused kernel) with edge_rings (rings
# that are the first of a chunk for these lengths whatever the damping zones cost: the GPU test checks it against the
# library's table); dt_scale; twin (the case whose state this one reuses); src, tr, cfl as in tests/rough_states.py.
# plant: ("frame", turns, add)         Omega so that a pair straddles turns * Nphi + add (pair: opt["pair"] or searched)
#        ("jump",)                     Omega = 0, a jump (k, A) that gives a +1 pair in the first step
#        ("jump_frame", turns, add)    the +1 pair of a jump placed across turns * Nphi + add
#        ("none",)                     Omega = 0, the state as it is
#        ("twin",)                     the state of the case opt["twin"], stepped at this case's dt_scale


def _case(name, nr, nphi, physics, plant, classes, **opt):
    opt.update(plant=plant, classes=tuple(classes))
    opt.setdefault("limiter", "vl")
    opt.setdefault("fast", True)
    opt.setdefault("slabs", 1)
    opt.setdefault("src", "march" if nphi >= 128 else "fused")
    opt.setdefault("tr", "fused" if nphi >= 256 else "two")
    opt.setdefault("cfl", R._cfl_path(nphi, physics))
    return (name, nr, nphi, physics, opt)


CASES = [
    # the frame offset alone, on even and odd fused rings, both equations of state, both limiters
    _case("plus_iso_40x256", 40, 256, "iso", ("frame", 1, 0), ["cross_plus_nphi", "dsh_minus", "dsh_zero", "tile"]),
    _case("minus_visc_32x263_mc", 32, 263, "visc", ("frame", -1, 0), ["cross_minus_nphi", "dsh_minus", "dsh_zero"],
          limiter="mc"),
    _case("tile_visc_32x320", 32, 320, "visc", ("frame", 0, TILE), ["tile", "dsh_minus", "dsh_zero"]),
    _case("twice_iso_40x263_mc", 40, 263, "iso", ("frame", 2, 0), ["twice_round", "cross_plus_nphi", "dsh_minus"],
          limiter="mc"),
    _case("zero_visc_16x256", 16, 256, "visc", ("frame", 0, 0), ["cross_zero", "dsh_minus", "dsh_zero"]),
    # a jump of the ring mean: the +1 pair, alone and across the wrap
    _case("jump_visc_32x320", 32, 320, "visc", ("jump",), ["dsh_plus", "dsh_minus", "dsh_zero"]),
    _case("jump_iso_32x263_mc", 32, 263, "iso", ("jump",), ["dsh_plus", "dsh_minus", "dsh_zero"], limiter="mc"),
    _case("jumpwrap_iso_32x256", 32, 256, "iso", ("jump_frame", 1, 0),
          ["plus_across_wrap", "dsh_plus", "cross_plus_nphi", "dsh_minus"]),
    _case("jumpwrap_iso_32x263_mc", 32, 263, "iso", ("jump_frame", -1, 0),
          ["plus_across_wrap", "dsh_plus", "cross_minus_nphi", "dsh_minus"], limiter="mc"),
    _case("jumpwrap_visc_32x256", 32, 256, "visc", ("jump_frame", 1, 0),
          ["plus_across_wrap", "dsh_plus", "cross_plus_nphi", "dsh_minus"]),
    # (the ideal EOS amplifies noise by 5e3 .. 8e3 from a jump in a fast frame, more than the isothermal one: the
    # search keeps the first candidate under its cap)
    # the two-kernel path: the marching azimuthal kernel (130 columns), the per-pass kernels without the FARGO split
    # (odd rings of 65 .. 128 columns)
    _case("narrow_iso_32x130", 32, 130, "iso", ("frame", 1, 0), ["cross_plus_nphi", "dsh_minus", "dsh_zero"]),
    _case("narrow_visc_16x97", 16, 97, "visc", ("frame", -1, 0), ["cross_minus_nphi", "dsh_minus", "dsh_zero"]),
    _case("nosplit_iso_16x97", 16, 97, "iso", ("none",), ["dsh_zero"], fast=False, cfl_number=0.4),
    # the fallback: a state stepped at the CFL step (fused, a pair across +Nphi) and at 4 x the CFL step (a true jump).
    # Four times the step must keep below the sound limit, and the shifts of neighbouring rings must part by more
    # than 1.5 in it: the step has to lie within 3/4 of the shear limit without being set by it (DT_ROUNDING), and
    # well below the sound limit -- 14 coarse rings, and alpha = 0.45, whose viscous limit sets the step
    _case("plus_alpha_iso_14x256", 14, 256, "iso", ("frame", 1, 0), ["cross_plus_nphi", "dsh_minus", "dsh_zero"], alpha=0.45),
    _case("fallback_iso_14x256", 14, 256, "iso", ("twin",), [], twin="plus_alpha_iso_14x256", dt_scale=4.0, tr="fallback",
          alpha=0.45),
    # three slabs, ragged chunks
    _case("slabs_iso_48x256", 48, 256, "iso", ("frame", 1, 0), ["pair_on_slab_edge", "cross_plus_nphi", "dsh_minus"],
          slabs=3, pair="slab"),
    _case("chunks_iso_40x320", 40, 320, "iso", ("frame", 1, 0), ["pair_on_chunk_edge", "cross_plus_nphi", "dsh_minus"],
          chunks=[5, 3, 7], edge_rings=(23, 30, 37), pair=23),
]
BY_NAME = {c[0]: c for c in CASES}

JUMP_RINGS = (4, 3, 5, 6, 7, 8)
JUMP_AMPS = (0.20, 0.18, 0.22, 0.16, 0.24, 0.14, 0.26, 0.12, 0.28, 0.10)


def _pairs(lib, case):
    """Upper rings of the pairs to try for a frame plant: the one the case fixes, or from the middle outward."""
    name, nr, nphi, physics, opt = case
    pair = opt.get("pair")
    if pair == "slab":
        d = case_desc(lib, nr, nphi, physics, opt)
        return R.slab_edges(lib, d, opt["slabs"])
    if pair is not None:
        return [pair]
    return sorted(range(3, nr - 2), key=lambda i: abs(i - nr // 2))


def _candidates(lib, oracle, case):
    """States to try, in a fixed order."""
    name, nr, nphi, physics, opt = case
    d = case_desc(lib, nr, nphi, physics, opt)
    plant = opt["plant"]
    if plant[0] == "none":
        yield make_fields(lib, d, 0.0)
    elif plant[0] == "frame":
        multiple = plant[1] * nphi + plant[2]
        for frac in FRACTIONS:
            for pair in _pairs(lib, case):
                yield make_fields(lib, d, tune_omega(lib, oracle, d, pair, multiple, frac=frac))
    else:
        for k in JUMP_RINGS:
            for amp in JUMP_AMPS:
                if plant[0] == "jump":
                    yield make_fields(lib, d, 0.0, (k, amp))
                else:
                    multiple = plant[1] * nphi + plant[2]
                    for frac in FRACTIONS:
                        yield make_fields(lib, d, tune_omega(lib, oracle, d, k, multiple, (k, amp), frac=frac), (k, amp))


_BUILT = {}


def build(lib, oracle, name):
    """(case, (descriptor, radii, fields), report) of a case: the first candidate that passes `check` at the search's
    margins -- and, where another case steps the same state at another dt_scale, whose twin passes too."""
    if name in _BUILT:
        return _BUILT[name]
    case = BY_NAME[name]
    opt = case[4]
    if opt["plant"][0] == "twin":
        _, state, _ = build(lib, oracle, opt["twin"])
        out = (case, state, report(oracle, case, state))
        _BUILT[name] = out
        return out
    twins = [c for c in CASES if c[4].get("twin") == name]
    tried = []
    for state in _candidates(lib, oracle, case):
        rep = report(oracle, case, state)
        bad = check(case, rep, MARGIN_SEARCH, CAP_SEARCH)
        for t in twins:
            if not bad:
                bad = [f"{t[0]}: {b}" for b in check(t, report(oracle, t, state), MARGIN_SEARCH, CAP_SEARCH)]
        if not bad:
            _BUILT[name] = (case, state, rep)
            return _BUILT[name]
        tried.append(bad)
    raise AssertionError(f"{name}: no candidate state holds the case's conditions; the failures: {tried}")


def describe(name, rep) -> str:
    """One line per step: the shift range, the set of dsh, the margin; then dt, Omega and the noise growth."""
    lines = []
    for k, s in enumerate(rep["steps"]):
        lines.append(f"[shift] {name} step {k + 1}: Nshift {int(s['nshift'].min())} .. {int(s['nshift'].max())}, "
                     f"dsh {sorted(set(int(x) for x in s['dsh']))}, classes {sorted(s['classes'])}, "
                     f"margin {s['margin']:.3f}, dt {rep['dts'][k]:.4e} (rounding {s.get('dt_rounding', np.nan):.1e})")
    lines.append(f"[shift] {name}: OmegaFrame {rep['omega']:.4f}, noise growth {rep['growth']:.2e}")
    return "\n".join(lines)
