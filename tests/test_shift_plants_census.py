"""The planted shifts reach what they are meant to reach (no GPU: tests/shift_plants.py and the oracle only), in
the very runs that tests/test_gpu_shift_plants.py compares: for every case and both compared steps the classes of
ring pairs, the path the differences send the fused transport down, the distance of every unrounded shift from a
rounding edge and the oracle's own amplification of 1e-15 noise.  A change to a generator, to a setup or to the
oracle that quietly moves a shift out of its class fails here, before a parity run could pass on a state that no
longer tests the lane coupling.

Why 1e-3 from a half-integer: the two libraries sum a ring's v_phi in different orders, which moves Ntilde by about
Nphi 2^-53 |Ntilde|, below 1e-10 for every case here; floor(Ntilde + 0.5) is then the same in both."""
import numpy as np
import pytest

from tests import shift_plants as P
from tests.util import GROWTH_CAP

NAMES = [c[0] for c in P.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_case_reaches_its_classes(product, oracle, name):
    case, state, rep = P.build(product, oracle, name)
    print(P.describe(name, rep))
    opt = case[4]
    assert set(opt["classes"]) <= set(P.CLASSES)
    assert len(rep["steps"]) == 2 and state[0].first_dt == 1.0
    bad = P.check(case, rep, P.MARGIN, GROWTH_CAP)
    assert not bad, f"{name}: {bad}\n{P.describe(name, rep)}"
    # the rounding-edge bar against the summation-order estimate it rests on
    for s in rep["steps"]:
        assert case[2] * 2.0 ** -53 * np.abs(s["ntilde"]).max() < 1e-10
    # a wrong lane must change a value: neighbouring columns of Sigma differ by far more than the parity bar
    sig = state[2][0]
    assert (np.abs(np.roll(sig, 1, axis=1) / sig - 1.0) > 1e-6).mean() > 0.99


def test_every_class_and_path_has_a_case():
    reached = set().union(*(c[4]["classes"] for c in P.CASES))
    assert reached == set(P.CLASSES), set(P.CLASSES) - reached
    assert {c[4]["tr"] for c in P.CASES} == {"fused", "two", "fallback"}
    assert all(c[1] <= 48 and c[2] <= 320 for c in P.CASES)
    fused = [c for c in P.CASES if c[4]["tr"] == "fused"]
    assert {c[2] % 2 for c in fused} == {0, 1} and {c[3] for c in fused} == {"iso", "visc"}
    assert {c[4]["limiter"] for c in fused} == {"vl", "mc"}
    assert any(c[4]["slabs"] == 3 for c in P.CASES) and any(c[4].get("chunks") for c in P.CASES)
    assert any(not c[4]["fast"] and c[4]["tr"] == "two" for c in P.CASES)
    assert any(c[2] < 256 and "cross_plus_nphi" in c[4]["classes"] for c in P.CASES)


def test_fallback_case_steps_the_state_of_a_fused_case(product, oracle):
    """The true jump (4 x the CFL step) and the pair that merely straddles Nphi (the CFL step) come from one state:
    the first must raise the shift-jump stamp, the second must not."""
    fb = [c for c in P.CASES if c[4]["tr"] == "fallback"]
    assert len(fb) == 1
    case, state, rep = P.build(product, oracle, fb[0][0])
    twin, tstate, trep = P.build(product, oracle, case[4]["twin"])
    assert twin[4]["tr"] == "fused" and "cross_plus_nphi" in twin[4]["classes"] and twin[4].get("dt_scale", 1.0) == 1.0
    assert all(np.array_equal(x, y) for x, y in zip(state[2], tstate[2]))
    assert "cross_plus_nphi" in trep["steps"][0]["classes"] and np.abs(trep["steps"][0]["dsh"]).max() == 1
    assert np.abs(rep["steps"][0]["dsh"]).max() > 1
    assert rep["dts"][0] == pytest.approx(4.0 * trep["dts"][0], rel=1e-12)


def test_classes_of_known_shifts():
    """The classifier itself, on shifts written by hand (Nphi = 256)."""
    c = lambda n, **kw: P.classes_of(n, 256, **kw)
    assert c([3, 3, 2]) == {"dsh_zero", "dsh_minus"}
    assert c([2, 3]) == {"dsh_plus"}
    assert c([0, -1]) == {"dsh_minus", "cross_zero"}
    assert c([-1, 0]) == {"dsh_plus", "cross_zero"}
    assert c([256, 255]) == {"dsh_minus", "cross_plus_nphi", "tile"}
    assert c([255, 256]) == {"dsh_plus", "cross_plus_nphi", "plus_across_wrap", "tile"}
    assert c([-256, -257]) == {"dsh_minus", "cross_minus_nphi", "tile"}
    assert c([-257, -256]) == {"dsh_plus", "cross_minus_nphi", "plus_across_wrap", "tile"}
    assert c([512, 511]) == {"dsh_minus", "cross_plus_nphi", "twice_round", "tile"}
    assert c([65, 66]) == {"dsh_plus"}                       # beyond a tile, but no multiple of one
    assert c([5, 4, 4], chunk_firsts=[1]) == {"dsh_minus", "dsh_zero", "pair_on_chunk_edge"}
    assert c([5, 4, 4], chunk_firsts=[2], slab_firsts=[1]) == {"dsh_minus", "dsh_zero", "pair_on_slab_edge"}
    assert list(P.fold([255, -255, 128, -128, 2], 256)) == [-1, 1, 128, 128, 2]
    assert P.half_integer_distance([1.25, -3.499, 7.0]) == pytest.approx(1e-3)


def test_states_are_seeded(product, oracle):
    name = "jump_visc_32x320"
    _, state, rep = P.build(product, oracle, name)
    P._BUILT.pop(name)
    try:
        _, again, rep2 = P.build(product, oracle, name)
    finally:
        P._BUILT[name] = (P.BY_NAME[name], state, rep)
    assert all(np.array_equal(x, y) for x, y in zip(state[2], again[2]))
    assert state[0].omega_frame == again[0].omega_frame
    assert all(np.array_equal(a["nshift"], b["nshift"]) for a, b in zip(rep["steps"], rep2["steps"]))
