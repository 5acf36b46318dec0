"""Parity from planted FARGO shifts, cell by cell: HIP against the oracle from the states of tests/shift_plants.py
(ring pairs with shift differences of +1, 0 and -1, pairs across 0, +Nphi and -Nphi, shifts of a tile and of more
than two turns, +-1 pairs on a chunk's and on a slab's first ring) over one and two steps, in the host loop and (one
slab, no fallback) in the device loop -- compared exactly as tests/test_gpu_rough_states.py compares its states
(tests/parity_runs.py:compare: every grid cell-wise at 1e-10, widened only by the oracle's own measured noise growth
up to 1e-9, dt within 1e-12, and the kernels the case is meant to test must be the ones that ran).

The fused transport kernel couples ring i-1 to ring i through one lane shift chosen by the folded difference of
their shifts; every state carries a Sigma pattern that differs from column to column by 1e-3 .. 1e-2, so a value
taken from the wrong lane misses the bar by seven orders of magnitude.  tests/test_shift_plants_census.py holds each
state to its classes on the CPU.

Worst cell-wise error over all runs of a case, on an MI355X (every case at the plain bar 1e-10): 4e-15 (no FARGO
split) .. 8.7e-13 (minus_visc_32x263_mc); the list is in DESIGN.md.  With lane_prev for lane_next in the kernel's
dsh > 0 branch the five dsh_plus cases fail; without the +-Nphi fold of dsh every fused case with a pair across 0 or
+-Nphi fails."""
import numpy as np
import pytest

from fargocpt_amd import driver
from tests import shift_plants as P
from tests.parity_runs import compare

pytestmark = pytest.mark.gpu


def _chunk_firsts(product, d0, radii, fields, lengths):
    """First rings of the chunks the library makes of `lengths` (every tile has the same)."""
    ctx = driver.make_context(product, d0, fields=fields, radii=radii)
    ctx.set_transport_chunks(lengths)
    tab = ctx.transport_chunks()
    ctx.close()
    live = tab[tab[:, 2] > tab[:, 1]]
    assert len(live) > 0
    return sorted(set(int(x) for x in live[:, 1]))


@pytest.mark.parametrize("name", [c[0] for c in P.CASES])
def test_shift_plant_parity(product, oracle, name):
    case, (d0, radii, fields), rep = P.build(product, oracle, name)
    _, nr, nphi, physics, opt = case
    assert not P.check(case, rep), P.describe(name, rep)
    if opt.get("chunks"):
        firsts = _chunk_firsts(product, d0, radii, fields, opt["chunks"])
        assert set(opt["edge_rings"]) <= set(firsts), f"{name}: chunks start at {firsts}, not at {opt['edge_rings']}"
    loops = ["host"] + (["device"] if opt["slabs"] == 1 and opt["tr"] != "fallback" else [])
    worst = []
    for loop in loops:
        for nsteps in (1, 2):
            worst.append(compare(name, d0, radii, fields, opt["slabs"], nsteps, loop, product, oracle, opt, tag="shift"))
    print(f"[shift] {name}: worst cell-wise error {max(w for w, _ in worst):.2e}, bar {max(t for _, t in worst):.1e}")
