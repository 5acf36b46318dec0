"""Parity from rough states, cell by cell: HIP against the oracle from noisy, floored and shocked states
(tests/rough_states.py) over one and two steps, in the host loop and (one slab) in the device loop.

Every grid the step writes is compared cell-wise (tests/util.py:cell_err, 1e-10 against the cell's own value or
the field's local scale), the heating and cooling rates included: before the first step both libraries get the same
non-zero sentinel in Q+ and Q-, so an edge ring that a step never writes cannot pass by holding 0 by luck.  Q+ and
Q- on rings 0 and Nr-1 must equal the oracle's exactly.  Each case also asserts that the kernels it is meant to test
ran (the profiler's launch counts), so that a state which trips a fallback or a changed dispatch cannot pass while
testing something else."""
import pytest

from tests import rough_states as R
from tests.parity_runs import compare

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_rough_state_parity(product, oracle, case):
    name, nr, nphi, physics, kind, opt = case
    d = R.case_desc(product, nr, nphi, physics, kind, av=opt.get("av", "TW"), leapfrog=opt.get("leapfrog", False),
                    massflow=opt.get("massflow", False))
    d0, radii, fields = R.make_state(product, d, kind, nslabs=opt["slabs"])
    loops = ["host"] + (["device"] if opt["slabs"] == 1 and opt["tr"] != "fallback" else [])
    for loop in loops:
        for nsteps in (1, 2):
            compare(name, d0, radii, fields, opt["slabs"], nsteps, loop, product, oracle, opt)

