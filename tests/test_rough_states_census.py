"""The rough states reach what they are meant to reach (no GPU: the generators and the oracle only).  A change to
a generator that quietly stops driving a branch fails here, before any parity run could pass on a state that no
longer tests it."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, driver
from tests import rough_states as R
from tests.util import gather_grids


def _wanted(names, d, counts):
    out = []
    for n in names:
        if n.startswith("ideal:") or n.startswith("uncooled:"):
            if d.eos != B.EOS_IDEAL or (n.startswith("uncooled:") and (d.cooling_surface or d.cooling_beta)):
                continue
            n = n.split(":", 1)[1]
        if n == "seams":
            out += [k for k in counts if k.startswith("seam_")]
        elif n == "slabs":
            out += [k for k in counts if k.startswith("slab")]
        else:
            out.append(n)
    return out


@pytest.mark.parametrize("case", R.CASES, ids=[c[0] for c in R.CASES])
def test_state_reaches_its_branches(product, oracle, case):
    name, nr, nphi, physics, kind, opt = case
    d = R.case_desc(product, nr, nphi, physics, kind, av=opt.get("av", "TW"), leapfrog=opt.get("leapfrog", False),
                    massflow=opt.get("massflow", False))
    d0, radii, fields = R.make_state(product, d, kind, nslabs=opt["slabs"])
    counts = R.census(product, d0, fields, opt["slabs"])
    wanted = _wanted(R.INTENDED[kind], d0, counts)
    if kind == "shocked":
        assert "seam_wrap" in wanted and (nphi < 128 or "seam_58_59" in wanted)
        assert opt["slabs"] == 1 or len([k for k in wanted if k.startswith("slab")]) == 3 * (opt["slabs"] - 1)
    low = {k: counts[k] for k in wanted if counts[k] < R.MIN_COUNT}
    assert not low, f"{name}: branches reached by fewer than {R.MIN_COUNT} cells or faces: {low} (census {counts})"
    if kind not in R.POST_INTENDED:
        return
    # one step of the oracle from the state: what did it clamp, which cells took the low-Sigma branch
    ctx = driver.make_context(oracle, d0, fields=fields, radii=radii)
    S = driver.SlabSet([ctx])
    S.prepare()
    S.run(1)
    after = gather_grids(S, ["sigma", "vrad", "vazi", "energy", "qplus", "qminus"])
    ctx.close()
    assert all(np.isfinite(v).all() for v in after.values())
    before = {"sigma": fields[0]}
    post = R.post_census(d0, before, after)
    wanted = _wanted(R.POST_INTENDED[kind], d0, post)
    low = {k: post[k] for k in wanted if post[k] < R.MIN_COUNT}
    assert not low, f"{name}: after one oracle step, fewer than {R.MIN_COUNT} cells in {low} (post-step census {post})"


def test_threshold_patches_straddle_the_low_sigma_threshold(product):
    """The floored state holds cells at the threshold and one ulp to either side of it, with the threshold formed
    in the kernels' operation order."""
    d = R.case_desc(product, 32, 320, "visc", "floored")
    d0, _, fields = R.make_state(product, d, "floored")
    thr = 10.0 * d0.sigma0 * d0.sigma_floor
    sig = fields[0]
    for v in (thr, np.nextafter(thr, 0.0), np.nextafter(thr, np.inf), d0.sigma_floor * d0.sigma0):
        assert (sig == v).sum() >= R.MIN_COUNT, v


def test_states_are_seeded(product):
    d = R.case_desc(product, 32, 320, "visc", "noisy")
    a = R.make_state(product, d, "noisy", seed=3)[2]
    b = R.make_state(product, d, "noisy", seed=3)[2]
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
