"""k_transport_fused where a chunk begins, and where a tile ends.

A chunk's wavefront fills its rolling window from the rings below its first ring: the ring just below goes through both
azimuthal passes only to leave Sigma and the transported rm+, from which the first ring's v_r is formed, and the limited
slope of L+ / Sigma is taken from the lane to the right, whose L- / Sigma it is (lane 63 has none and is halo).

Every ring is stored by exactly one chunk, and the ring below it is a full ring of the chunk before: so a run with
ragged explicit chunks must leave the bits of the run with equal chunks (the library's choice on grids this small), for
both limiters, both equations of state, a last tile of two columns, and chunks of one and two rings, where the
window-filling rings are most of what a wavefront marches."""
import numpy as np
import pytest

from fargocpt_amd import binding as B, setups

pytestmark = pytest.mark.gpu

CASES = {
    # 5 tiles of 53 columns, the last one 44 wide; single rings at both ends of the slab (damping zones)
    "iso_64x256": (64, 256, False, [1, 9, 1, 3, 17, 2, 5]),
    # 320 = 6 x 53 + 2: the last tile stores two columns
    "ideal_64x320": (64, 320, True, [11, 1, 2, 23, 1, 4]),
    # chunks of 1 and 2 rings only (the last entry repeats)
    "iso_64x256_ones_and_twos": (64, 256, False, [2, 1, 1, 2, 2, 1, 2, 1]),
}


def _uniform_residual(product, d, st, dt):
    """Per ring, the fraction of a cell the second azimuthal pass moves the ring by (ComputeConstantResidual): its sign is
    the sign of vconst, which selects the specialisation of that pass."""
    r = product.radii(d)
    ri, ro = r[:d.nr_global], r[1:d.nr_global + 1]
    rmed = 2.0 / 3.0 * (ro ** 3 - ri ** 3) / (ro ** 2 - ri ** 2)
    ntilde = st["vazi"].mean(axis=1) / rmed * dt / (2.0 * np.pi / d.nphi)
    return ntilde - np.floor(ntilde + 0.5)


@pytest.mark.parametrize("limiter", [B.LIMITER_VANLEER, B.LIMITER_MC], ids=["vanleer", "mc"])
@pytest.mark.parametrize("case", list(CASES))
def test_ragged_chunks_leave_the_bits_of_equal_chunks(product, case, limiter):
    from fargocpt_amd import driver
    nr, nphi, adi, lengths = CASES[case]
    d = setups.planet_disk(product, nr, nphi, adiabatic=adi)
    d.flux_limiter = limiter
    bodies = setups.jupiter_bodies(d)
    out = []
    for explicit in (True, False):
        ctx = driver.make_context(product, d, bodies=bodies)
        if explicit:
            ctx.set_transport_chunks(lengths)
            tab = ctx.transport_chunks()
            live = tab[tab[:, 2] > tab[:, 1]]
            tiles = -(-nphi // 53)
            cover = np.zeros((tiles, nr), dtype=np.int32)      # every ring of every tile exactly once
            for tl, a, b in live:
                cover[tl, a:b] += 1
            assert (cover == 1).all()
            if case.endswith("ones_and_twos"):
                # (the chunk dealt last, where the two ends meet, also takes what is left when fewer than three rings
                #  remain -- "no crumbs", transport_chunk_list(): up to 2 + 2 rings, one such chunk per tile)
                n = live[:, 2] - live[:, 1]
                assert (n == 1).any() and (n == 2).any() and n.max() <= 4 and (n > 2).sum() <= tiles
        else:
            ctx.set_option("transport_graded", 0)
            assert len(ctx.transport_chunks()) == 0
        S = driver.SlabSet([ctx])
        S.prepare()
        assert ctx.run_steps(13) == 13
        c = ctx.clock
        out.append((ctx.state(), (c.time, c.last_dt, c.n_hydro_iter)))
        ctx.close()
    assert out[0][1] == out[1][1]
    for k in out[0][0]:
        assert np.isfinite(out[0][0][k]).all(), k
        assert np.array_equal(out[0][0][k], out[1][0][k]), k
    # both specialisations of the second pass ran: rings of this very run whose uniform residual is clearly positive and
    # clearly negative (by a tenth of a cell: the thirteenth step's residuals, and no source step moves a ring mean that far)
    frac = _uniform_residual(product, d, out[0][0], out[0][1][1])[2:-2]
    assert (frac > 0.1).any() and (frac < -0.1).any(), (frac.min(), frac.max())
