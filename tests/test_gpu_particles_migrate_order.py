"""The emigration serves the leavers of a side in ascending slot order, whatever the order in which wavefronts run.

The middle slab of three (a neighbour on either side), no gas step and no particle step: every slot starts inside the
window, and the leavers are planted by particles_migrate_unpack, which scatters a record into its slot as it stands.
particles_migrate_pack must then fill each message with the lowest leaver slots of its side, in ascending order, as many as
the capacity allows; the rest stay alive and are counted as deferred, and the next call takes the next lowest.  The expected
messages follow from the planted slots alone, so the bar is equality.

Two sizes: 1000 slots (one pass, four workgroups of four wavefronts) and a size at which a workgroup makes three passes of
256 slots, with leavers in the first and last lane of a wavefront, of a pass and of a workgroup's stretch."""
import numpy as np
import pytest

from fargocpt_amd import driver, setups

import tests.particles_cases as cases
import tests.particles_slab_cases as sc

pytestmark = pytest.mark.gpu

REC = 6
GROUPS = 1024            # PARTICLE_MIGRATE_GROUPS: with more than 256 * GROUPS slots a workgroup makes several passes
BIG = 2 * 256 * GROUPS + 77


def _records(slots, r, rng):
    """-> a message's records for `slots` at radius `r`, shuffled: r, phi, r_dot, phi_dot, stokes told apart by slot"""
    rec = np.zeros((slots.size, REC))
    rec[:, 0] = slots
    rec[:, 1] = r
    rec[:, 2] = (slots % 628) * 0.01
    rec[:, 3] = 1e-3 * (slots % 7)
    rec[:, 4] = r ** -1.5
    rec[:, 5] = 1.0 + slots * 1e-7
    return rec[rng.permutation(slots.size)]


def _message(count, rec):
    m = np.zeros(count)
    m[0] = rec.shape[0]
    m[1:1 + rec.size] = rec.ravel()
    return m


@pytest.mark.parametrize("n", [1000, BIG])
def test_lowest_slots_first(product, n):
    d = cases.parity_desc(product, 48, 256)
    radii = product.radii(d)
    fields = product.initial_fields(d.copy(), radii)
    dk = sc.slab_descs(d, 3)[1]
    lo, hi = sc.slab_windows(product, d, radii, 3)[1]
    ctx = driver.make_context(product, dk, fields=sc.cut_fields(product, dk, fields), radii=radii, bodies=setups.jupiter_bodies(d))
    ctx.particles_slabs(True)
    count = ctx.particles_migrate_count()
    built_in = (count - 1) // REC
    k = np.arange(n)
    r0 = np.full(n, 0.5 * (lo + hi))
    ctx.particles_set(cases.parity_params(product, d, False), k + 1, r0, (k % 628) * 0.01, np.zeros(n), r0 ** -1.5, np.full(n, 1e-3),
                      np.ones(n))
    assert ctx.particles_count() == n

    rng = np.random.default_rng(5)
    passes = -(-(-(-n // 256)) // GROUPS)
    chunk = 256 * passes
    assert (passes == 3) == (n == BIG)
    n_out, n_in = (60, 50) if n == 1000 else (3 * built_in // 4, built_in // 2)
    marks = np.array([0, 63, 64, 255, 256, chunk - 1, chunk, chunk + 256, 2 * chunk - 1, n - 1])
    marks = np.unique(marks[marks < n])
    rest = np.setdiff1d(k, marks)
    drawn = rng.choice(rest, n_out + n_in - marks.size, replace=False)
    out_slots = np.sort(np.concatenate([marks[::2], drawn[:n_out - marks[::2].size]]))
    in_slots = np.sort(np.concatenate([marks[1::2], drawn[n_out - marks[::2].size:]]))
    assert out_slots.size == n_out and in_slots.size == n_in and not np.intersect1d(out_slots, in_slots).size
    assert max(n_out, n_in) <= built_in
    rec_out, rec_in = _records(out_slots, hi * 1.001, rng), _records(in_slots, lo * 0.999, rng)
    ctx.particles_migrate_unpack(_message(count, rec_out), _message(count, rec_in))
    assert ctx.particles_count() == n and ctx.particles_slabs_get().received == n_out + n_in

    def by_slot(rec):
        return rec[np.argsort(rec[:, 0])]

    want = {"inner": by_slot(rec_in), "outer": by_slot(rec_out)}
    taken = {"inner": 0, "outer": 0}
    deferred = 0
    cap = 16
    for capacity in (cap, cap, 0):
        ctx.particles_slabs(True, capacity)
        room = capacity or built_in
        msg = {"inner": np.full(count, np.nan), "outer": np.full(count, np.nan)}
        ctx.particles_migrate_pack(msg["inner"], msg["outer"])
        for side in ("inner", "outer"):
            left = want[side][taken[side]:]
            sent = min(room, left.shape[0])
            assert msg[side][0] == sent, (side, capacity, msg[side][0], sent)
            got = msg[side][1:1 + sent * REC].reshape(sent, REC)
            assert np.array_equal(got[:, 0], left[:sent, 0]), (side, capacity, got[:, 0], left[:sent, 0])
            assert np.array_equal(got, left[:sent])
            taken[side] += sent
            deferred += left.shape[0] - sent
        t = ctx.particles_slabs_get()
        assert (t.sent_inner, t.sent_outer, t.deferred) == (taken["inner"], taken["outer"], deferred)
        assert ctx.particles_count() == n - taken["inner"] - taken["outer"]
    assert taken == {"inner": n_in, "outer": n_out} and deferred == 2 * (n_in - cap) + 2 * (n_out - cap) - 2 * cap
    left = ctx.particles_get()
    assert np.array_equal(left["id"], np.setdiff1d(k, np.concatenate([out_slots, in_slots])) + 1)
    ctx.close()
