"""`bench.py --dump-outputs DIR`: what the last timed step computed, as float64 .npy files within 64 MB, from a
timed region whose starting state does not depend on how long the settle steps took."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_budget_and_fixed_sample(tmp_path):
    """The six grids of the ideal EOS at the headline's 2048 x 4096 stay below 64 MB; the sample is the same cells
    in every call; small grids are written whole."""
    sys.path.insert(0, ROOT)
    import bench

    class Clock:
        time, last_dt, n_hydro_iter = 0.5, 1e-3, 7

    nr, nphi = 2048, 4096
    cell = np.arange(nr * nphi, dtype=np.float64).reshape(nr, nphi)
    grids = {k: cell for k in ("sigma", "vazi", "energy", "qplus", "qminus")}
    grids["vrad"] = np.arange((nr + 1) * nphi, dtype=np.float64).reshape(nr + 1, nphi)
    files = bench.dump_outputs(str(tmp_path / "a"), grids, Clock)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 * 2 ** 20
    for f in files:
        assert np.load(tmp_path / "a" / f).dtype == np.float64, f
    picked = np.load(tmp_path / "a" / "sigma_sample.npy")
    assert picked.size == bench.DUMP_MAX_CELLS and np.all(np.diff(picked) > 0)   # the flat indices themselves, sorted
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "sigma_ring_mean.npy"), cell.mean(axis=1))
    bench.dump_outputs(str(tmp_path / "b"), {"sigma": cell}, Clock)
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "sigma_sample.npy"), picked)
    small = np.ones((64, 512))
    assert bench.dump_outputs(str(tmp_path / "c"), {"sigma": small}, Clock, prefix="rank1_") == ["rank1_sigma.npy",
                                                                                                   "rank1_clock.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "rank1_sigma.npy"), small)
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "rank1_clock.npy"), [0.5, 1e-3, 7.0])


@pytest.mark.gpu
@pytest.mark.parametrize("eos", ["isothermal", "ideal"])
def test_dumped_outputs_do_not_depend_on_the_settle_steps(tmp_path, eos):
    """Two bench runs whose time-bound settle loops take different numbers of steps dump the same bits; the clock
    in the dump counts the fixed untimed steps after the rewind plus exactly --steps timed ones."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["FCPT_BENCH_SETTLE_STEPS"] = "20"
    recs = []
    for run, settle_ms in (("a", "1"), ("b", "60")):
        env["FCPT_BENCH_SETTLE_MS"] = settle_ms
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "12", "--warmup", "3", "--nr", "64", "--nphi", "512",
                            "--eos", eos, "--no-cpu-baseline", "--no-configs", "--settle-blocks", "1",
                            "--dump-outputs", str(tmp_path / run)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1
        recs.append(json.loads(lines[0]))
    a, b = recs
    assert a["steps"] == 12 and a["ms_per_step"] > 0 and a["untimed_steps_before_timed_region"] == 20 + 3
    names = {"sigma", "vrad", "vazi"} | ({"energy", "qplus", "qminus"} if eos == "ideal" else set())
    assert set(a["dump_outputs"]["files"]) == {n + ".npy" for n in names | {"clock"}}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b"))
    for f in a["dump_outputs"]["files"]:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and np.isfinite(x).all(), f
        assert np.array_equal(x, y), f
    assert np.load(tmp_path / "a" / "clock.npy")[2] == 20 + 3 + 12
