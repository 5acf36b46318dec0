"""fcpt_particles_follow_run_steps without a GPU: the entry points are exported by the library and bound, and the driver
takes tests/golden/setups/dust_drift_live_small.yml (particles over a live gas) as far as the device."""
import inspect
import os

from fargocpt_amd import binding as B

from tests.test_driver_particles_refusals import ROOT, driver

LIVE_SETUP = os.path.join(ROOT, "tests", "golden", "setups", "dust_drift_live_small.yml")
FROZEN_SETUP = os.path.join(ROOT, "tests", "golden", "setups", "dust_drift_small.yml")


def live_config(tmp_path):
    text = open(LIVE_SETUP).read().splitlines()
    text = [("OutputDir: " + str(tmp_path / "out")) if l.startswith("OutputDir") else l for l in text]
    cfg = tmp_path / "config.yml"
    cfg.write_text("\n".join(text) + "\n")
    return str(cfg)


def test_the_entry_points_are_exported_and_bound(product):
    for name in ("particles_follow_run_steps", "particles_follow_run_steps_get"):
        assert product.has(name), name
        assert callable(getattr(B.Context, name)), name
    assert list(inspect.signature(B.Context.particles_follow_run_steps).parameters) == ["self", "on"]
    assert inspect.signature(B.Context.particles_follow_run_steps).parameters["on"].default is True
    header = open(os.path.join(ROOT, "include", "fargocpt_hip.h")).read()
    assert "int fcpt_particles_follow_run_steps(fcpt_ctx *ctx, int32_t on);" in header
    assert "int fcpt_particles_follow_run_steps_get(const fcpt_ctx *ctx, int32_t *on);" in header
    assert "fcpt_run_steps does not" not in header
    assert product.desc_default().abi_version == B.ABI_VERSION == 5        # additive: no new version, fcpt_desc as it was


def test_the_live_setup_differs_from_the_frozen_one_in_the_disk_alone():
    a, b = open(FROZEN_SETUP).read().splitlines(), open(LIVE_SETUP).read().splitlines()
    assert len(a) == len(b)
    changed = sorted(x.split(":")[0] for x, y in zip(a, b) if x != y)
    assert changed == ["Disk", "OutputDir"]
    assert "Disk: 'yes'" in b


def test_live_setup_reaches_the_device(tmp_path):
    """No device visible: the run ends where the library reports FCPT_ENODEV's condition, not at a refusal."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = driver("-q", "start", live_config(tmp_path), env=env)
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "no HIP device" in r.stderr and "not supported" not in r.stderr
