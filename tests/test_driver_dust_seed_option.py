"""`fargocpt_hip --dust-seed N`: the opt-in to dust diffusion (a stochastic run needs a seed, and the driver has no
hidden default).  All of this happens before a device is asked for, so it runs without a GPU."""
import os

import pytest

from tests.test_driver_particles_refusals import config, driver

NO_DEVICE = dict(HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


@pytest.mark.parametrize("edits", [{"ParticleDustDiffusion": "yes"},
                                   {"ParticleDustDiffusion": "yes", "ParticleGasDragEnabled": "no"},
                                   {"ParticleDustDiffusion": "yes", "HydroFrameCenter": "all"}])
def test_with_a_seed_diffusion_reaches_the_device(tmp_path, edits):
    r = driver("-q", "--dust-seed", "7", "start", config(tmp_path, edits), env=dict(os.environ, **NO_DEVICE))
    assert r.returncode == 1, (r.returncode, r.stderr)
    assert "no HIP device" in r.stderr and "not supported" not in r.stderr


def test_the_largest_seed_is_accepted(tmp_path):
    r = driver("-q", "--dust-seed", str(2 ** 64 - 1), "start", config(tmp_path, {"ParticleDustDiffusion": "yes"}),
               env=dict(os.environ, **NO_DEVICE))
    assert r.returncode == 1 and "no HIP device" in r.stderr, (r.returncode, r.stderr)


def test_drag_off_without_diffusion_stays_refused(tmp_path):
    r = driver("-q", "--dust-seed", "7", "start", config(tmp_path, {"ParticleGasDragEnabled": "no"}))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "ParticleGasDragEnabled" in r.stderr and "IntegrateParticles" in r.stderr
    assert not os.path.exists(tmp_path / "out" / "snapshots")


@pytest.mark.parametrize("edits,name", [({"ParticleIntegrator": "explicit"}, "ParticleIntegrator"),
                                        ({"ParticleDiskGravityEnabled": "yes"}, "ParticleDiskGravityEnabled"),
                                        ({"Integrator": "Leapfrog"}, "Integrator: Leapfrog")])
def test_the_seed_lifts_no_other_refusal(tmp_path, edits, name):
    edits = dict(edits, ParticleDustDiffusion="yes")
    r = driver("-q", "--dust-seed", "7", "start", config(tmp_path, edits))
    assert r.returncode == 2 and name in r.stderr, (r.returncode, r.stderr)


def test_without_a_seed_the_refusal_points_at_the_option(tmp_path):
    r = driver("-q", "start", config(tmp_path, {"ParticleDustDiffusion": "yes"}))
    assert r.returncode == 2
    assert "ParticleDustDiffusion is not supported with IntegrateParticles" in r.stderr      # the words it had
    assert "--dust-seed" in r.stderr


@pytest.mark.parametrize("seed", ["-1", "seven", "1.5", "0x10", str(2 ** 64), ""])
def test_a_malformed_seed_is_a_usage_error(tmp_path, seed):
    r = driver("-q", "--dust-seed", seed, "start", config(tmp_path, {"ParticleDustDiffusion": "yes"}))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert "usage:" in r.stderr and "--dust-seed" in r.stderr
    assert not os.path.exists(tmp_path / "out" / "snapshots")
