"""`fargocpt_hip --bodies circular|free`: what the option refuses, it refuses before the driver asks for a device,
so these run without a GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fargocpt_amd", "bin", "fargocpt_hip")
SETUPS = os.path.join(ROOT, "tests", "golden", "setups")


def _config(tmp_path, setup, edits):
    text = open(os.path.join(SETUPS, setup)).read().splitlines()
    text = [("OutputDir: " + str(tmp_path / "out")) if l.startswith("OutputDir") else l for l in text]
    for key, val in edits.items():
        assert any(l.split(":")[0].strip() == key for l in text), key
        text = [(f"{key}: {val}") if l.split(":")[0].strip() == key else l for l in text]
    cfg = tmp_path / "config.yml"
    cfg.write_text("\n".join(text) + "\n")
    return str(cfg)


def _driver(*args):
    return subprocess.run([BIN, *args], capture_output=True, text=True, timeout=120)


def test_free_bodies_refuse_leapfrog(tmp_path):
    cfg = _config(tmp_path, "mpi_simple.yml", {"Integrator": "LeapFrog"})
    r = _driver("-q", "--bodies", "free", "start", cfg)
    assert r.returncode != 0
    assert "--bodies free needs Integrator: Euler" in r.stderr
    assert not os.path.exists(tmp_path / "out" / "snapshots")


def test_free_bodies_refuse_other_frame_centres(tmp_path):
    cfg = _config(tmp_path, "mpi_simple.yml", {"HydroFrameCenter": "binary"})
    r = _driver("-q", "--bodies", "free", "start", cfg)
    assert r.returncode != 0
    assert "HydroFrameCenter: primary" in r.stderr


def test_unknown_bodies_mode_is_a_usage_error(tmp_path):
    cfg = _config(tmp_path, "mpi_simple.yml", {})
    r = _driver("-q", "--bodies", "kepler", "start", cfg)
    assert r.returncode != 0
    assert "usage:" in r.stderr and "--bodies circular|free" in r.stderr
