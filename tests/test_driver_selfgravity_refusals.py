"""What the host driver refuses of a setup with SelfGravity: yes, each with exit code 2 and the key named in the first line
of stderr, before any device is asked for (the runs see no GPU).  SelfGravity: yes WITHOUT SelfGravityMode keeps the
generic refusal that tests/test_driver_exits_pinned.py pins (the reference's default is the Bessel kernel)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fargocpt_amd", "bin", "fargocpt_hip")
SETUP = os.path.join(ROOT, "tests", "golden", "setups", "self_gravity.yml")

# name -> (extra arguments, {key: new value} (None: the line is dropped), words the first line of stderr must hold)
CASES = {
    "besselkernel": ([], {"SelfGravityMode": "BesselKernel"}, ["SelfGravityMode: besselkernel", "not supported with SelfGravity"]),
    "unknown_mode": ([], {"SelfGravityMode": "bogus"}, ["SelfGravityMode: bogus", "not supported"]),
    "ideal_eos": ([], {"EquationOfState": "ideal"}, ["EquationOfState: ideal", "not supported with SelfGravity"]),
    "arithmetic_grid": ([], {"RadialSpacing": "Arithmetic"}, ["RadialSpacing", "not supported with SelfGravity"]),
    "ranks_2": (["--ranks", "2"], {}, ["--ranks > 1", "not supported with SelfGravity"]),
    "naz_252": ([], {"Naz": "252"}, ["Naz = 252", "not supported with SelfGravity"]),          # 252 = 4 * 9 * 7
    "nrad_4100": ([], {"Nrad": "4100"}, ["Nrad = 8200", "not supported with SelfGravity"]),    # 2 Nrad > 8192
    "mode_not_written": ([], {"SelfGravityMode": None}, ["'selfgravity' is switched on, but that part of the reference is outside"]),
}


def run_case(case, tmp):
    args, changes, _ = case
    out = []
    for line in open(SETUP).read().splitlines():
        key = line.split(":")[0].strip()
        if line.startswith("OutputDir"):
            line = "OutputDir: " + os.path.join(str(tmp), "out")
        elif key in changes and not line.startswith("#"):
            if changes[key] is None:
                continue
            line = f"{key}: {changes[key]}"
        out.append(line)
    cfg = os.path.join(str(tmp), "config.yml")
    with open(cfg, "w") as f:
        f.write("\n".join(out) + "\n")
    environ = {k: v for k, v in os.environ.items() if not k.startswith("FCPT_")}
    environ.update({"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"})
    return subprocess.run([BIN, "-q"] + args + ["start", cfg], capture_output=True, text=True, timeout=120, env=environ, cwd=str(tmp))


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusal(name, tmp_path):
    r = run_case(CASES[name], tmp_path)
    first = r.stderr.splitlines()[0] if r.stderr else ""
    print(r.returncode, first)
    assert r.returncode == 2
    for word in CASES[name][2]:
        assert word in first, (word, first)
    assert not os.path.exists(os.path.join(str(tmp_path), "out", "snapshots"))


def test_supported_setup_gets_as_far_as_the_device(tmp_path):
    """The reference's own setup (symmetric mode, isothermal, logarithmic, 128 x 256) passes every refusal: without a GPU the
    run ends where the first device is asked for, with exit code 1."""
    r = run_case(([], {}, []), tmp_path)
    assert r.returncode == 1
    assert "no HIP device" in r.stderr
