"""Every exit `fargocpt_hip` takes before it asks for a device, pinned: exit code, stderr and stdout of each case equal
what tests/golden/driver_exits.json recorded from the driver of the commit named in that file (the one before main()
was split into stages; tests/golden/make_driver_exits.py wrote it).  The order of the stages is the behaviour: a bad
unit exits with 2 before an unknown key can exit with 1, and no case needs a GPU."""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "fargocpt_amd", "bin", "fargocpt_hip")
SETUP = os.path.join(ROOT, "tests", "golden", "setups", "shocktube_SN.yml")
GOLDEN = os.path.join(ROOT, "tests", "golden", "driver_exits.json")
TOKEN = "<TMP>"

REFUSED_WHEN_ON = ["SelfGravity", "RadiativeDiffusion", "RocheLobeOverflow", "KeepDiskMassConstant", "CircumbinaryRing",
                   "PlanetOrbitDiskTest", "ViscAccretMassFlowTest"]
PLANET = ["- name: Planet{k}", "  semi-major axis: 1000.5 au", "  mass: 0.001", "  eccentricity: '0.0'"]


def _planets(n):
    return ["nbody:"] + [line.format(k=k) for k in range(n) for line in PLANET]


# name -> (arguments, lines appended to the setup, environment); {cfg} is the config, {tmp} the temporary directory
CASES = {
    "no_arguments": ([], [], {}),
    "start_without_config": (["start"], [], {}),
    "mode_bogus": (["bogus", "{cfg}"], [], {}),
    "transport_bogus": (["--transport", "bogus", "start", "{cfg}"], [], {}),
    "ranks_0": (["--ranks", "0", "start", "{cfg}"], [], {}),
    "bodies_bogus": (["--bodies", "bogus", "start", "{cfg}"], [], {}),
    "config_missing": (["start", "{tmp}/nothing.yml"], [], {}),
    "restart_7_empty_dir": (["-q", "restart", "7", "{cfg}"], [], {}),
    "auto_empty_dir": (["auto", "{cfg}"], [], {}),
    **{"refused_" + k.lower(): (["start", "{cfg}"], [k + ": yes"], {}) for k in REFUSED_WHEN_ON},
    "sigmacondition_1d": (["start", "{cfg}"], ["SigmaCondition: 1D"], {}),
    "sigmacondition_2d_setsigma0": (["start", "{cfg}"], ["SigmaCondition: 2D", "SetSigma0: yes"], {}),
    "sigmacondition_2d_missing_file": (["start", "{cfg}"], ["SigmaCondition: 2D", "SigmaFilename: {tmp}/nothing.dat"], {}),
    "rmin_parsec": (["start", "{cfg}"], ["Rmin: 1 parsec"], {}),
    "l0_km": (["start", "{cfg}"], ["l0: 1 km"], {}),
    "innerboundarysigma_bogus": (["start", "{cfg}"], ["InnerBoundarySigma: bogus"], {}),
    "innerboundary_bogus": (["start", "{cfg}"], ["InnerBoundary: bogus"], {}),
    "surfacecooling_bogus": (["start", "{cfg}"], ["SurfaceCooling: bogus"], {}),
    "opacity_bogus": (["start", "{cfg}"], ["Opacity: bogus"], {}),
    "cps_exponential": (["start", "{cfg}"], ["cps: 2", "RadialSpacing: Exponential"], {}),
    "typo": (["start", "{cfg}"], ["Typo: 1"], {}),
    "typo_lenient": (["--lenient", "start", "{cfg}"], ["Typo: 1"], {}),
    "typo_and_rmin_parsec": (["start", "{cfg}"], ["Typo: 1", "Rmin: 1 parsec"], {}),
    "rank_2_of_2": (["start", "{cfg}"], [], {"FCPT_RANK": "2", "FCPT_NRANKS": "2"}),
    "ranks_3_but_nranks_2": (["--ranks", "3", "start", "{cfg}"], [], {"FCPT_RANK": "0", "FCPT_NRANKS": "2"}),
    "bodies_free_with_planet": (["-q", "--bodies", "free", "start", "{cfg}"], _planets(1), {}),
    "bodies_free_nine_bodies": (["-q", "--bodies", "free", "start", "{cfg}"], _planets(8), {}),
}


def run_case(binary, name, tmp):
    """Runs one case in the directory tmp; returns {"code", "stderr", "stdout"} with tmp replaced by TOKEN."""
    args, lines, env = CASES[name]
    tmp = str(tmp)
    text = open(SETUP).read().splitlines()
    text = [("OutputDir: " + os.path.join(tmp, "out")) if line.startswith("OutputDir") else line for line in text]
    cfg = os.path.join(tmp, "config.yml")
    with open(cfg, "w") as f:
        f.write("\n".join(text + [line.format(tmp=tmp) for line in lines]) + "\n")
    environ = {k: v for k, v in os.environ.items() if not k.startswith("FCPT_")}
    environ.update({"HIP_VISIBLE_DEVICES": "-1", "ROCR_VISIBLE_DEVICES": "-1"}, **env)
    r = subprocess.run([binary] + [a.format(cfg=cfg, tmp=tmp) for a in args], capture_output=True, text=True, timeout=120,
                       env=environ, cwd=tmp)
    return {"code": r.returncode, "stderr": r.stderr.replace(tmp, TOKEN), "stdout": r.stdout.replace(tmp, TOKEN)}


def test_the_golden_file_covers_every_case():
    golden = json.load(open(GOLDEN))
    assert len(golden["commit"]) == 40
    assert sorted(golden["cases"]) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_exit_is_the_pinned_one(name, tmp_path):
    want = json.load(open(GOLDEN))["cases"][name]
    got = run_case(BIN, name, tmp_path)
    print(got)
    assert got["code"] == want["code"]
    assert got["stderr"] == want["stderr"]
    assert got["stdout"] == want["stdout"]
