"""Writes tests/golden/driver_exits.json: exit code, stderr and stdout of every case of
tests/test_driver_exits_pinned.py, run through a driver built from the commit BEFORE a change that must keep them --
never through the driver under test.  Needs no GPU.
Usage: python tests/golden/make_driver_exits.py <fargocpt_hip of that commit> <its 40-digit commit hash> [output path]"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import tests.test_driver_exits_pinned as T  # noqa: E402


def main():
    binary, commit = os.path.abspath(sys.argv[1]), sys.argv[2]
    out = sys.argv[3] if len(sys.argv) > 3 else T.GOLDEN
    cases = {}
    for name in sorted(T.CASES):
        with tempfile.TemporaryDirectory() as tmp:
            cases[name] = T.run_case(binary, name, tmp)
    with open(out, "w") as f:
        json.dump({"commit": commit, "cases": cases}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
