"""Writes tests/golden/narrow_source_parent_bits.json: the SHA-256 of every grid and of the dt history of the cases of
tests/test_gpu_narrow_source_bits.py, and of the StabilizeViscosity correction-factor grids where k_visc_factors has filled them (asserted non-zero).  Meant for
a build of the commit before the per-loop source kernels were retired (point FCPT_LIB_PATH at its libfargocpt_hip.so); the test
demands the same hashes from the current build.  Every case is run twice: a case that does not reproduce its own hashes on
the recording build is refused.
Needs the GPU.  Usage: python tests/golden/make_narrow_source_parent_bits.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import fargocpt_amd  # noqa: E402

import tests.test_gpu_narrow_source_bits as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    lib = fargocpt_amd.load()
    doc = {"library": "parent commit of the change that retired the per-loop source kernels", "cases": {}, "factors": {}}
    for name in T.CASES:
        doc["cases"][name] = T.case_hashes(lib, name)
        assert T.case_hashes(lib, name) == doc["cases"][name], "%s does not reproduce its own hashes" % name
    for grid in T.FACTOR_GRIDS:
        doc["factors"][T.factor_key(*grid)] = T.factor_hashes(lib, *grid)
        assert T.factor_hashes(lib, *grid) == doc["factors"][T.factor_key(*grid)], grid
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
