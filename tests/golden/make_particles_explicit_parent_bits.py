"""Writes tests/golden/particles_explicit_parent_bits.json: the SHA-256 of the ids and of every state and adaptive array of the
eight cases of tests/test_gpu_particles_explicit_bits.py.  Meant for a build of the commit before the clock and slab forms of
k_particles_step_explicit became template arguments (point FCPT_LIB_PATH at its libfargocpt_hip.so); the test demands the same
hashes from the current build.
Needs the GPU.  Usage: python tests/golden/make_particles_explicit_parent_bits.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import fargocpt_amd  # noqa: E402

import tests.test_gpu_particles_explicit_bits as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    lib = fargocpt_amd.load()
    doc = {"library": "parent commit of the one-template explicit kernel", "cases": {T.case_key(*c): T.hashes(lib, c) for c in T.CASES}}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
