"""Writes tests/golden/transport_rows_parent_bits.json: the SHA-256 of every state grid and of the dt history of the cases
of tests/test_gpu_transport_rows.py.  Meant for a build of the commit before k_transport_fused took its per-ring scalars
from TfRow and the widened ShiftRow (point FCPT_LIB_PATH at its libfargocpt_hip.so); the test demands the same hashes
from the current build.  Every case is run twice: a case that does not reproduce its own hashes on the recording build
is refused.
Needs the GPU and the oracle (make -C oracle).  Usage: python tests/golden/make_transport_rows_parent_bits.py [output path]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import fargocpt_amd  # noqa: E402

import tests.test_gpu_transport_rows as T  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    lib = fargocpt_amd.load()
    oracle = T.load_oracle()
    doc = {"library": "parent commit of the change that gave k_transport_fused one packed scalar row per ring", "cases": {}}
    for name in T.CASES:
        doc["cases"][name] = T.case_hashes(lib, oracle, name)
        assert T.case_hashes(lib, oracle, name) == doc["cases"][name], "%s does not reproduce its own hashes" % name
        print("recorded", name, flush=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
