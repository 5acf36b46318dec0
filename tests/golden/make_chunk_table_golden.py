"""Writes tests/golden/chunk_tables_parent.json: the chunk tables of the marching kernels (fcpt_selftest_chunk_tables:
host logic, no GPU) as a given build of the library computes them.

    python tests/golden/make_chunk_table_golden.py /path/to/libfargocpt_hip.so

The library named must be a build of the commit BEFORE the change under test -- never the tree the test then runs
on -- so that tests/test_chunk_tables_golden.py compares the two.  Every case runs in a fresh child process: the FCPT_*
variables of the case seed the options there, every other FCPT_* variable is removed.

Recorded per table: the row count, the SHA-256 of its int32 bytes (rows of (tile or segment, first ring, one past the
last)), and the first and last 16 rows so that a mismatch can be read.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "chunk_tables_parent.json")

# (nr, nphi, CUs, ideal EOS, damped rings at the inner end, at the outer end)
GRIDS = [(2048, 4096, 256, 0, 100, 100), (2048, 4096, 256, 1, 100, 100), (2048, 6144, 256, 0, 0, 0),
         (1024, 3072, 256, 1, 50, 50), (4096, 4096, 256, 0, 0, 0), (1367, 5462, 256, 1, 33, 33),
         (512, 1536, 256, 0, 20, 20), (128, 384, 256, 0, 0, 0), (100, 2, 256, 0, 0, 0),
         (2048, 4096, 304, 0, 100, 100), (2048, 4096, 64, 0, 0, 0), (2048, 4096, 8, 0, 0, 0),
         (2048, 4096, 256, 0, 100, 0)]
OPTIONS = ["FCPT_TRANSPORT_GRADED=0", "FCPT_TRANSPORT_ROWS=20", "FCPT_TRANSPORT_BIG=24", "FCPT_TRANSPORT_LADDER=60",
           "FCPT_TRANSPORT_FUSED=0", "FCPT_SOURCE_GRADED=0", "FCPT_SOURCE_GRADED=50", "FCPT_SOURCE_ROWS=24"]
MIN_NONEMPTY = 10  # cases with a table in the parent: the comparison must not pass on empties


def cases():
    out = [(g, "") for g in GRIDS]
    out += [(g, o) for g in GRIDS[:2] for o in OPTIONS]
    out += [(GRIDS[3], o) for o in ("FCPT_TRANSPORT_RANK_GRADE=0", "FCPT_TRANSPORT_RANK_GRADE=30")]
    return out


def case_id(grid, option):
    nr, nphi, cus, adi, di, do = grid
    return f"{nr}x{nphi}_cu{cus}_{'ideal' if adi else 'iso'}_damp{di}+{do}" + (f"_{option}" if option else "")


def _table(rows):
    flat = [v for r in rows for v in r]
    raw = (ctypes.c_int32 * len(flat))(*flat)
    return {"rows": len(rows), "sha256": hashlib.sha256(bytes(raw)).hexdigest(), "first": rows[:16], "last": rows[-16:]}


def _child(lib_path, grid):
    lib = ctypes.CDLL(lib_path)
    f = lib.fcpt_selftest_chunk_tables
    i32 = ctypes.c_int32
    nt, ns = i32(), i32()
    args = [i32(v) for v in grid]
    assert f(*args, None, i32(0), ctypes.byref(nt), None, i32(0), ctypes.byref(ns)) == 0
    t, s = (i32 * (3 * nt.value))(), (i32 * (3 * ns.value))()
    assert f(*args, t, i32(nt.value), ctypes.byref(nt), s, i32(ns.value), ctypes.byref(ns)) == 0
    rows = lambda a: [list(a[3 * k:3 * k + 3]) for k in range(len(a) // 3)]
    print(json.dumps({"transport": _table(rows(t)), "source": _table(rows(s))}))


def record(lib_path):
    """{case id: {"transport": ..., "source": ...}} from the library at lib_path, one child process per case."""
    out = {}
    for grid, option in cases():
        env = {k: v for k, v in os.environ.items() if not k.startswith("FCPT_")}
        if option:
            k, v = option.split("=")
            env[k] = v
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(lib_path), json.dumps(grid)],
                           env=env, capture_output=True, text=True, check=True)
        out[case_id(grid, option)] = json.loads(r.stdout)
    return out


def nonempty(tables):
    return sum(1 for c in tables.values() if c["transport"]["rows"] or c["source"]["rows"])


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        _child(sys.argv[2], json.loads(sys.argv[3]))
    else:
        tables = record(sys.argv[1])
        assert nonempty(tables) >= MIN_NONEMPTY, nonempty(tables)
        with open(GOLDEN, "w") as fh:
            json.dump(tables, fh, indent=0, separators=(",", ":"))
            fh.write("\n")
        print(f"{GOLDEN}: {len(tables)} cases, {nonempty(tables)} with a table")
