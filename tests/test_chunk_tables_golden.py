"""The chunk tables of the marching kernels (fcpt_schedule.cpp), byte for byte those of the commit before the planner
left the HIP unit: tests/golden/chunk_tables_parent.json, written by tests/golden/make_chunk_table_golden.py from a
build of that commit.  Host logic, no GPU."""
import importlib.util
import json
import os

import pytest

import fargocpt_amd

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_chunk_table_golden", os.path.join(HERE, "golden", "make_chunk_table_golden.py"))
golden = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(golden)

with open(golden.GOLDEN) as _fh:
    PARENT = json.load(_fh)


@pytest.fixture(scope="module")
def tables(product):
    return golden.record(fargocpt_amd.LIB_PATH)


def test_the_golden_file_holds_every_case_and_enough_tables():
    assert sorted(PARENT) == sorted(golden.case_id(g, o) for g, o in golden.cases())
    assert golden.nonempty(PARENT) >= golden.MIN_NONEMPTY


@pytest.mark.parametrize("case", sorted(PARENT))
def test_chunk_tables_equal_the_parent_commits(tables, case):
    for which in ("transport", "source"):
        for field in ("rows", "first", "last", "sha256"):
            assert tables[case][which][field] == PARENT[case][which][field], (case, which, field)
