"""The step loop launches what it launched when tests/golden/launch_census.json was recorded: per case (tests/launch_census.py)
the per-kernel launch counts, the graph-replay counters, the clock and the sha256 of Sigma, v_r, v_phi, e, Q+ and Q-
are those of the record, exactly.  The record was written once, by `python -m tests.launch_census --record`, from a
build of the commit before the launch decisions moved into fcpt_plan.cpp; the host code between the kernels can be
rearranged freely while this holds, and a change that means to alter a launch sequence re-records the cases it
alters and says so.

A case listed under "unstable" in the record did not reproduce its own digests on the recording build: it is held to
counts (or graph counters) and clock only."""
import json
import os

import pytest

from tests import launch_census as LC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_census.json")
MAX_UNSTABLE = 2


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_record_holds_every_case(golden):
    assert sorted(golden["cases"]) == sorted(LC.CASES)
    assert len(golden["unstable"]) <= MAX_UNSTABLE, golden["unstable"]
    for name, rec in golden["cases"].items():
        assert "error" not in rec, (name, rec)
        assert ("counts" in rec) != ("graph" in rec), name
        assert (rec["digests"] is None) == (name in golden["unstable"]), name


@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_case_launches_what_the_record_says(product, golden, name):
    want = golden["cases"][name]
    got = LC.run_case(product, name)
    print(name, json.dumps(got, sort_keys=True))
    if "counts" in want:
        assert got["counts"] == want["counts"]
    else:
        assert got["graph"] == want["graph"]   # [graph_cycle, graph_replays]
    assert got["clock"] == want["clock"]
    if want["digests"] is not None:
        assert got["digests"] == want["digests"]
