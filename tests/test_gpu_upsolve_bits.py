"""rome_clique_proposals, rome_clique_upsolve and the up-solve plans are held to the bytes they returned before their host side was
rebuilt around one update index and one arena layout (csrc/rome_upsolve_index.h): the cases of scripts/upsolve_bits.py -- a Pose2
chain through DeviceStore + UpsolvePlan; poses and landmarks with forked phases, host and store-resident messages, stream ids and host
outputs; a Pose3 pair; mirrors at both strides; the one-shot entry in AoS; all five families of the proposals entry."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_upsolve_output_bits_are_the_recorded_ones():
    """tests/golden/upsolve_bits.json was written by scripts/upsolve_bits.py on an MI355X from the library of commit 89975eb, the last
    one in which plan_build sized and carved its arena by hand; two recordings (separate processes) were equal, forked steps included."""
    spec = importlib.util.spec_from_file_location("upsolve_bits", os.path.join(ROOT, "scripts", "upsolve_bits.py"))
    UB = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(UB)
    with open(os.path.join(ROOT, "tests", "golden", "upsolve_bits.json")) as f:
        want = json.load(f)["sha256"]
    got = UB.hashes()
    assert sorted(got) == sorted(want) and len(got) == 7 * len(UB.SHAPES_N)
    diff = [k for k in got if got[k] != want[k]]
    assert not diff, diff
