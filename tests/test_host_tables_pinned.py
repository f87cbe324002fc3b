"""The host packing (graph.PackedGraph, device.DeviceGraph's family records, clique.CliqueBatch / fill_upsolve_plan, the refusals),
pinned without a GPU against tests/golden/host_tables.json.

The fixture is the output of scripts/host_tables_fingerprint.py at the commit BEFORE the table builders were folded (one builder per
row shape, every column always): the script was copied into a checkout of that commit and run there.  It is NOT produced by the code
under test.  Arrays are compared by a digest of dtype, shape and bytes.

(a) every column of every PackedGraph table that the recording holds is unchanged; a column the recording does not hold is one of
    the hypothesis columns and holds its absent value throughout (alt -1, w 1, w2 0, nh 0);
(b) the plan-only DeviceGraph of the four graphs that tests/golden/device_graph_plans.json does not cover: `describe()` of
    test_device_graph_plan.py plus each record's entry, stream, partial, prop_lo, the scalars of `tab` and the fused / unfused lists;
(c) every field of the rome_clique_host that CliqueBatch._fill writes (clique-local arrays) and of the rome_clique_upsolve_host that
    plan_level + fill_upsolve_plan write for every logged level of four tree solves (store-addressed), with the batch's row lists;
(d) the refusals: exception type and whole message at each of the five sites."""
import importlib.util
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_spec = importlib.util.spec_from_file_location("host_tables_fingerprint", os.path.join(ROOT, "scripts", "host_tables_fingerprint.py"))
HT = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(HT)

with open(os.path.join(ROOT, "tests", "golden", "host_tables.json")) as _f:
    GOLDEN = json.load(_f)

ABSENT = {"alt": -1, "w": 1, "w2": 0, "nh": 0}


def _plain(x):
    return json.loads(json.dumps(x))


def test_the_pinned_cases_are_the_scripts_cases():
    assert sorted(GOLDEN["packed"]) == sorted(HT.PACKED_GRAPHS) and len(HT.PACKED_GRAPHS) == 12
    assert sorted(GOLDEN["device"]) == sorted(HT.DEVICE_GRAPHS) and sorted(GOLDEN["clique"]) == sorted(HT.CLIQUE_LOCAL)
    assert sorted(GOLDEN["upsolve"]) == sorted(HT.UPSOLVE)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", HT.PACKED_GRAPHS)
def test_packed_tables_are_what_they_were(name):
    pk = HT.packed(name)
    got, want = _plain(HT.packed_tables(pk)), GOLDEN["packed"][name]
    assert sorted(got) == sorted(want)
    for table in HT.TABLES:
        for col, w in want[table].items():
            assert col in got[table] and got[table][col] == w, (table, col)
        for col in set(got[table]) - set(want[table]):      # a column the tables did not always carry: absent-valued throughout
            v = getattr(pk, table)[col]
            assert col in ABSENT and v.shape == (want[table]["F"],) and np.all(v == ABSENT[col]), (table, col)
            assert v.dtype == (np.int32 if col == "alt" else np.float64), (table, col)
    for key in ("N", "index", "labels"):
        assert got[key] == want[key], key


def test_every_relative_table_carries_the_hypothesis_columns():
    pk = HT.packed("pose2_tables")
    for table in ("p2p2", "p3p3", "p3xyy", "p3rot"):
        assert set(ABSENT) <= set(getattr(pk, table)), table
    assert "nh" in pk.br and GOLDEN["packed"]["pose2_tables"]["p2p2"].keys() & set(ABSENT) == set()
    nh = HT.packed("bearing_only").pbear["nh"]
    assert nh.tolist() == [0.0, 0.25, 0.0]                                 # (the recorded graphs do carry hypotheses where they say)
    assert HT.packed("partial3").p3rot["nh"].tolist() == [0.25] and (HT.packed("beehive_mh").p2p2["alt"] >= 0).sum() == 1


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("name", HT.DEVICE_GRAPHS)
def test_device_graph_layout_is_what_it_was(name):
    got, want = HT.device_layout(name), GOLDEN["device"][name]
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_lean_kernels_stay_selected():
    """no multihypo row -> alt = w = None; nh all zero -> nh = None (the null pointers select the lean kernels)"""
    for name in ("pose2_tables", "prior_only"):
        fam = GOLDEN["device"][name]["families"]
        assert fam["p2p2"]["null"] == ["alt", "w", "nh"] and HT.device_layout(name)["families"]["p2p2"]["null"] == ["alt", "w", "nh"]


# ------------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("name", HT.CLIQUE_LOCAL)
def test_clique_host_fields_are_what_they_were(name):
    got, want = _plain(HT.clique_local(name)), GOLDEN["clique"][name]
    for key in ("rows", "fam_rows", "fam_hyp", "fam_sid", "fam_meas", "vars"):
        assert got[key] == want[key], key
    assert sorted(got["struct"]) == sorted(want["struct"])
    for field, w in want["struct"].items():
        assert got["struct"][field] == w, field


def test_clique_cases_take_every_family_and_hypothesis_column():
    st = {name: g["struct"] for name, g in GOLDEN["clique"].items()}
    assert all(st["beehive_mh"][f + "_alt"] and st["beehive_mh"][f + "_hypo_w"] for f in ("p2p2", "br1", "br0"))
    assert all(st["bearingrange_nullhypo"][f + "_nullhypo"] for f in ("p2p2", "br1", "br0"))
    assert st["landmark_prior_frozen"]["n_prpt2"] == 1 and st["helix3d"]["n_p3p3"] > 0 and st["helix3d"]["n_pose3"] == 24
    assert any(row[1] == 2 for row in GOLDEN["clique"]["helix3d"]["fam_rows"]["p3p3"])           # its PriorPose3 row


@pytest.mark.parametrize("case", HT.UPSOLVE)
def test_upsolve_host_fields_are_what_they_were(case):
    got, want = HT.upsolve_steps(case), GOLDEN["upsolve"][case]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for key in w:
            assert g[key] == w[key], "%s: %s of step %d of %d differs" % (case, key, k, len(want))


def test_error_paths_are_what_they_were():
    want = GOLDEN["errors"]
    assert HT.error_paths() == want
    assert [want[k][0] for k in ("sampled_without_store", "sampled_multihypo", "target_not_on_factor")] == ["TypeError", "TypeError", "KeyError"]


# ------------------------------------------------------------------------------------------------ (d)
def test_refusals_are_what_they_were():
    got, want = HT.refusals(), GOLDEN["refusals"]
    assert sorted(want) == ["bearing", "bearing_then_range", "partial3", "range"]
    for kind in want:
        assert sorted(want[kind]) == ["CliqueBatch", "DeviceStore", "TreeSolver", "initAllOrdered", "solveTree"]
        for site, w in want[kind].items():
            assert w is not None and w[0] == "TypeError" and w[1].startswith(site + ": ")
            assert got[kind][site] == w, (kind, site)
    assert all("Pose2Point2Range" in w[1] for w in want["bearing_then_range"].values())     # range is refused first
