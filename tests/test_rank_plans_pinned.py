"""The multi-rank drivers without a GPU or a process group: what SeparatorPipeline, TargetShardedSweep and FrontierShard.plan lay out
over plan-only DeviceGraphs of the fixture graphs of test_device_graph_plan.py equals tests/golden/rank_plans.json, key by key.

The fixture is the output of scripts/rank_plan_fingerprint.py at the commit BEFORE the drivers were folded onto one all-gather, one
launch-keyword builder and one plan per TargetShardedSweep (five hand-written exchanges, the rome_conv_dev keywords assembled in three
places).  It is NOT produced by the code under test: arena layout, ghost blocks, stream offsets, the null-ness of the optional columns
and every index tensor are what that commit handed to its launches."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import rank_plan_fingerprint as F   # noqa: E402

FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "rank_plans.json")))
CASES = F.cases()


def test_fixture_and_script_name_the_same_cases():
    assert sorted(FIXTURE) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_rank_plan_equals_the_recorded_one(case):
    want = FIXTURE[case]
    got = json.loads(json.dumps(CASES[case]()))
    assert sorted(got) == sorted(want)
    for key in want:
        if key == "plans":   # SeparatorPipeline: name the slot and the family that differ
            assert len(got[key]) == len(want[key])
            for b, (gb, wb) in enumerate(zip(got[key], want[key])):
                assert len(gb) == len(wb), b
                for k, (gp, wp) in enumerate(zip(gb, wb)):
                    for field in wp:
                        assert gp[field] == wp[field], (b, k, field)
        else:
            assert got[key] == want[key], key


def test_fixture_takes_every_branch():
    fx = FIXTURE
    plans = lambda case: [p for slot in fx[case]["plans"] for p in slot]   # noqa: E731
    by_entry = lambda case: {p["entry"] + str(p["ints"]["dir_all"]): p for p in fx[case]["plans"][0]}   # noqa: E731
    # SeparatorPipeline: three families; every optional column null and non-null; Pose3; a depth-3 slot; ghosts move rows
    hexa = fx["pipeline/hexagon/world3/rank1/depth3"]
    assert hexa["families"] == ["p2p2", "br1", "br0"] and len(hexa["plans"]) == 3 and all(len(s) == 3 for s in hexa["plans"])
    assert all(p["null"] == ["alt_var", "hypo_w", "nullhypo"] for p in plans("pipeline/hexagon/world3/rank1/depth3"))
    assert all(p["null"] == ["nullhypo"] for p in plans("pipeline/beehive_mh/world3/rank0/depth2"))
    assert all(p["null"] == ["alt_var", "hypo_w"] for p in plans("pipeline/bearingrange_nullhypo/world1/rank0/depth2"))
    assert fx["pipeline/helix3d/world3/rank2/depth2"]["families"] == ["p3p3"] and list(fx["pipeline/helix3d/world3/rank2/depth2"]["store"]) == ["Pose3"]
    for g in F.PIPE_GRAPHS:   # slot 0 and slot 1 address different receive buffers: the remapped columns differ
        s0, s1 = fx["pipeline/%s/world3/rank0/depth2" % g]["plans"]
        assert all(a["digests"]["rows4"] != b["digests"]["rows4"] for a, b in zip(s0, s1)), g
    bee0, bee1 = (fx["pipeline/beehive_mh/world3/rank0/depth2"]["plans"][b] for b in (0, 1))
    assert all(a["digests"]["alt_var"] != b["digests"]["alt_var"] for a, b in zip(bee0, bee1))   # the alternative column follows the ghost
    p = by_entry("pipeline/hexagon/world1/rank0/depth2")["rome_conv_pose2point2br_dev0"]
    assert p["views"]["bel_fixed"][0] == p["views"]["bel_target"][0] == "arena" and p["views"]["mirror_out"][0] == "send0" and p["views"]["out"][0] == "out0.br0"
    # TargetShardedSweep: ranks without rows, every optional column null and non-null
    empty = [c for c in fx if c.startswith("shard/") and fx[c]["n_rows"] == 0]
    assert empty and all(fx[c]["plan"] is None for c in empty) and all("/world8/" in c for c in empty)
    assert fx["shard/manhattan_prefix/world3/rank1"]["plan"]["null"] == ["alt_var", "hypo_w", "nullhypo", "mirror_map", "mirror_out"]
    assert fx["shard/beehive_mh/world2/rank1"]["plan"]["null"] == ["nullhypo", "mirror_map", "mirror_out"]
    assert fx["shard/bearingrange_nullhypo/world2/rank0"]["plan"]["null"] == ["alt_var", "hypo_w", "mirror_map", "mirror_out"]
    for c in fx:
        if c.startswith("shard/") and fx[c]["plan"] is not None:
            pl = fx[c]["plan"]
            assert pl["stream_offset"] == F.STREAM0 + fx[c]["row_lo"] and pl["ints"]["n_conv"] == fx[c]["n_rows"] == fx[c]["row_hi"] - fx[c]["row_lo"]
            assert pl["views"]["out"] == ["prop", fx[c]["row_lo"] * 3 * F.N, fx[c]["n_rows"] * 3 * F.N]
    # FrontierShard: an empty share (nothing to up-solve), no scatter at world 1 unless the collective is forced
    assert fx["frontier/two/world3/rank2/plain"]["mirror"] is None and fx["frontier/two/world3/rank2/plain"]["scatter"] is not None
    assert fx["frontier/level0/world1/rank0/plain"]["scatter"] is None and fx["frontier/level0/world1/rank0/collective"]["scatter"] is not None
    assert fx["frontier/level1/world2/rank1/plain"]["send"][1] == fx["frontier/level1/world2/rank1/plain"]["width"] * F.N
