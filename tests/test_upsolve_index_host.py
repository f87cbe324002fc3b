"""Host-only check of csrc/rome_upsolve_index.h: the update index that every up-solve plan is launched from, the refusals of a
rome_clique_upsolve_host, and the layout of the three device arenas of rome_capi_clique.hip.

tests/c/upsolve_index_check.cpp, a stand-alone host program (no HIP), is built with ASan + UBSan and run ONCE as a child process on
all tables below (stdin); what it prints is compared with `index_ref`, a restatement of the index written from the documentation of
rome_clique_upsolve_host in include/rome_mi355.h.  The arena layouts are checked inside the program (measured size == placed size,
alignment, disjoint pieces, tables read back; the sanitizer catches a write past the block) and their sizes against `arena_ref`."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = (3, 2, 6)
TYPES = ("pose2", "point2", "pose3")
# family -> (table, target type, the family whose rows precede it in the proposal buffer of that type)
FAMILIES = {"p2p2": ("p2p2", 0, None), "br1": ("br", 0, "p2p2"), "br0": ("br", 1, None), "p3p3": ("p3p3", 2, None), "prpt2": ("prpt2", 1, "br0")}
# bytes per factor of the uploaded tables: mean, and the packed Cholesky factor (bearing-range: the two sigmas)
TABLE_BYTES = {"p2p2": (24, 48), "br": (16, 16), "p3p3": (48, 168), "prpt2": (16, 24)}

# ---- tables.  Base: poses x0..x3, landmarks l0..l2; updated x0, x1, l0; two Pose2Pose2 rows on x0 (none on x1: the family's row range
# ---- is empty for the middle update), one bearing-range row on l0
BASE = dict(N=[33], nv=[4, 3, 0], up_type=[0, 0, 1], up_var=[0, 1, 0], F_p2p2=[2], F_br=[1],
            rows_p2p2=[0, 0, 2, 0, 1, 1, 3, 0], rows_br0=[0, 0, 2, 0])
MESSAGES = dict(BASE, msg_up_pose2=[0], msg_up_point2=[2], smsg_src_pose2=[2], smsg_up_pose2=[0], smsg_src_point2=[1], smsg_up_point2=[2])
EVERY_COLUMN = dict(N=[128], nv=[4, 3, 2], F_p2p2=[2], F_br=[2], F_p3p3=[1], F_prpt2=[1],
                    rows_p2p2=[0, 0, 2, 0, 1, 1, 3, 1], rows_br1=[0, 1, 1, 1], rows_br0=[1, 0, 2, 0, 0, 0, 3, 0], rows_p3p3=[0, 2, 0, 0, 0, 1, 1, 0],
                    rows_prpt2=[0, 2, 0, 0],
                    alt_p2p2=[-1, 2], hw_p2p2=[1.0, 0.5], nh_p2p2=[0.0, 0.25], alt_br1=[2], hw_br1=[0.75], nh_br1=[0.5],
                    alt_br0=[1, -1], hw_br0=[0.5, 1.0], nh_br0=[0.0, 0.0], nh_p3p3=[0.0, 0.5],
                    sid_p2p2=[9, 4], sid_br1=[7], sid_br0=[1, 0], sid_p3p3=[3, 2], sid_prpt2=[268435455],
                    meas_p2p2=[-1, 2], meas_br1=[-1], meas_br0=[1, -1], meas_p3p3=[-1, 1])
VALID = {
    "nothing_updated": dict(N=[33], nv=[2, 1, 0]),
    "one_update_no_row": dict(N=[2], nv=[1, 0, 0], up_type=[0], up_var=[0]),
    "two_families_empty_middle_range": BASE,
    "messages_first_and_last": MESSAGES,
    "one_group": dict(BASE, up_group=[4, 4, 4]),
    "two_groups": dict(BASE, up_group=[0, 0, 1]),
    "n_up_groups": dict(BASE, up_group=[0, 1, 5]),
    "sequential": dict(BASE, schedule=[0]),
    "jacobi": dict(MESSAGES, schedule=[1]),
    "streams_and_mirrors": dict(MESSAGES, up_stream=[268435455, 0, 7], up_mirror=[2, -1, 0]),
    "mirrors_only": dict(BASE, up_mirror=[-1, 5, 0]),
    "pose3_only": dict(N=[256], nv=[0, 0, 3], up_type=[2, 2], up_var=[1, 0], F_p3p3=[2], rows_p3p3=[0, 2, 1, 1, 1, 0, 0, 1, 1, 1, 2, 0],
                       nh_p3p3=[0.0, 0.5, 0.0], meas_p3p3=[-1, 2, -1]),
    "every_family_every_column": dict(EVERY_COLUMN, up_type=[0, 2, 0, 1], up_var=[0, 0, 1, 0], up_group=[0, 0, 1, 1], msg_up_pose3=[1],
                                      smsg_src_pose3=[1], smsg_up_pose3=[1]),
}
GROUPED = dict(BASE, rows_p2p2=[0, 0, 2, 0, 1, 1, 3, 1])     # valid: one row on x0, then one on x1
REFUSED = {
    "duplicate_type_var": dict(BASE, up_var=[0, 0, 0]),
    "type_out_of_range": dict(BASE, up_type=[0, 3, 1]),
    "type_negative": dict(BASE, up_type=[0, -1, 1]),
    "var_out_of_range": dict(BASE, up_var=[0, 4, 0]),
    "row_targets_a_variable_not_updated": dict(BASE, rows_p2p2=[0, 0, 2, 0, 1, 1, 0, 3]),
    "rows_not_grouped_in_update_order": dict(BASE, rows_p2p2=[0, 0, 2, 1, 1, 1, 3, 0]),
    "up_group_decreasing": dict(BASE, up_group=[0, 1, 0]),
    "up_stream_too_large": dict(BASE, up_stream=[0, 268435456, 1]),
    "up_stream_negative": dict(BASE, up_stream=[0, 1, -1]),
    "up_mirror_below_minus_one": dict(BASE, up_mirror=[0, -2, 1]),
    "host_message_on_an_update_of_another_type": dict(MESSAGES, msg_up_pose2=[2]),
    "store_message_from_an_updated_block": dict(MESSAGES, smsg_src_pose2=[1]),
    "store_message_source_out_of_range": dict(MESSAGES, smsg_src_point2=[3]),
    "schedule_unknown": dict(BASE, schedule=[2]),
    "null_update_list": dict(N=[33], nv=[4, 3, 0], n_up=[3]),
}


def al256(b):
    return (int(b) + 255) & ~255


def family_rows(case, fam):
    return np.array(case.get("rows_" + fam, []), dtype=np.int64).reshape(-1, 4)


def index_ref(case):
    """the update index of a table, as text in the program's format.  From the header: the variables are updated in the order of the update
    list; every row targets an updated variable; a product takes the factor proposals of its variable (PriorPoint2 rows behind the
    bearing-range rows of their landmark), then the host messages, then the store-resident messages; steps follow up_group, else schedule;
    the product of the k-th updated variable of a type draws stream up_stream[k], else k."""
    up_type, up_var = case.get("up_type", []), case.get("up_var", [])
    n_up = len(up_type)
    pos_of = {(t, v): k for k, (t, v) in enumerate(zip(up_type, up_var))}
    base = {fam: (len(family_rows(case, before)) if before else 0) for fam, (_, _, before) in FAMILIES.items()}
    lines = []
    for t, name in enumerate(TYPES):
        ks = [k for k in range(n_up) if up_type[k] == t]
        n_fam = sum(len(family_rows(case, fam)) for fam, (_, vt, _) in FAMILIES.items() if vt == t)
        msg_up, smsg_up, smsg_src = (case.get(key + name, []) for key in ("msg_up_", "smsg_up_", "smsg_src_"))
        msg_base, smsg_base = n_fam, n_fam + len(msg_up)
        ptr, rows = [0], []
        for k in ks:
            for fam, (_, vt, _) in FAMILIES.items():
                if vt == t:
                    rows += [base[fam] + r for r, e in enumerate(family_rows(case, fam)) if pos_of[(t, e[3])] == k]
            rows += [msg_base + m for m, kk in enumerate(msg_up) if kk == k]
            rows += [smsg_base + m for m, kk in enumerate(smsg_up) if kk == k]
            ptr.append(len(rows))
        max_k = max([1] + list(np.diff(ptr)))
        lines.append("type %d counts %d %d %d %d %d %d" % (t, len(msg_up), msg_base, len(smsg_up), smsg_base, smsg_base + len(smsg_up), max_k))
        cols = [("up", ks), ("ptr", ptr), ("rows", rows or [0]), ("block", [up_var[k] for k in ks]),
                ("stream", [case["up_stream"][k] if "up_stream" in case else p for p, k in enumerate(ks)]),
                ("mirror", [case["up_mirror"][k] if "up_mirror" in case else -1 for k in ks]),
                ("gather", [e for p, k in enumerate(ks) for e in (DIM[t], up_var[k], p, t)]),
                ("smsg", [e for m, s in enumerate(smsg_src) for e in (DIM[t], s, smsg_base + m, t)])]
        lines += [" ".join([" " + what] + [str(int(e)) for e in v]) for what, v in cols]
    for f, (fam, (_, vt, _)) in enumerate(FAMILIES.items()):
        at = [pos_of[(vt, e[3])] for e in family_rows(case, fam)]
        lines.append(" ".join(["fam %d base %d lo" % (f, base[fam])] + [str(sum(a < k for a in at)) for k in range(n_up + 1)]))
    if "up_group" in case:
        g = case["up_group"]
        steps = [0] + [k for k in range(1, n_up) if g[k] != g[k - 1]] + [n_up]
    else:
        steps = [0] + (list(range(1, n_up)) if case.get("schedule", [0])[0] == 0 else []) + [n_up]
    lines.append(" ".join(["step_k"] + [str(k) for k in steps]))
    lines.append(" ".join(["up_cnt_before"] + [str(sum(tt == t for tt in up_type[:k])) for k in range(n_up + 1) for t in range(3)]))
    lines.append("flags %d %d %d" % (n_up, "up_mirror" in case, "up_stream" in case))
    return lines


def family_table_bytes(case, fam):
    n, (table, _, _) = len(family_rows(case, fam)), FAMILIES[fam]
    if n == 0:
        return 0
    F = case["F_" + table][0]
    cols = sum(al256(n * w) for key, w in (("alt_", 4), ("hw_", 8), ("nh_", 8), ("sid_", 4), ("meas_", 4)) if key + fam in case)
    return al256(n * 16) + al256(F * TABLE_BYTES[table][0]) + al256(F * TABLE_BYTES[table][1]) + cols


def arena_ref(case):
    """bytes of the three arenas: every piece rounded up to 256 bytes, nothing else"""
    N, nv = case["N"][0], case["nv"]
    store = sum(al256(nv[t] * DIM[t] * N * 8) for t in range(3))
    tables = sum(family_table_bytes(case, fam) for fam in FAMILIES)
    proposals = store + tables + sum(al256(len(family_rows(case, fam)) * DIM[vt] * N * 8) for fam, (_, vt, _) in FAMILIES.items())
    plan = tables
    for t, name in enumerate(TYPES):
        nu = sum(tt == t for tt in case.get("up_type", []))
        n_smsg = len(case.get("smsg_up_" + name, []))
        prop = sum(len(family_rows(case, fam)) for fam, (_, vt, _) in FAMILIES.items() if vt == t) + len(case.get("msg_up_" + name, [])) + n_smsg
        csr = max(1, prop)            # (every row enters exactly one product; an empty list is uploaded as one entry)
        plan += al256(prop * DIM[t] * N * 8) + al256(prop * DIM[t] * 8) + al256(nu * DIM[t] * N * 8) + al256(nu * DIM[t] * 8) + \
            al256((nu + 1) * 4) + al256(csr * 4) + 3 * al256(nu * 4) + al256(nu * 16) + al256(n_smsg * 16)
    return {"store": store, "plan": plan, "proposals": proposals}


def as_text(name, case):
    return "case %s\n%s\nend\n" % (name, "\n".join("%s %d %s" % (k, len(v), " ".join(repr(e) for e in v)) for k, v in case.items()))


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{case name: the lines the program printed for it}, from one build and one run"""
    exe = str(tmp_path_factory.mktemp("upsolve_index") / "upsolve_index_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "c", "upsolve_index_check.cpp"), "-o", exe])
    cases = dict(VALID, grouped_rows=GROUPED, **REFUSED)
    cases["proposals_every_family_every_column"] = dict(EVERY_COLUMN, proposals=[1])
    cases["too_many_particles_and_schedule_unknown"] = dict(REFUSED["schedule_unknown"], N=[257])
    out = subprocess.run([exe], input="".join(as_text(k, v) for k, v in cases.items()), capture_output=True, text=True)
    assert out.returncode == 0 and "upsolve_index_check ok: %d cases, 0 faults" % len(cases) in out.stdout, out.stdout + out.stderr
    by_case = {}
    for line in out.stdout.splitlines():
        if line.startswith("case "):
            cur = by_case.setdefault(line[5:], [])
        elif not line.startswith("upsolve_index_check"):
            cur.append(line)
    assert sorted(by_case) == sorted(cases)
    return by_case


@pytest.mark.parametrize("name", sorted(VALID) + ["grouped_rows"])
def test_index_of_a_valid_table(printed, name):
    case = dict(VALID, grouped_rows=GROUPED)[name]
    want = arena_ref(case)
    got = printed[name]
    assert got[0] == "rc 0"
    assert got[1:-2] == index_ref(case)
    assert got[-2].startswith("arena store ok need %d pieces" % want["store"]), got[-2]
    assert got[-1].startswith("arena plan ok need %d pieces" % want["plan"]), got[-1]


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_table_wrong_in_exactly_one_way_is_refused(printed, name):
    assert printed[name] == ["rc -1"]                       # ROME_ERR_INVALID_ARG, and nothing laid out


def test_particle_limit_is_reported_before_anything_else(printed):
    """N above ROME_MAX_PARTICLES_GIBBS (256) is ROME_ERR_UNSUPPORTED_N, also for a table that is wrong as well"""
    assert printed["too_many_particles_and_schedule_unknown"] == ["rc -5"]


def test_proposals_arena_with_every_family_and_every_column(printed):
    want = arena_ref(EVERY_COLUMN)
    got = printed["proposals_every_family_every_column"]
    assert len(got) == 1 and got[0].startswith("arena proposals ok need %d pieces" % want["proposals"]), got
