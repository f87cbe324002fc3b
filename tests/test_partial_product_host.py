"""The partial-aware product on the host side: the two references of tests/partial_product_ref.py check one another and
the CPU conditions of the margin rule hold for every table; the task builder (device.partial_tasks) on the graphs that need it; the
default stays what it was; header, ctypes table and Julia wrapper agree.  Runs without a GPU.  Run with -s, it prints the reference-side
error figures recorded in partial_product_ref's docstring."""
import math
import os
import re

import numpy as np
import pytest

import partial_product_ref as PP
import rome_jl_amd as R
from rome_jl_amd.factors import partial_coverage
from test_julia_shim_static import c_prototypes, jl_source, _call_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_CEILING = 8.0 * PP.EPS
TABLES = dict(PP.all_tables())


# ------------------------------------------------------------------ the references
def test_tables_cover_the_launch_shapes():
    src = open(os.path.join(ROOT, "rome.jl_amd", "csrc", "rome_product_partial.hip")).read()
    assert int(re.search(r"constexpr int kCoordMaxN = (\d+);", src).group(1)) == PP.MAXN == max(PP.SHAPE_N) == R._lib.MAX_PARTICLES_PRODUCT
    assert set(PP.SHAPE_N) >= {1, 2, 63, 64, 65, 128, 129, 256, 257, 512}        # S = 1, 2, 4, 8 at their emptiest and full
    for D in PP.DIMS:
        t = PP.shape_table(D, 65, PP.SILVERMAN)
        tk = t["tasks"]
        M = [PP._n_dens(t, k) for k in range(len(tk["task_var"]))]
        assert set(M) >= ({1, 2, 3, 9}), (D, M)
        assert {int(j) for j in tk["task_joint"]} == {0, 1}
        per_var = np.bincount(tk["task_var"], minlength=t["V"])
        assert per_var.max() >= 2 and per_var.min() == 0                         # two tasks on one variable, a variable without any
        lines = {(int(v), int(c)) for v, c in zip(tk["task_var"], tk["task_coord"])}
        assert len(lines) == len(tk["task_var"])                                 # one owner per line
        assert any((v, c) not in lines for v in set(tk["task_var"].tolist()) for c in range(D))   # an untouched line beside a task
        circ = [bool((t["circ"] >> c) & 1) for c in tk["task_coord"]]
        assert (D == 2 and not any(circ)) or (any(circ) and not all(circ))
        # rows: a permutation with unused rows in between; pass-through lines are NaN
        assert len(set(tk["task_rows"].tolist())) < t["n_rows"] and (np.diff(tk["task_rows"]) < 0).any()
        for r, cov in t["cover"].items():
            assert all(np.isnan(t["prop"][r, c]).all() != (c in cov) for c in range(D))
        if D >= 3:                                                               # circular clusters with points on both sides of ±π
            ks = [k for k in range(len(circ)) if circ[k] and M[k] >= 2]
            assert any(min(x.min() for x in PP.densities(t, k)[0]) < -3.0 and max(x.max() for x in PP.densities(t, k)[0]) > 3.0 for k in ks)
    assert PP.shape_table(3, 65, PP.SILVERMAN)["stream_offset"] > 2 ** 32


@pytest.mark.parametrize("D", PP.DIMS)
def test_np_task_against_mp(D):
    kinds = set()
    for name, mk in TABLES.items():
        t = mk()
        if t["D"] != D or not t["mp_tasks"]:
            continue
        ref = PP.reference(name, True)
        kinds.add((t["key"][0], t["mode"]))
        for k in t["mp_tasks"]:
            r, m = ref.res[k], ref.mp[k]
            assert m["base"] == r["base"] and list(r["picks"]) == m["picks"], (name, k)
            # a double difference of two angles on either side of ±π is rounded at ulp(2π)/2 = 2 eps BEFORE it is wrapped (in any double
            # evaluation, the kernel's included; mp subtracts exactly): relative 2 eps / sd = 2 eps·c_N / h on a Silverman bandwidth, and
            # |d| / h · 2 eps / h on a log-weight term, |d| / h <= sqrt(2·scale_w)
            wrap_h = 2.0 * PP.EPS * PP.silverman_factor(t["N"]) / r["h"] if r["circ"] and t["mode"] == PP.SILVERMAN else 0.0
            wrap_w = math.sqrt(2.0 * r["scale_w"]) * 2.0 * PP.EPS / r["h"].min() + 2.0 * r["scale_w"] * np.max(wrap_h) if r["circ"] else 0.0
            assert (np.abs(np.array([float(x) for x in m["h"]]) / r["h"] - 1.0) <= DEV_CEILING + wrap_h).all()
            assert np.abs(np.array([float(x) for x in m["logw"]]) - r["logw"]).max() <= (DEV_CEILING * r["scale_w"] + wrap_w) * r["M"]
        print("PARTREF cpu %-28s dev_c %.2f eps  dev_out %.2f eps  (scale_w %.1e, %d mp tasks)"
              % (name, ref.dev["c"] / PP.EPS, ref.dev["out"] / PP.EPS, ref.scale_w, len(t["mp_tasks"])))
        assert ref.dev["c"] <= DEV_CEILING and ref.dev["out"] <= DEV_CEILING, (name, ref.dev)
    assert kinds == {("shape", PP.SILVERMAN), ("shape", PP.SUPPLIED), ("zero", PP.SILVERMAN), ("far", PP.SUPPLIED), ("tie", PP.SUPPLIED)}


@pytest.mark.parametrize("D", PP.DIMS)
def test_margin_conditions_of_every_table(D):
    """every particle of every table is decided: min g >= 1000 δ and the base is decided (or tied bit for bit, lowest l)"""
    dev_c = max(PP.reference(n, True).dev["c"] for n, mk in TABLES.items() if mk()["mp_tasks"])
    draws = 0
    for name, mk in TABLES.items():
        t = mk()
        if t["D"] != D:
            continue
        ref = PP.reference(name)
        assert ref.conditions(dev_c) == [], name
        live = [r for r in ref.res if r["M"] >= 2]
        draws += t["N"] * len(live)
        assert all(np.isfinite(r["out"]).all() for r in live)
        fig, bad = ref.check(ref.expected())                                     # the checker accepts the definition's own output ...
        assert bad == [], (name, bad)
        if live and t["N"] >= 63:                                                # ... and refuses a neighbouring pick and a line left alone
            k = next(k for k, r in enumerate(ref.res) if r["M"] >= 2)
            v, c = int(t["tasks"]["task_var"][k]), int(t["tasks"]["task_coord"][k])
            wrong = ref.expected()
            r = ref.res[k]
            i = int(np.argmax(r["X"][np.minimum(r["picks"] + 1, t["N"] - 1)] != r["X"][r["picks"]]))
            wrong[v, c, i] = r["X"][min(r["picks"][i] + 1, t["N"] - 1)] + r["hp"] * r["xi"][i]
            assert any(b[0] in ("pick", "output") for b in ref.check(wrong)[1]), name
            assert ref.check(t["bel"])[1] != [], name
    print("PARTREF cpu D=%d: %d output particles decided" % (D, draws))


def test_special_tables_do_what_they_are_for():
    for D in PP.DIMS:
        z = PP.reference("zero D=%d" % D)
        assert all(r["base"] == 0 and r["h"][0] == PP.FLOOR and (r["h"][1:] > 1e-3).all() for r in z.res)
        f = PP.reference("far D=%d" % D)
        for k, r in enumerate(f.res):
            assert r["base"] == r["M"] - 1 and r["scale_w"] > 0.4 * PP.FAR ** 2   # exp(−½·1000²) = 0 in double: only the running maximum saves it
            assert bool(f.table["tasks"]["task_joint"][k]) == (k >= 2)            # the base is the joint line on the last four tasks
        ti = PP.reference("tie D=%d" % D)
        assert all(r["base"] == 0 and len(set(r["h"].tolist())) == 1 for r in ti.res) and all(eq for _, eq in ti.hgap)
        one = PP.reference("shape D=%d N=1 %s" % (D, PP.SILVERMAN))                # N = 1: every h is the floor, base l = 0
        assert all(r["M"] == 1 or (r["base"] == 0 and set(r["h"].tolist()) == {PP.FLOOR}) for r in one.res)


# ------------------------------------------------------------------ coverage and the task builder
def test_partial_coverage_from_the_class_attributes():
    assert partial_coverage(R.Pose3Pose3XYYaw, 0) == partial_coverage(R.Pose3Pose3XYYaw, 1) == (0, 1, 5)
    assert partial_coverage(R.PriorPose3ZRP, 0) == (2, 3, 4)
    assert partial_coverage(R.Pose2Point2Range, 0) == (0, 1) and partial_coverage(R.Pose2Point2Range, 1) is None
    f = R.Pose2Point2Range(R.Normal(3.0, 0.1))
    assert partial_coverage(f, 0) == (0, 1)
    for cls in (R.Pose2Pose2, R.PriorPose2, R.Pose2Point2BearingRange, R.Pose3Pose3, R.PriorPose3, R.Point2Point2Range, R.Pose2Point2Bearing):
        assert all(partial_coverage(cls, k) is None for k in range(len(cls.variable_types))), cls


def _zero_init(fg):
    for l, t in fg.variables.items():
        fg.initVariable(l, np.zeros((t.dim, fg.N)))
    return fg


def _chain_graph(N):
    """test/testPartialPose3.jl:455-501, the sigma_RP = 0 graph (as tests/test_gpu_partial3.py builds it)"""
    fg = R.initfg(N=N)
    for i in range(5):
        fg.addVariable("x%d" % i, R.Pose3)
    fg.addFactor(["x0"], R.PriorPose3(R.MvNormal(np.zeros(6), np.diag([0.1, 0.1, 0.1, 0.01, 0.01, 0.01]) ** 2)))
    for i in range(1, 5):
        fg.addFactor(["x%d" % i], R.PriorPose3ZRP(R.Normal(float(i), 0.1), R.MvNormal([0.0, 0.0], np.diag([0.01, 0.01]) ** 2)))
    for i in range(1, 5):
        fg.addFactor(["x%d" % (i - 1), "x%d" % i], R.Pose3Pose3XYYaw(R.MvNormal([10.0, 0.0, math.pi / 2], np.diag([0.1, 0.1, 0.01]) ** 2)))
    return fg


def _range_graph(N, with_prior=False):
    """one pose seen from three landmarks by range only"""
    fg = R.initfg(N=N)
    fg.addVariable("x0", R.Pose2)
    for k, xy in enumerate(([10.0, 0.0], [0.0, 10.0], [-7.0, -7.0])):
        fg.addVariable("l%d" % k, R.Point2)
        fg.addFactor(["l%d" % k], R.PriorPoint2(R.MvNormal(xy, np.eye(2) * 0.01)))
        fg.addFactor(["x0", "l%d" % k], R.Pose2Point2Range(R.Normal(float(np.hypot(*xy)), 0.1)))
    if with_prior:
        fg.addFactor(["x0"], R.PriorPose2(R.MvNormal(np.zeros(3), np.eye(3) * 0.01)))
    return fg


# rows of prop[Pose3] on the chain: 0 the PriorPose3 of x0; 1 .. 8 the XYYaw rows (2f + dir: towards x_{f+1}, then towards x_f);
# 9 .. 12 the ZRP rows of x1 .. x4
CHAIN_PTR = [0, 2, 5, 8, 11, 13]
CHAIN_ROWS = [0, 2, 1, 4, 9, 3, 6, 10, 5, 8, 11, 7, 12]


def _chain_tasks_expected():
    xy = {0: [2], 1: [1, 4], 2: [3, 6], 3: [5, 8], 4: [7]}
    var, coord, rows, joint, ptr = [], [], [], [], [0]
    for v in range(5):
        for c in range(6):
            r = xy[v] if c in (0, 1, 5) else ([8 + v] if v >= 1 else [])
            if r:
                var.append(v); coord.append(c); rows += r; joint.append(1 if v == 0 else 0); ptr.append(len(rows))
    return var, coord, ptr, rows, joint


def test_partial_tasks_on_the_chain_graph():
    dg = R.DeviceGraph(_zero_init(_chain_graph(16)), plan_only=True)
    assert {n: r["partial"] for n, r in dg.fams.items()} == {"p3p3": None, "prior3": None, "p3xyy": (0, 1, 5), "zrp3": (2, 3, 4)}
    assert dg._prop_cover[R.Pose3] == [None] + [(0, 1, 5)] * 8 + [(2, 3, 4)] * 4
    c = dg.csr[R.Pose3]
    assert c["ptr_h"].tolist() == CHAIN_PTR and c["rows_h"].tolist() == CHAIN_ROWS
    pt = dg.tasks[R.Pose3]["host"]
    var, coord, ptr, rows, joint = _chain_tasks_expected()
    assert pt["full_ptr"].tolist() == [0, 1, 1, 1, 1, 1] and pt["full_rows"].tolist() == [0]
    assert (pt["task_var"].tolist(), pt["task_coord"].tolist(), pt["task_ptr"].tolist(), pt["task_rows"].tolist(), pt["task_joint"].tolist()) \
        == (var, coord, ptr, rows, joint)
    assert dg.tasks[R.Pose3]["T"] == 27 and dg.tasks[R.Pose3]["any_joint"]       # x0: 3 lines, x1 .. x4: 6 each
    assert all(a.dtype == np.int32 for a in pt.values())
    f = dg.csr_full[R.Pose3]
    assert f["ptr"].tolist() == [0, 1, 1, 1, 1, 1] and f["rows"].tolist() == [0] and f is not c
    for vt in (R.Pose2, R.Point2):                                               # no variables of these types: no tasks, the CSR of today
        assert dg.tasks[vt]["T"] == 0 and dg.csr_full[vt] is dg.csr[vt]
    # the pure function gives the same from the plain CSR
    again = R.partial_tasks(CHAIN_PTR, CHAIN_ROWS, dg._prop_cover[R.Pose3], 6)
    assert all(np.array_equal(again[k], pt[k]) for k in pt)


def test_partial_tasks_three_ranges_no_full_row():
    dg = R.DeviceGraph(_zero_init(_range_graph(16)), plan_only=True)
    assert dg.fams["pprng1"]["partial"] == (0, 1) and dg.fams["pprng0"]["partial"] is None and dg.fams["priorpt2"]["partial"] is None
    pt = dg.tasks[R.Pose2]["host"]
    rows = dg.csr[R.Pose2]["rows_h"].tolist()
    assert len(rows) == 3
    assert pt["task_var"].tolist() == [0, 0] and pt["task_coord"].tolist() == [0, 1] and pt["task_joint"].tolist() == [0, 0]
    assert pt["task_ptr"].tolist() == [0, 3, 6] and pt["task_rows"].tolist() == rows + rows      # the heading has no task
    assert pt["full_ptr"].tolist() == [0, 0] and not dg.tasks[R.Pose2]["any_joint"]
    # the landmarks: range rows towards a landmark and the landmark priors are full -> no tasks, stage 1 on the tables of today
    assert dg.tasks[R.Point2]["T"] == 0 and dg.csr_full[R.Point2] is dg.csr[R.Point2]
    assert np.diff(dg.csr[R.Point2]["ptr_h"]).tolist() == [2, 2, 2]
    # with a prior on the pose: one full row, joint = 1
    dg1 = R.DeviceGraph(_zero_init(_range_graph(16, with_prior=True)), plan_only=True)
    p1 = dg1.tasks[R.Pose2]["host"]
    assert p1["task_joint"].tolist() == [1, 1] and np.diff(p1["full_ptr"]).tolist() == [1] and np.diff(p1["task_ptr"]).tolist() == [3, 3]


def test_partial_tasks_full_rows_only_and_frozen():
    cover = [None, (0, 1), None, (2,), (0, 1)]
    pt = R.partial_tasks([0, 2, 4, 5], [0, 2, 1, 3, 4], cover, 3)                # v0: rows 0, 2 (full only); v1: rows 1, 3; v2: row 4
    assert pt["task_var"].tolist() == [1, 1, 1, 2, 2] and pt["task_coord"].tolist() == [0, 1, 2, 0, 1]
    assert pt["task_rows"].tolist() == [1, 1, 3, 4, 4] and pt["task_joint"].tolist() == [0] * 5
    assert pt["full_ptr"].tolist() == [0, 2, 2, 2] and pt["full_rows"].tolist() == [0, 2]
    empty = R.partial_tasks([0, 1, 2], [0, 1], [None, None], 2)
    assert len(empty["task_var"]) == 0 and empty["task_ptr"].tolist() == [0] and empty["full_rows"].tolist() == [0, 1]
    # a frozen variable has no rows in the CSR, hence no tasks
    dg = R.DeviceGraph(_zero_init(_chain_graph(16)), plan_only=True)
    dg.set_frozen(["x2"])
    pt = dg.tasks[R.Pose3]["host"]
    assert 2 not in pt["task_var"].tolist() and dg.tasks[R.Pose3]["T"] == 21
    assert dg.csr[R.Pose3]["ptr_h"].tolist() == [0, 2, 5, 5, 8, 10]
    assert set(pt["task_rows"].tolist()) == set(range(1, 13)) - {3, 6, 10}         # the rows towards x2 feed nobody
    dg.set_frozen([])
    assert dg.tasks[R.Pose3]["T"] == 27


def test_partial_tasks_errors():
    with pytest.raises(ValueError, match="coordinates"):
        R.partial_tasks([0, 1], [0], [(0, 3)], 3)
    with pytest.raises(ValueError, match="coordinates"):
        R.partial_tasks([0, 1], [0], [(-1,)], 3)
    with pytest.raises(ValueError, match="coordinates"):
        R.partial_tasks([0, 1], [0], [()], 3)
    with pytest.raises(ValueError, match="row"):
        R.partial_tasks([0, 1], [1], [(0,)], 3)
    with pytest.raises(ValueError, match="row"):
        R.partial_tasks([0, 1], [-1], [(0,)], 3)


def test_off_is_the_plan_and_csr_of_today():
    """the chain graph's conv_plan and CSR, as recorded before the partial-aware product existed"""
    dg = R.DeviceGraph(_zero_init(_chain_graph(16)), plan_only=True)
    o = R.make_opts(N=16, solver=1, stream_offset=1000)
    plan = dg.conv_plan(o, sweep=3)
    base = 1000 + (3 << 32)
    assert plan == [
        dict(name="p3p3", entry="rome_conv_pose3pose3_dev", n_conv=1, dir_all=0, stream_offset=base + (5 << 28), vt_target="Pose3", prop_lo=0, cols=[], fused=False),
        dict(name="p3xyy", entry="rome_conv_pose3pose3xyyaw_dev", n_conv=8, dir_all=0, stream_offset=base + (13 << 28), vt_target="Pose3", prop_lo=1, cols=[], fused=False),
        dict(name="zrp3", entry="rome_conv_priorpose3zrp_dev", n_conv=4, dir_all=0, stream_offset=base + (14 << 28), vt_target="Pose3", prop_lo=9, cols=[], fused=False)]
    assert dg.csr[R.Pose3]["ptr_h"].tolist() == CHAIN_PTR and dg.csr[R.Pose3]["rows_h"].tolist() == CHAIN_ROWS
    assert dg.csr[R.Pose3]["ptr"].tolist() == CHAIN_PTR and dg.csr[R.Pose3]["rows"].tolist() == CHAIN_ROWS
    assert dg.n_prop[R.Pose3] == 13 and list(dg.families(every=True)) == ["p3p3", "prior3", "p3xyy", "zrp3"]
    import inspect
    for fn in (R.DeviceGraph.product_step, R.DeviceGraph.solve, R.solveGraph):
        assert inspect.signature(fn).parameters["partial_product"].default == "off"
    with pytest.raises(ValueError, match="partial_product"):                     # (raised before anything touches the device)
        dg.product_step(o, partial_product="on")
    assert (R.DeviceGraph.STREAM_PARTIAL2, R.DeviceGraph.STREAM_PARTIAL3) == (15 << 28, (15 << 28) + (1 << 27))
    bases = sorted(v for k, v in vars(R.DeviceGraph).items() if k.startswith("STREAM_"))
    assert bases[-2:] == [15 << 28, (15 << 28) + (1 << 27)] and len(set(bases)) == len(bases) and bases[-1] + (1 << 27) == 1 << 32


def test_product_partial_validates_its_tables_on_the_host():
    """the library trusts coordinates and rows, so R.product_partial refuses bad tables before it touches the device"""
    o = R.make_opts(N=8)
    prop, bel = np.zeros((3, 3, 8)), np.zeros((2, 3, 8))
    good = dict(task_var=[0, 1], task_coord=[0, 2], task_ptr=[0, 2, 3], task_rows=[0, 1, 2], task_joint=[0, 1])
    for key, val, msg in (("task_coord", [0, 3], "outside"), ("task_rows", [0, 1, 3], "outside"), ("task_var", [0, 2], "outside"),
                          ("task_var", [-1, 1], "outside"), ("task_ptr", [0, 2, 2], "task_ptr"), ("task_ptr", [1, 2, 3], "task_ptr"),
                          ("task_ptr", [0, 2, 4], "task_ptr"), ("task_joint", [0], "lengths"), ("task_coord", [0, 2, 1], "lengths")):
        with pytest.raises(ValueError, match=msg):
            R.product_partial(o, 3, dict(good, **{key: val}), prop, bel)
    with pytest.raises(ValueError, match="more than one task"):
        R.product_partial(o, 3, dict(good, task_var=[1, 1], task_coord=[2, 2]), prop, bel)
    with pytest.raises(ValueError, match="must be"):
        R.product_partial(o, 3, good, prop[:, :2], bel)
    with pytest.raises(ValueError):
        R.product_partial(o, 3, good, prop, bel, prop_bw=np.ones((2, 3)))


# ------------------------------------------------------------------ the surface
def test_header_ctypes_and_julia_agree():
    hdr = open(os.path.join(ROOT, "include", "rome_mi355.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rome_[a-z0-9_]+)\s*\(", hdr))
    new = {"rome_product_partial_dev", "rome_product_partial"}
    assert new <= declared and new <= set(R._lib.SIGNATURES) and declared == set(R._lib.SIGNATURES)
    protos = c_prototypes()
    want_dev = ["Ptr", "Ptr", "Int32", "Int32", "Int32"] + ["Ptr{Int32}"] * 5 + ["Ptr{Float64}"] * 3 + ["UInt32", "Ptr{Float64}"]
    assert protos["rome_product_partial_dev"] == want_dev and protos["rome_product_partial"] == want_dev + ["Int32"]
    import ctypes as C
    cls = {C.c_int32: "Int32", C.c_uint32: "UInt32", C.c_void_p: "Ptr", R._lib._PO: "Ptr"}
    for name in new:
        res, args = R._lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(protos[name])
        for a, p in zip(args, protos[name]):
            got = cls.get(a) or ("Ptr{Int32}" if a is R._lib._PI else "Ptr{Float64}" if a is R._lib._PD else None)
            assert got == p or (got == "Ptr" and p.startswith("Ptr")), (name, a, p)
    src = jl_source()
    calls = [m for m in re.finditer(r"ccall\(", src) if _call_args(src, m.end() - 1)[0].replace(" ", "") == "(:rome_product_partial,LIB)"]
    assert len(calls) == 1 and "function product_partial!" in src
    assert "product_partial" in dir(R) and "partial_tasks" in dir(R)
