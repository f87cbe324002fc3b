"""Deconvolution, host side: the two references of deconv_ref.py against each other, the C declarations against the ctypes table, the
refusals by name (no device is touched), and the reference's acceptance line (test/testBasicPose2Conv.jl:56) on the restatement."""
import os
import re

import numpy as np
import pytest

import deconv_ref as dr
import rome_jl_amd as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the deviation of the float64 restatement from mp, relative to the row scale, as measured on the CPU over ALL rows of the geometry
# tables (profiles/deconv_reference_errors.md), rounded up: the restatement has to stay inside it
RECORDED = {"p2p2": 3e-16, "br": 3e-16, "pbear": 3e-16, "p2rng": 3e-16, "pprng": 3e-16, "p3p3": 7e-16, "p3xyy": 6e-16, "p3rot": 6e-16}
RECORDED_NEAR_PI = 2e-13   # Pose3 edge rows with a relative rotation of pi - 1e-3 (the matrix Log divides by sin: 1e-16 / 1e-3)


@pytest.mark.parametrize("family", sorted(dr.FAMILIES))
def test_mp_is_finite_and_numpy_sits_inside_its_recorded_figure(family):
    A, B = dr.geometry_table(family)
    ref = dr.Reference(family, A, B)   # every row through mp
    assert np.isfinite(ref.mp).all() and np.isfinite(ref.np).all()
    assert ref.mp.shape == (len(A), dr.FAMILIES[family][1])
    print("%s: figure %.3e (recorded %.1e), kernel bound %.3e" % (family, ref.figure, RECORDED[family], ref.rel_bound))
    assert ref.figure <= RECORDED[family]
    assert ref.rel_bound == 64.0 * dr.EPS   # 8 x the figure stays under the floor on the generic tables


def test_edge_tables_finite_and_inside_their_figures():
    for family, (A, B) in (("p2p2", dr.pose2_edge_table()), ("br", dr.landmark_edge_table()), ("pbear", dr.landmark_edge_table()),
                           ("pprng", dr.landmark_edge_table())):
        ref = dr.Reference(family, A, B)
        assert np.isfinite(ref.mp).all()
        assert ref.figure <= RECORDED[family], (family, ref.figure)
    A, B = dr.pose3_edge_table()
    near = dr.near_pi_rows(A, B)
    rest = np.setdiff1d(np.arange(len(A)), near)
    assert len(near) == 6
    for family in ("p3p3", "p3rot", "p3xyy"):
        assert np.isfinite(dr.Reference(family, A, B).mp).all()
        assert dr.Reference(family, A[rest], B[rest]).figure <= 1.5e-15, family
    for family in ("p3p3", "p3rot"):
        fig = dr.Reference(family, A[near], B[near]).figure
        assert 1e-15 < fig <= RECORDED_NEAR_PI, (family, fig)


def test_mp_known_answers():
    """rows whose answer is known in closed form"""
    z = dr.mp_predict("p2p2", [1.0, 2.0, np.pi / 2], [1.0, 5.0, np.pi])
    assert abs(float(z[0]) - 3.0) < 1e-15 and abs(float(z[1])) < 1e-15 and abs(float(z[2]) - np.pi / 2) < 1e-15
    z = dr.mp_predict("br", [0.0, 0.0, np.pi / 2], [0.0, 2.0])
    assert abs(float(z[0])) < 1e-15 and abs(float(z[1]) - 2.0) < 1e-15
    z = dr.mp_predict("p3p3", [0, 0, 0, 0, 0, 0.5], [1.0, 0, 0, 0, 0, 1.25])
    assert np.allclose([float(x) for x in z], [np.cos(0.5), -np.sin(0.5), 0, 0, 0, 0.75], atol=1e-15)
    z = dr.mp_predict("p3xyy", [0, 0, 7.0, 0, 0, 0.5], [1.0, 0, -3.0, 0, 0, 1.25])
    assert np.allclose([float(x) for x in z], [np.cos(0.5), -np.sin(0.5), 0.75], atol=1e-15)
    assert float(dr.mp_predict("pprng", [3.0, 0.0, 1.0], [0.0, 4.0])[0]) == 5.0


def test_header_declares_the_entries_and_the_table_carries_them():
    hdr = open(os.path.join(ROOT, "include", "rome_mi355.h")).read()
    assert "NOT CHECKED against IIF" in hdr
    assert re.search(r"#define ROME_MI355_VERSION 122\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rome_[a-z0-9_]+)\s*\(", hdr))
    new = {"rome_deconv", "rome_deconv_dev"}
    assert new <= declared and new <= set(R._lib.SIGNATURES)
    assert declared == set(R._lib.SIGNATURES)
    # the family enum of the header and of the binding agree, name by name
    enum = re.search(r"enum \{ (ROME_DECONV_[^}]*)\}", hdr).group(1)
    pairs = dict((n.strip(), int(v)) for n, v in (e.split("=") for e in enum.split(",")))
    assert len(pairs) == 8
    for name, v in pairs.items():
        assert getattr(R._lib, name[len("ROME_"):]) == v
    # the descriptor: the header's fields in the header's order
    body = re.search(r"typedef struct rome_deconv_table \{(.*?)\} rome_deconv_table;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f[0] for f in R._lib.DeconvTable._fields_]


def _graph():
    fg = R.initfg(N=20)
    for l, t in (("x0", R.Pose2), ("x1", R.Pose2), ("x2", R.Pose2), ("l1", R.Point2), ("l2", R.Point2), ("q0", R.Pose3)):
        fg.addVariable(l, t)
        fg.initVariable(l, np.zeros((t.dim, fg.N)))
    lab = {}
    lab["prior2"] = fg.addFactor(["x0"], R.PriorPose2(R.MvNormal(np.zeros(3), 0.01 * np.eye(3))))
    lab["prior3"] = fg.addFactor(["q0"], R.PriorPose3(R.MvNormal(np.zeros(6), 0.01 * np.eye(6))))
    lab["priorpt"] = fg.addFactor(["l1"], R.PriorPoint2(R.MvNormal(np.zeros(2), np.eye(2))))
    lab["zrp"] = fg.addFactor(["q0"], R.PriorPose3ZRP(R.Normal(0.0, 0.1), R.MvNormal(np.zeros(2), 0.01 * np.eye(2))))
    lab["pt2pt2"] = fg.putFactor("l1l2f1", ["l1", "l2"], R.Point2Point2(R.MvNormal(np.zeros(2), np.eye(2))))
    lab["mh"] = fg.addFactor(["x0", "x1", "x2"], R.Pose2Pose2(R.MvNormal([1.0, 0, 0], 0.01 * np.eye(3))), multihypo=[1.0, 0.5, 0.5])
    lab["range"] = fg.addFactor(["x0", "l1"], R.Pose2Point2Range(R.Normal(5.0, 0.1)))
    lab["odo"] = fg.addFactor(["x0", "x1"], R.Pose2Pose2(R.MvNormal([1.0, 0, 0], 0.01 * np.eye(3))))
    return fg, lab


def test_refusals_without_a_device():
    fg, lab = _graph()
    for k, cls in (("prior2", "PriorPose2"), ("prior3", "PriorPose3"), ("priorpt", "PriorPoint2"), ("zrp", "PriorPose3ZRP"), ("pt2pt2", "Point2Point2")):
        with pytest.raises(TypeError, match=cls):
            R.approxDeconv(fg, lab[k])
        with pytest.raises(TypeError, match=cls):
            R.factorMMD(fg, [lab[k]])
        with pytest.raises(TypeError, match=cls):
            R.deconv_family(cls)
    with pytest.raises(TypeError, match="multihypo"):
        R.approxDeconv(fg, lab["mh"])
    with pytest.raises(TypeError, match="multihypo"):
        R.factorMMD(fg, [lab["odo"], lab["mh"]])
    with pytest.raises(TypeError, match="Pose2Point2Range"):
        R.factorMMD(fg, [lab["range"]])
    # what labels=None selects: the mmd families without multihypo
    assert [fl for fl, _, f in fg.factors if isinstance(f, R.convolution._MMD_FAMILIES) and fg.multihypo.get(fl) is None] == [lab["odo"]]
    with pytest.raises(ValueError, match="want"):
        R.deconv(R.Pose2Pose2, None, np.zeros((1, 3)), np.eye(3)[None], None, None, want=())
    # every family of the C enum has a Python row with the same dimensions as the reference module's
    for fam, (cls, dz, da, db, _) in dr.FAMILIES.items():
        e = R.deconv_family(cls)
        assert e[1:4] == (dz, da, db) and e[0] == getattr(R._lib, "DECONV_" + cls.upper()
                                                          .replace("BEARINGRANGE", "BR")), fam


def test_the_reference_line_on_the_restatement():
    """test/testBasicPose2Conv.jl:56 `mmd(M, pts, meas) < 0.001`: two independent sample sets of N = 100 draws of MvNormal([10, 0, pi], 0.1 I),
    headings wrapped, for seeds 0..19; and at N in {50, 100, 200}.  (Measured over 600 draws: the largest value was 1.2e-4.)  The threshold
    is the reference's; no case is masked."""
    worst = 0.0
    for N in (100, 50, 200):
        for seed in range(20):
            rng = np.random.default_rng(seed)

            def draw():
                x = np.array([10.0, 0.0, np.pi])[:, None] + np.sqrt(0.1) * rng.standard_normal((3, N))
                x[2] = np.arctan2(np.sin(x[2]), np.cos(x[2]))
                return x
            v = dr.np_mmd_pose2(draw(), draw())
            worst = max(worst, v)
            assert 0.0 <= v < 0.001, (N, seed, v)
    print("largest mmd over 60 draws: %.3e" % worst)
