"""The reference side of the belief-evaluation tests (tests/kde_eval_ref.py) and what needs no device, checked on the CPU: the header
and the binding table, the float64 restatement against mpmath on every case, the stored mp values against a fresh mp run, the constructed
rows against what they are meant to exercise, closed forms, and the wrappers' argument validation.  Run with -s it prints the
reference-side error figures recorded in profiles/kde_eval_reference_errors.md."""
import inspect
import math
import os
import re

import mpmath as mpm
import numpy as np
import pytest

import kde_eval_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entries_and_the_table_carries_them():
    import rome_jl_amd as R
    hdr = open(os.path.join(ROOT, "include", "rome_mi355.h")).read()
    assert re.search(r"#define ROME_MAX_PARTICLES_KDE_EVAL 512\b", hdr)
    doc = re.search(r"/\* rome_kde_eval\*:.*?\*/", hdr, flags=re.S).group(0)
    assert "NOT CHECKED against AMP" in doc
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(rome_[a-z0-9_]+)\s*\(", hdr))
    new = {"rome_kde_eval", "rome_kde_eval_dev"}
    assert new <= declared and new <= set(R._lib.SIGNATURES)
    assert declared == set(R._lib.SIGNATURES)
    for name in new:        # as many ctypes arguments as the prototype has parameters
        proto = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr).group(1)
        assert len(R._lib.SIGNATURES[name][1]) == proto.count(",") + 1, name
    assert R.MAX_PARTICLES_KDE_EVAL == R._lib.MAX_PARTICLES_KDE_EVAL == 512


@pytest.mark.parametrize("dim", K.DIMS)
def test_restatement_and_stored_values_against_mp_on_every_case(dim):
    """mp finite on every mp row, tests/golden/kde_eval_reference.json equal to a fresh mp run to 25 digits, and dev_np per case printed:
    it is what the device's bound is made of (kde_eval_ref's docstring)"""
    worst = {}
    for name, c in K.cases().items():
        if c["dim"] != dim:
            continue
        fresh = K.compute(name)
        for tag, h in c["bws"]:
            ref = K.reference(name, tag)
            assert len(ref["mp"]) == len(c["idx"]) and (len(c["idx"]) <= K.MP_QUERIES or not name.startswith(("eval/", "loo/")))
            with mpm.workdps(K.DPS):
                for a, b in zip(fresh[tag], ref["mp"]):
                    assert mpm.isfinite(b) and abs(mpm.mpf(a) - b) <= mpm.mpf(10) ** -25 * max(1, abs(b)), (name, tag)
            assert np.isfinite(ref["np"]).all(), (name, tag)
            print("%-28s %-5s logp_mp in [%.6g, %.6g]  dev_np = %.2f eps  bound = %.1f ulp"
                  % (name, tag, float(min(ref["mp"])), float(max(ref["mp"])), ref["dev_np"] / K.EPS, ref["tol"] / K.EPS))
            key = (name.split("/")[0], name.split("/")[2] if name.startswith("eval/") else "-", tag)
            worst[key] = max(worst.get(key, 0.0), ref["dev_np"] / K.EPS)
    for key, dev in sorted(worst.items()):
        print("dim %d worst dev_np of %-24s = %.2f eps" % (dim, "/".join(key), dev))
    # 8·dev_np stays under the 64 ulp floor on every case, so the floor is the device's bound everywhere
    assert all(8.0 * dev <= 64.0 for dev in worst.values()), worst


@pytest.mark.parametrize("dim", K.DIMS)
def test_constructed_rows_lie_where_they_are_meant_to(dim):
    N, Q = 100, 256
    bel, pts = K.table(dim, "ordinary", N, Q)
    assert np.array_equal(pts[:, :N], bel) and not np.array_equal(pts[:, N:2 * N], bel)     # the particles themselves, then others
    bel, pts = K.table(dim, "edges", N, Q)
    d = K.np_diffs(dim, bel, pts)
    assert np.all(d[0, 0] == 0.0)                                                           # query 0 equals particle 0
    if dim == 3:        # every heading difference crosses the cut: the raw one is beyond π, the wrapped one small
        raw = pts[2][1:, None] - bel[2][None, :]
        assert (np.abs(raw) > math.pi).all() and (np.abs(d[1:, :, 2]) < 0.07).all()
    if dim == 6:        # every relative rotation within 1e-3 of π and clear of the snap zone (acos(1 − √eps) = 1.7e-4)
        ang = np.linalg.norm(d[1:, 1:, 3:], axis=2)
        assert (math.pi - ang).max() < 1e-3 and (math.pi - ang).min() > 2.5e-4, (math.pi - ang.max(), math.pi - ang.min())
    bel, pts = K.table(dim, "identical", N, Q)
    assert (bel == bel[:, :1]).all() and np.array_equal(pts[:, 0], bel[:, 0])
    bel, pts = K.table(dim, "far", N, Q)
    d = K.np_diffs(dim, bel, pts)
    assert (np.abs(d[:, :, 0]) > 30.0).all()
    for tag, hs in K.BANDWIDTHS:        # a plain exp(−½q) is 0 in float64 at either bandwidth: the log-density must not be −inf
        q = np.sum((d / np.array(hs[dim])) ** 2, axis=2)
        assert q.min() > 2 * 745.2 and math.exp(-0.5 * q.min()) == 0.0
        lp = K.reference("eval/%d/far/%d/%d" % (dim, N, Q), tag)
        assert np.isfinite(lp["np"]).all() and lp["np"].max() < -5000.0
    assert float(K.reference("eval/%d/far/%d/%d" % (dim, N, Q), "aniso")["mp"][0]) < -5e8     # 40 units at h = 1e-3: logp ≈ −8e8


def test_closed_forms_of_both_sides():
    """one particle on Point2: the Gaussian log-pdf; a leave-one-out pair: each point under the other's kernel; a Riemann sum of the
    restatement over a grid is 1"""
    y, h = np.array([[0.7], [-1.1]]), (0.3, 0.5)
    x = np.array([[0.9, -2.0], [-1.0, 3.0]])
    want = [-0.5 * (((x[0, i] - 0.7) / 0.3) ** 2 + ((x[1, i] + 1.1) / 0.5) ** 2) - math.log(0.3 * 0.5) - math.log(2 * math.pi) for i in range(2)]
    got = K.np_logpdf(2, y, h, x)
    mp = K.mp_logpdf(2, K.mp_diffs(2, y, x, [0, 1]), h)
    assert np.allclose(got, want, rtol=1e-14, atol=1e-14) and np.allclose([float(v) for v in mp], want, rtol=1e-14, atol=1e-14)
    pair = np.array([[0.0, 0.4], [0.0, -0.3], [0.1, 0.3]])
    loo = K.np_logpdf(3, pair, (0.3, 0.3, 0.3), None, leave_one_out=True)
    one = K.np_logpdf(3, pair[:, 1:], (0.3, 0.3, 0.3), pair[:, :1])
    assert abs(loo[0] - one[0]) <= 1e-14
    mp = K.mp_logpdf(3, K.mp_diffs(3, pair, pair, [0, 1]), (0.3, 0.3, 0.3), [0, 1], leave_one_out=True)
    assert abs(float(mp[0]) - loo[0]) <= 1e-14 and abs(float(mp[1]) - loo[1]) <= 1e-14
    g = np.linspace(-5.0, 5.0, 128)
    grid = np.stack([a.ravel() for a in np.meshgrid(g, g, indexing="ij")])
    bel = np.array([[0.5, -1.0, 0.2], [0.1, 0.8, -0.6]])
    total = np.sum(np.exp(K.np_logpdf(2, bel, (0.3, 0.3), grid))) * (g[1] - g[0]) ** 2
    assert abs(total - 1.0) <= 1e-10, total


def test_public_surface_and_argument_validation_that_need_no_device():
    import rome_jl_amd as R
    assert str(inspect.signature(R.kde_logpdf)) == "(bel, pts=None, bw=None, leave_one_out=False, ctx=None)"
    assert str(inspect.signature(R.kde_mode)) == "(bel, bw=None, ctx=None)"
    assert str(inspect.signature(R.kld)) == "(a, b, bw_a=None, bw_b=None, leave_one_out=False, ctx=None)"
    assert str(inspect.signature(R.evalBelief)) == "(fg, label, pts, log=True)"
    assert str(inspect.signature(R.beliefLogLikelihood)) == "(fg, truth)"
    assert str(inspect.signature(R.kldBeliefs)) == "(fg_a, fg_b, labels=None)"
    assert str(inspect.signature(R.DeviceGraph.logpdf)) == "(self, vartype, queries=None, bw=None, leave_one_out=False, out=None)"
    for name in ("kde_logpdf", "kde_mode", "kld", "evalBelief", "beliefLogLikelihood", "kldBeliefs"):
        assert getattr(R.api, name) is getattr(R, name) and not name.startswith(("conv_", "sample_", "residual_"))
    assert "unvendored" in R.kld.__doc__ and "⚠" in R.kld.__doc__
    bel, bw = np.zeros((3, 8)), [0.3, 0.3, 0.3]
    bad = [dict(bel=np.zeros((4, 8))),                                   # dim 4
           dict(bel=np.zeros(8)),                                        # not a block
           dict(bel=np.zeros((3, 513))),                                 # beyond MAX_PARTICLES_KDE_EVAL
           dict(pts=np.zeros((2, 5))),                                   # other coordinates
           dict(pts=np.zeros((1, 3, 5))),                                # a stack against one block
           dict(pts=np.zeros((3, 5)), leave_one_out=True),               # leave-one-out with queries
           dict(bel=np.zeros((3, 1)), leave_one_out=True),               # ... or with one particle
           dict(bw=[0.3, 0.0, 0.3]), dict(bw=[0.3, -1.0, 0.3]), dict(bw=[0.3, float("nan"), 0.3]), dict(bw=[0.3, float("inf"), 0.3]),
           dict(bw=[0.3, 0.3])]
    for kw in bad:
        with pytest.raises(ValueError, match="kde_logpdf"):
            R.kde_logpdf(**dict(dict(bel=bel, bw=bw), **kw))
    with pytest.raises(ValueError, match="kde_mode"):
        R.kde_mode(np.zeros((5, 8)), bw=[1.0] * 5)
    with pytest.raises(ValueError, match="kld"):
        R.kld(np.zeros((3, 8)), np.zeros((2, 8)), bw_a=bw, bw_b=[0.3, 0.3])
    fa, fb = R.generateGraph_Hexagonal(N=10), R.generateGraph_Hexagonal(N=10)
    for l in fa.ls():
        fa.initVariable(l, np.zeros((fa.variables[l].dim, 10)))
    with pytest.raises(ValueError, match=r"\bx0\b.*second"):            # uninitialised in the second graph: named
        R.kldBeliefs(fa, fb, labels=["x0"])
    with pytest.raises(ValueError, match=r"\bl1\b.*first"):
        R.kldBeliefs(fb, fa, labels=["l1"])
    with pytest.raises(ValueError, match=r"\bx3\b"):
        R.beliefLogLikelihood(fb, {"x3": [0.0, 0.0, 0.0]})
    with pytest.raises(ValueError, match=r"\bnowhere\b"):
        R.beliefLogLikelihood(fa, {"nowhere": [0.0, 0.0]})
    with pytest.raises(ValueError, match=r"\bx1\b.*3 coordinates"):
        R.beliefLogLikelihood(fa, {"x1": [0.0, 0.0]})
    with pytest.raises(ValueError, match=r"\bl1\b"):
        R.evalBelief(fb, "l1", np.zeros((2, 4)))
