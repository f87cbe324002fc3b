"""The reference side of the mmd tests (tests/mmd_ref.py), checked on the CPU: the float64 restatement against mpmath on every row and
case, the stored mp sums against a fresh mp run, the constructed rows against what they are meant to exercise, and the golden values on
the reference's own sample files.  Run with -s it prints the reference-side error figures recorded in profiles/mmd_reference_errors.md.
The mp runs are what takes the time here (Pose3: 20 000 quaternion pairs per row): the GPU tests read the stored sums instead."""
import math

import mpmath as mpm
import numpy as np
import pytest

import mmd_ref as M

KINDS = [(kind, dim) for kind in ("features", "golden") for dim in M.DIMS]


@pytest.mark.parametrize("kind,dim", KINDS)
def test_restatement_and_stored_sums_against_mp_on_every_row(kind, dim):
    """np_sums within the floor's share of mp_sums on every panel of every row and case (8·dev <= 64 ulp, so every GPU bound is the floor), and tests/golden/mmd_reference.json equal to a fresh mp run to 25 digits."""
    A, B = M.tables(kind, dim)
    fresh, stored = M.compute(kind, dim), M.reference(kind, dim)
    assert len(fresh["rows"]) == len(stored) == A.shape[0]
    for r, (frow, srow) in enumerate(zip(fresh["rows"], stored)):
        for name, sigma, scale in M.cases(kind):
            f, s = frow[name], srow[name]
            with mpm.workdps(M.DPS):
                for a, b in zip(f["S"] + [f["mmd"]], list(s["S"]) + [s["mmd"]]):
                    assert abs(mpm.mpf(a) - b) <= mpm.mpf(10) ** -25 * max(abs(b), mpm.mpf(10) ** -10), (kind, dim, r, name)
            got = M.np_sums(dim, A[r], B[r], sigma, s["scale"])
            dev, ok = M.np_within_floor(s, got)
            print("%-8s dim %d row %d %-14s S = %.6g %.6g %.6g  mmd = %.12g  dev_np = %.2f %.2f %.2f eps  "
                  "|mmd_np - mmd| = %.2e  bound(mmd) = %.2e" % ((kind, dim, r, name) + tuple(float(x) for x in s["S"]) + (float(s["mmd"]),) +
                                                                tuple(dev) + (abs(got[3] - float(s["mmd"])), s["bound"][1])))
            assert all(ok), (kind, dim, r, name, dev)
            assert abs(got[3] - float(s["mmd"])) <= s["bound"][1] / 4.0


@pytest.mark.parametrize("dim", M.DIMS)
def test_constructed_rows_lie_where_they_are_meant_to(dim):
    A, B = M.features(dim)
    X, Y = A[1].T, B[1].T
    d = np.stack([M.np_diff(dim, x, Y) for x in X])                         # (Na, Nb, dim): edges row, ab panel
    coincident = np.all(d == 0.0, axis=2)
    assert coincident.sum() >= 10 and np.array_equal(A[1][:, 50:55], A[1][:, 0:5])
    if dim == 3:       # every ab heading difference crosses the cut: the raw difference is beyond π, the wrapped one small
        raw = X[:, None, 2] - Y[None, :, 2]
        assert (np.abs(raw[:, 10:]) > math.pi).all() and (np.abs(d[:, 10:, 2]) < 0.07).all()
    if dim == 6:       # every ab relative rotation within 1e-3 of π and clear of the snap zone (acos(1 − √eps) = 1.7e-4)
        ang = np.linalg.norm(d[:, 10:, 3:], axis=2)
        assert (math.pi - ang).max() < 1e-3 and (math.pi - ang).min() > 2.5e-4, (math.pi - ang.max(), math.pi - ang.min())
    Xf, Yf = A[2].T, B[2].T
    q = np.stack([np.sum(M.np_diff(dim, x, Yf) ** 2, axis=1) for x in Xf])
    assert q.min() > 800.0                                                  # σ = 1: every ab term is below exp(−750) -> 0 on the device
    for name, sigma, scale in M.CASES:
        ref = M.reference("features", dim)[2][name]
        dropped = scale is not None and M.ZERO_SCALE[dim][0] == 0.0         # (dim 2: the zero entry drops the very coordinate they differ in)
        assert (float(ref["S"][1]) < 1e-300) == (sigma == 1.0 and not dropped)


def test_golden_values_on_the_reference_sample_files():
    """mmd(X1ptst, X2ptst) (100 against 200 points) and the even / odd halves of each file at σ = 1e-3, unit scale: the mp values, which
    round to the float64 figures the feature was specified with (1.0735; 1.46e-3 and 1.18e-3), and the two candidate rotation weights."""
    ab = M.reference("golden", 6)[0]["s1e-3"]
    h1, h2 = M.golden_halves()
    with mpm.workdps(M.DPS):
        for got, want in ((ab["mmd"], "1.07351165216416186"), (h1["mmd"], "0.00146095114060761055"), (h2["mmd"], "0.00117540231620796679")):
            assert abs(got - mpm.mpf(want)) <= mpm.mpf(10) ** -17, (mpm.nstr(got, 25), want)
    assert "%.4f" % float(ab["mmd"]) == "1.0735" and "%.2e" % float(h1["mmd"]) == "1.46e-03" and "%.2e" % float(h2["mmd"]) == "1.18e-03"
    X1, X2 = M.golden_files()
    assert abs(M.np_sums(6, X1, X2)[3] - float(ab["mmd"])) <= ab["bound"][1]
    frob = M.np_sums(6, X1, X2, 1e-3, [1.0, 1.0, 1.0, math.sqrt(2.0), math.sqrt(2.0), math.sqrt(2.0)])[3]
    assert "%.5f" % float(ab["mmd"]) == "1.07351" and "%.5f" % frob == "1.07340"       # geodesic angle | Frobenius norm: 1e-4 relative
    print("golden: mmd(X1ptst, X2ptst) = %s, X1 halves %s, X2 halves %s, rotation weight sqrt(2): %.10g"
          % (mpm.nstr(ab["mmd"], 18), mpm.nstr(h1["mmd"], 18), mpm.nstr(h2["mmd"], 18), frob))


def test_public_surface_and_refusals_that_need_no_device():
    import inspect
    import rome_jl_amd as R
    assert R.MAX_PARTICLES_MMD == R._lib.MAX_PARTICLES_MMD == 512
    assert str(inspect.signature(R.mmd)) == "(a, b, bw=0.001, scale=None, return_sums=False, ctx=None)"
    assert str(inspect.signature(R.DeviceGraph.mmd)) == "(self, vartype, other, bw=0.001, scale=None, out=None)"
    assert list(inspect.signature(R.mmdBeliefs).parameters)[:5] == ["fg_a", "fg_b", "labels", "bw", "scale"]
    fa, fb = R.generateGraph_Hexagonal(N=10), R.generateGraph_Hexagonal(N=10)
    for l in fa.ls():
        fa.initVariable(l, np.zeros((fa.variables[l].dim, 10)))
    with pytest.raises(ValueError, match=r"\bx0\b.*second"):            # uninitialised in the second graph: named
        R.mmdBeliefs(fa, fb, labels=["x0"])
    with pytest.raises(ValueError, match=r"\bl1\b.*first"):
        R.mmdBeliefs(fb, fa, labels=["l1"])
    with pytest.raises(ValueError):
        R.mmd(np.zeros((3, 4)), np.zeros((2, 3, 4)))
