"""mmd between particle sets on the device (k_mmd<M> of rome.jl_amd/csrc/rome_product.hip behind rome_mmd / rome_mmd_dev, api.mmd, R.mmdBeliefs,
DeviceGraph.mmd), against the references of tests/mmd_ref.py.

  * exact pair counting: σ = 0 makes every kernel value 1, so the three sums are the pair counts and mmd is 0.0 -- exactly, at the block
    shapes where a mis-mapped pair index would show (one point, fewer pairs than threads, one past a wave, 512 + 512)
  * against mpmath at Na = Nb = 100 (σ = 1e-3 and 1, and a scale with a zero entry) and on the reference's sample files (100 against
    200 points): sums relative, mmd absolute, bounds from the reference side (mmd_ref's docstring; figures in
    profiles/mmd_reference_errors.md)
  * properties, indexing, the three host layouts, the graph-level wrappers, the reference's own acceptance line and the refusals
"""
import ctypes as C
import math

import numpy as np
import pytest

import mmd_ref as M

pytestmark = pytest.mark.gpu

PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
COUNT_SHAPES = [(1, 1), (1, 2), (2, 1), (63, 65), (64, 64), (100, 200), (257, 3), (512, 512)]
PROPERTY_SHAPES = [(100, 200), (257, 3)]
PROPERTY_BOUND = 4.0 * M.ULP64     # the absolute bound of mmd (mmd_ref: bounds)


@pytest.fixture(scope="module", autouse=True)
def _pkg():
    global R, _lib, torch
    import torch as T
    import rome_jl_amd
    from rome_jl_amd import _lib as L
    R, _lib, torch = rome_jl_amd, L, T
    R.default_context()
    yield


def _cloud(rng, P, dim, N, shift=0.0):
    x = np.clip(rng.standard_normal((P, dim, N)), -3.0, 3.0)
    x[:, 0] += shift
    if dim == 3:
        x[:, 2] = rng.uniform(-math.pi, math.pi, (P, N))
    if dim == 6:
        x[:, 3:] *= 0.5
    return x


def _p(a, t=PD):
    return None if a is None else a.ctypes.data_as(t)


def _host(layout, dim, P, Na, a, a_rows, Nb, b, b_rows, scale=None, sigma=1e-3, sums=True, n_a=None, n_b=None):
    """rome_mmd as it is -> (code, out, sums)"""
    ctx = R.default_context()
    out, sm = np.full(max(P, 1), np.nan), (np.full((max(P, 1), 3), np.nan) if sums else None)
    ar = None if a_rows is None else np.ascontiguousarray(a_rows, dtype=np.int32)
    br = None if b_rows is None else np.ascontiguousarray(b_rows, dtype=np.int32)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    rc = _lib.load().rome_mmd(ctx.handle, layout, dim, P, Na, a.shape[0] if n_a is None else n_a, _p(a), _p(ar, PI), Nb,
                              b.shape[0] if n_b is None else n_b, _p(b), _p(br, PI), _p(sc), float(sigma), _p(out), _p(sm))
    return rc, out, sm


def _dev(dim, P, Na, a, a_rows, Nb, b, b_rows, scale=None, sigma=1e-3, sums=True):
    """rome_mmd_dev on device copies of SoA host arrays -> (code, out, sums)"""
    ctx = R.default_context()
    dev = torch.device("cuda", 0)
    t = lambda x, dt: None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    ta, tb, tar, tbr = t(a, torch.float64), t(b, torch.float64), t(a_rows, torch.int32), t(b_rows, torch.int32)
    out = torch.full((max(P, 1),), float("nan"), dtype=torch.float64, device=dev)
    sm = torch.full((max(P, 1), 3), float("nan"), dtype=torch.float64, device=dev) if sums else None
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    ptr = lambda x: None if x is None else x.data_ptr()
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    rc = _lib.load().rome_mmd_dev(ctx.handle, dim, P, Na, ptr(ta), ptr(tar), Nb, ptr(tb), ptr(tbr), _p(sc), float(sigma), ptr(out), ptr(sm))
    torch.cuda.synchronize(dev)
    return rc, out.cpu().numpy(), None if sm is None else sm.cpu().numpy()


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------------ pair counting
@pytest.mark.parametrize("Na,Nb", COUNT_SHAPES)
@pytest.mark.parametrize("dim", M.DIMS)
def test_sigma_zero_counts_every_ordered_pair_exactly(dim, Na, Nb):
    rng = np.random.default_rng(1000 * dim + 7 * Na + Nb)
    a, b = _cloud(rng, 2, dim, Na), _cloud(rng, 2, dim, Nb, shift=1.0)
    out, sums = R.mmd(a, b, bw=0.0, return_sums=True)
    assert np.array_equal(sums, np.tile([float(Na * Na), float(Na * Nb), float(Nb * Nb)], (2, 1))), sums
    assert np.array_equal(_bits(out), _bits(np.zeros(2))), out


# ------------------------------------------------------------------------------------------------------------ against mpmath
@pytest.mark.parametrize("dim", M.DIMS)
@pytest.mark.parametrize("kind", ["features", "golden"])
def test_sums_and_value_against_mp(kind, dim):
    """every row of the table in one launch per case; sums within 64 ulp·S + T·2^-1022, mmd within 4 x 64 ulp (mmd_ref: bounds)"""
    A, B = M.tables(kind, dim)
    ref = M.reference(kind, dim)
    worst = []
    for name, sigma, scale in M.cases(kind):
        out, sums = R.mmd(A, B, bw=sigma, scale=M.case_scale(dim, scale), return_sums=True)
        for r, row in enumerate(ref):
            c = row[name]
            with M.mpm.workdps(M.DPS):
                ds = [abs(float(M.mpm.mpf(float(sums[r, k])) - c["S"][k])) for k in range(3)]
                dm = abs(float(M.mpm.mpf(float(out[r])) - c["mmd"]))
            print("%-8s dim %d row %d %-14s |ΔS| / bound = %s   |Δmmd| = %.2e / %.2e   (ΔS in ulp of S: %s)"
                  % (kind, dim, r, name, " ".join("%.3f" % (d / bd) for d, bd in zip(ds, c["bound"][0])), dm, c["bound"][1],
                     " ".join("%.1f" % (d / (M.EPS * max(float(s), M.TINY))) if float(s) > 1e-290 else "-" for d, s in zip(ds, c["S"]))))
            worst.append((max(d / bd for d, bd in zip(ds, c["bound"][0])), dm / c["bound"][1], r, name))
    for ws, wm, r, name in worst:
        assert ws <= 1.0 and wm <= 1.0, (kind, dim, r, name, ws, wm)
    if kind == "features":      # the far row at σ = 1: S_ab underflowed to exactly 0 (unless the scale drops the coordinate they differ in)
        out, sums = R.mmd(A, B, bw=1.0, return_sums=True)
        assert sums[2, 1] == 0.0 and out[2] == sums[2, 0] / 1e4 + sums[2, 2] / 1e4


# ------------------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("Na,Nb", PROPERTY_SHAPES)
@pytest.mark.parametrize("dim", M.DIMS)
def test_properties(dim, Na, Nb):
    rng = np.random.default_rng(31 * dim + Na)
    a, b = _cloud(rng, 3, dim, Na), _cloud(rng, 3, dim, Nb, shift=0.7)
    ab = R.mmd(a, b)
    ba = R.mmd(b, a)
    aa = R.mmd(a, a)
    pa, pb = rng.permutation(Na), rng.permutation(Nb)
    perm = R.mmd(a[:, :, pa], b[:, :, pb])
    print("dim %d (%d, %d): mmd %s  |ab - ba| %.2e  |aa| %.2e  |perm - ab| %.2e  bound %.2e"
          % (dim, Na, Nb, ab, np.abs(ab - ba).max(), np.abs(aa).max(), np.abs(perm - ab).max(), PROPERTY_BOUND))
    assert (ab > 0.0).all()
    assert np.abs(ab - ba).max() <= PROPERTY_BOUND
    assert np.abs(aa).max() <= PROPERTY_BOUND
    assert np.abs(perm - ab).max() <= PROPERTY_BOUND
    # exactly: the same bits in a second run, and pair 0 alone against pair 0 among three
    again, sums_again = R.mmd(a, b, return_sums=True)
    first, sums_first = R.mmd(a[:1], b[:1], return_sums=True)
    assert np.array_equal(_bits(again), _bits(ab))
    assert np.array_equal(_bits(first), _bits(ab[:1])) and np.array_equal(_bits(sums_first), _bits(sums_again[:1]))


# ------------------------------------------------------------------------------------------------------------ indexing
@pytest.mark.parametrize("dim", M.DIMS)
def test_row_tables_repeat_and_reverse_rows(dim):
    rng = np.random.default_rng(5 + dim)
    Na, Nb = 65, 130
    a, b = _cloud(rng, 3, dim, Na), _cloud(rng, 4, dim, Nb, shift=0.4)
    a_rows, b_rows = [2, 2, 0, 1, 0, 2], [3, 0, 0, 1, 3, 3]
    want = np.array([R.mmd(a[i], b[j], return_sums=True)[0] for i, j in zip(a_rows, b_rows)])
    for call in (_host, _dev):
        args = (dim, 6, Na, a, a_rows, Nb, b, b_rows)
        rc, out, sums = call(_lib.LAYOUT_SOA, *args) if call is _host else call(*args)
        assert rc == 0 and np.array_equal(_bits(out), _bits(want)), (call.__name__, out, want)
        assert np.array_equal(_bits(out[0]), _bits(out[5])) and np.array_equal(_bits(sums[0]), _bits(sums[5]))
    # one array on both sides, one table reversed: mmd of a set with itself is 0 to the bound, and (i, j) mirrors (j, i) to the bound
    rc, out, _ = _dev(dim, 3, Na, a, [0, 1, 2], Na, a, [2, 1, 0])
    assert rc == 0 and abs(out[1]) <= PROPERTY_BOUND and abs(out[0] - out[2]) <= PROPERTY_BOUND and out[0] > 0.0
    # no tables: pair p is (block p, block p)
    rc, out, _ = _dev(dim, 3, Na, a, None, Nb, b, None)
    assert rc == 0 and np.array_equal(_bits(out), _bits(R.mmd(a, b[:3])))


@pytest.mark.parametrize("dim", M.DIMS)
def test_host_and_device_entries_agree_in_every_layout(dim):
    """the coordinates are the device conversion's own image of native points (as tests/test_gpu_capi_layouts.py), so the three layouts
    carry the same values and every entry must return the same bits"""
    rng = np.random.default_rng(77 + dim)
    P, Na, Nb = 2, 70, 33
    sets = []
    for N in (Na, Nb):
        x = rng.standard_normal((P * N, dim)) * (1.0 if dim != 6 else np.array([2.0, 2.0, 2.0, 0.6, 0.6, 0.6]))
        pts = R.coords_to_points(dim, x)
        sets.append((pts.reshape(P, N, -1), R.points_to_coords(dim, pts).reshape(P, N, dim)))
    (pa, ca), (pb, cb) = sets
    soa = lambda c: np.ascontiguousarray(c.transpose(0, 2, 1))
    scale = [0.5, 2.0, 1.0, 1.0, 0.0, 3.0][:dim]
    rc, want, want_s = _dev(dim, P, Na, soa(ca), None, Nb, soa(cb), None, scale, 0.02)
    assert rc == 0 and (want > 0.0).all()
    for layout, a, b in ((_lib.LAYOUT_SOA, soa(ca), soa(cb)), (_lib.LAYOUT_AOS, np.ascontiguousarray(ca), np.ascontiguousarray(cb)),
                         (_lib.LAYOUT_AOS_POINTS, np.ascontiguousarray(pa), np.ascontiguousarray(pb))):
        rc, out, sums = _host(layout, dim, P, Na, a, None, Nb, b, None, scale, 0.02)
        assert rc == 0 and np.array_equal(_bits(out), _bits(want)) and np.array_equal(_bits(sums), _bits(want_s)), layout


def test_device_graph_and_graph_wrappers_agree_with_api_mmd():
    N = 100
    fgs = []
    for seed in (3, 4):
        fg = R.generateGraph_Hexagonal(N=N)
        R.dead_reckon_init(fg, seed=seed)
        fg.initVariable("l1", np.array([[20.0], [0.0]]) + np.random.default_rng(seed).standard_normal((2, N)))
        fgs.append(fg)
    fa, fb = fgs
    want = {l: R.mmd(fa.getVal(l), fb.getVal(l), bw=0.01) for l in fa.ls()}
    assert all(v > 0.0 for v in want.values())
    got = R.mmdBeliefs(fa, fb, bw=0.01)
    assert list(got) == fa.ls() and all(_bits(got[l]) == _bits(want[l]) for l in want), (got, want)
    sub = R.mmdBeliefs(fa, fb, labels=["l1", "x2"], bw=0.01)
    assert list(sub) == ["l1", "x2"] and sub["x2"] == want["x2"]
    dg = R.DeviceGraph(fa)
    dg.upload_beliefs(fa)
    for vt in (R.Pose2, R.Point2):
        labels = dg.packed.labels[vt]
        other = dg.bel[vt].clone()
        other[:len(labels)].copy_(torch.as_tensor(np.stack([fb.getVal(l) for l in labels])))
        res = dg.mmd(vt, other, bw=0.01)
        assert res.shape == (dg.bel[vt].shape[0],) and res.is_cuda
        h = res.cpu().numpy()
        assert all(_bits(h[k]) == _bits(want[l]) for k, l in enumerate(labels))
        # capturable: one launch, no allocation when `out` is given
        out = torch.zeros_like(res)
        g = dg.capture(lambda: dg.mmd(vt, other, bw=0.01, out=out))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(h))
        with pytest.raises(ValueError):
            dg.mmd(vt, other[:, :, :N - 1])


# ------------------------------------------------------------------------------------------------------------ the reference's acceptance line
def test_pose3pose3_nullhypo_proposals_pass_the_reference_mmd_line():
    """test/testPose3Pose3NH.jl:141-145 as the reference writes it: mmd(M, X1ptst, X1pts, bw=[0.001]) < 0.6, for both directions, on the
    graph of tests/test_gpu_multihypo.py::test_pose3pose3_nullhypo_against_reference_validation_samples (rebuilt here).
    Measured: profiles/mmd_reference_errors.md."""
    X1ref, X2ref = M.golden_files()
    N = 100
    cov = np.diag(np.square([1, 1, 1, 0.01, 0.01, 0.01]))
    fg = R.initfg(N)
    fg.addVariable("x1", R.Pose3)
    f1 = fg.addFactor(["x1"], R.PriorPose3(R.MvNormal(np.zeros(6), cov)))
    fg.initVariable("x1", R.approxConv(fg, f1, "x1", seed=1))
    fg.addVariable("x2", R.Pose3); f12 = fg.addFactor(["x1", "x2"], R.Pose3Pose3(R.MvNormal([25.0, 0, 0, 0, 0, 0], cov)))
    fg.initVariable("x2", R.approxConv(fg, f12, "x2", seed=2))
    fg.addVariable("x3", R.Pose3); f23 = fg.addFactor(["x2", "x3"], R.Pose3Pose3(R.MvNormal([25.0, 0, 0, 0, 0, 0], cov)))
    fg.initVariable("x3", R.approxConv(fg, f23, "x3", seed=3))
    f31 = fg.addFactor(["x3", "x1"], R.Pose3Pose3(R.MvNormal([-35.0, 0, 0, 0, 0, 0], cov)))
    X1 = R.approxConv(fg, f31, "x1", seed=4, nullhypo=0.5)
    X3 = R.approxConv(fg, f31, "x3", seed=5, nullhypo=0.5)
    m1, m3 = R.mmd(X1ref, X1, bw=0.001), R.mmd(X2ref, X3, bw=0.001)
    print("mmd(X1ptst, device x1 proposals) = %.6g   mmd(X2ptst, device x3 proposals) = %.6g   (reference: < 0.6)" % (m1, m3))
    assert 0.0 <= m1 < 0.6 and 0.0 <= m3 < 0.6, (m1, m3)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    rng = np.random.default_rng(9)
    a, b = _cloud(rng, 2, 3, 8), _cloud(rng, 2, 3, 9)
    ok = lambda **kw: dict(dict(layout=_lib.LAYOUT_SOA, dim=3, P=2, Na=8, a=a, a_rows=None, Nb=9, b=b, b_rows=None), **kw)
    both = lambda **kw: [_host(**ok(**kw))[0], _dev(**{k: v for k, v in ok(**kw).items() if k not in ("layout", "n_a", "n_b")})[0]]
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED_N
    assert both() == [0, 0]
    assert both(dim=4) == [INV, INV] and both(dim=1) == [INV, INV]
    for sigma in (-1e-3, float("nan"), float("inf")):
        assert both(sigma=sigma) == [INV, INV]
    for bad in (-1.0, float("nan"), float("inf")):
        assert both(scale=[1.0, bad, 1.0]) == [INV, INV]
    assert both(scale=[1.0, 0.0, 1.0]) == [0, 0]
    assert both(P=-1) == [INV, INV] and both(Na=0) == [INV, INV] and both(Nb=0) == [INV, INV]
    # P = 0: a no-op that writes nothing
    for rc, out, _ in (_host(**ok(P=0)), _dev(**{k: v for k, v in ok(P=0).items() if k != "layout"})):
        assert rc == 0 and np.isnan(out).all()
    # N = 513: refused before any launch, by both entries, on either side
    big = _cloud(rng, 1, 3, 513)
    assert both(P=1, Na=513, a=big) == [UNS, UNS] and both(P=1, Nb=513, b=big) == [UNS, UNS]
    assert _host(**ok(P=1, Na=512, a=_cloud(rng, 1, 3, 512)))[0] == 0
    # host entry only: layout, and row tables (or P without them) that leave the arrays
    assert _host(**ok(layout=3))[0] == INV
    assert _host(**ok(a_rows=[0, 2]))[0] == INV and _host(**ok(b_rows=[-1, 0]))[0] == INV and _host(**ok(P=3))[0] == INV
    # needed pointers
    lib, ctx = _lib.load(), R.default_context()
    out = np.zeros(2)
    assert lib.rome_mmd(ctx.handle, 0, 3, 2, 8, 2, None, None, 9, 2, _p(b), None, None, 1e-3, _p(out), None) == INV
    assert lib.rome_mmd(ctx.handle, 0, 3, 2, 8, 2, _p(a), None, 9, 2, None, None, None, 1e-3, _p(out), None) == INV
    assert lib.rome_mmd(ctx.handle, 0, 3, 2, 8, 2, _p(a), None, 9, 2, _p(b), None, None, 1e-3, None, None) == INV
    assert lib.rome_mmd_dev(ctx.handle, 3, 2, 8, None, None, 9, None, None, None, 1e-3, None, None) == INV
    assert lib.rome_mmd(None, 0, 3, 2, 8, 2, _p(a), None, 9, 2, _p(b), None, None, 1e-3, _p(out), None) == INV
    with pytest.raises(R.RomeError) as e:
        R.mmd(big[0], big[0])
    assert e.value.code == UNS
