"""Belief evaluation on the device (k_kde_eval<M> of rome.jl_amd/csrc/rome_product.hip behind rome_kde_eval / rome_kde_eval_dev, api.kde_logpdf,
kde_mode, kld, beliefLogLikelihood, DeviceGraph.logpdf), against the references of tests/kde_eval_ref.py.

  * against mpmath on the mp rows and the float64 restatement on the others, at the block shapes where a mis-mapped query or particle
    index would show (one particle, one query, one past a wave, one past a tile, N = 512), on ordinary, edge, identical and far rows at
    two bandwidth sets; bounds from the reference side (kde_eval_ref's docstring; figures in profiles/kde_eval_reference_errors.md)
  * leave-one-out, placement independence (same bits wherever a query stands), normalisation on a grid, the three host layouts, the
    wrappers and the refusals
"""
import ctypes as C
import math

import numpy as np
import pytest

import kde_eval_ref as K

pytestmark = pytest.mark.gpu

PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)


@pytest.fixture(scope="module", autouse=True)
def _pkg():
    global R, _lib, torch
    import torch as T
    import rome_jl_amd
    from rome_jl_amd import _lib as L
    R, _lib, torch = rome_jl_amd, L, T
    R.default_context()
    yield


def _p(a, t=PD):
    return None if a is None else a.ctypes.data_as(t)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _host(layout, dim, P, N, bel, bel_rows, bw, Q, queries, query_rows, loo=0, n_bel=None, n_q=None):
    """rome_kde_eval as it is -> (code, out (P, Q))"""
    ctx = R.default_context()
    out = np.full((max(P, 1), max(Q, 1)), np.nan)
    br = None if bel_rows is None else np.ascontiguousarray(bel_rows, dtype=np.int32)
    qr = None if query_rows is None else np.ascontiguousarray(query_rows, dtype=np.int32)
    h = None if bw is None else np.ascontiguousarray(bw, dtype=np.float64)
    rc = _lib.load().rome_kde_eval(ctx.handle, layout, dim, P, N, bel.shape[0] if n_bel is None else n_bel, _p(bel), _p(br, PI), _p(h), Q,
                                   (0 if queries is None else queries.shape[0]) if n_q is None else n_q, _p(queries), _p(qr, PI), loo, _p(out))
    return rc, out


def _dev(dim, P, N, bel, bel_rows, bw, Q, queries, query_rows, loo=0):
    """rome_kde_eval_dev on device copies of SoA host arrays -> (code, out (P, Q))"""
    ctx = R.default_context()
    dev = torch.device("cuda", 0)
    t = lambda x, dt: None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dt, device=dev)
    tb, tq, th = t(bel, torch.float64), t(queries, torch.float64), t(bw, torch.float64)
    tbr, tqr = t(bel_rows, torch.int32), t(query_rows, torch.int32)
    out = torch.full((max(P, 1), max(Q, 1)), float("nan"), dtype=torch.float64, device=dev)
    ptr = lambda x: None if x is None else x.data_ptr()
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    rc = _lib.load().rome_kde_eval_dev(ctx.handle, dim, P, N, ptr(tb), ptr(tbr), ptr(th), Q, ptr(tq), ptr(tqr), loo, ptr(out))
    torch.cuda.synchronize(dev)
    return rc, out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ against mpmath
@pytest.mark.parametrize("N,Q", K.SHAPES)
@pytest.mark.parametrize("dim", K.DIMS)
def test_logpdf_against_mp(dim, N, Q):
    """the four rows of a shape in one call per bandwidth set; every output finite, the mp rows within max(8·dev_np, 64 ulp)·max(1, |logp|)
    of mp, the others within that plus dev_np of the restatement"""
    names = ["eval/%d/%s/%d/%d" % (dim, row, N, Q) for row in K.ROWS]
    cs = [K.cases()[n] for n in names]
    bel, pts = np.stack([c["bel"] for c in cs]), np.stack([c["pts"] for c in cs])
    bad = []
    for tag, hs in K.BANDWIDTHS:
        got = R.kde_logpdf(bel, pts, bw=hs[dim])
        assert got.shape == (len(K.ROWS), Q)
        for r, name in enumerate(names):
            ref = K.reference(name, tag)
            wm, wn, finite = K.deviation(ref, got[r])
            print("%-26s %-5s logp in [%.6g, %.6g]  |Δ|/bound: mp rows %.3f, np rows %.3f  (bound %.0f ulp)"
                  % (name, tag, got[r].min(), got[r].max(), wm, wn, ref["tol"] / K.EPS))
            if not (finite and wm <= 1.0 and wn <= 1.0):
                bad.append((name, tag, wm, wn, finite))
    assert not bad, bad


@pytest.mark.parametrize("N", K.LOO_N)
@pytest.mark.parametrize("dim", K.DIMS)
def test_leave_one_out_self_evaluation_against_mp(dim, N):
    name = "loo/%d/%d" % (dim, N)
    bel = K.cases()[name]["bel"]
    for tag, hs in K.BANDWIDTHS:
        got = R.kde_logpdf(bel, bw=hs[dim], leave_one_out=True)
        wm, wn, finite = K.deviation(K.reference(name, tag), got)
        print("%-12s %-5s |Δ|/bound: mp rows %.3f, np rows %.3f" % (name, tag, wm, wn))
        assert finite and wm <= 1.0 and wn <= 1.0, (name, tag, wm, wn)
        # without leave-one-out, self-evaluation is evaluation at pts = bel: the same bits, and a larger density than with it left out
        own, at = R.kde_logpdf(bel, bw=hs[dim]), R.kde_logpdf(bel, bel, bw=hs[dim])
        assert np.array_equal(_bits(own), _bits(at))
        assert (own + math.log(N) > got + math.log(N - 1)).all()


# ------------------------------------------------------------------------------------------------------------ placement
@pytest.mark.parametrize("dim", K.DIMS)
def test_bits_do_not_depend_on_where_a_query_stands(dim):
    rng = np.random.default_rng(40 + dim)
    N, Q, places = 100, 600, [0, 255, 256, 257, 599]
    bel = np.stack([K._cloud(rng, dim, N) for _ in range(3)])
    pts = np.stack([K._cloud(rng, dim, Q) for _ in range(2)])
    x = K._cloud(rng, dim, 1)
    pts[0][:, places] = x
    bw = np.abs(rng.standard_normal((3, dim))) * 0.3 + 0.05
    alone = R.kde_logpdf(bel[0], x, bw=bw[0])
    block = R.kde_logpdf(bel[0], pts[0], bw=bw[0])
    assert alone.shape == (1,) and all(_bits(block[k]) == _bits(alone[0]) for k in places), (alone, block[places])
    assert np.array_equal(_bits(R.kde_logpdf(bel[0], pts[0], bw=bw[0])), _bits(block))             # a second run
    # P = 1 against P = 3 with repeated and reversed row tables, through both entries
    bel_rows, query_rows = [2, 0, 2], [1, 0, 0]
    want = np.stack([R.kde_logpdf(bel[i], pts[j], bw=bw[i]) for i, j in zip(bel_rows, query_rows)])
    assert np.array_equal(_bits(want[1]), _bits(block))
    for call in (_host, _dev):
        args = (dim, 3, N, bel, bel_rows, bw, Q, pts, query_rows)
        rc, out = call(_lib.LAYOUT_SOA, *args) if call is _host else call(*args)
        assert rc == 0 and np.array_equal(_bits(out), _bits(want)), call.__name__
    # no tables: pair p is (block p, block p); self-evaluation with a table reads the block the table names
    rc, out = _dev(dim, 2, N, bel, None, bw, Q, pts, None)
    assert rc == 0 and np.array_equal(_bits(out[0]), _bits(block))
    rc, out = _dev(dim, 2, N, bel, [2, 1], bw, N, None, None)
    assert rc == 0 and np.array_equal(_bits(out), _bits(np.stack([R.kde_logpdf(bel[i], bw=bw[i]) for i in (2, 1)])))


# ------------------------------------------------------------------------------------------------------------ normalisation
def test_density_integrates_to_one_on_a_grid():
    """Point2: N = 3, h = 0.3, 256 x 256 points on [−5, 5]² (spacing 0.13 h: the Riemann sum of a Gaussian is exact to rounding; the tails
    lie beyond 11 σ).  Pose2: 64³ points on [−5, 5]² x [−2, 2], h = (0.3, 0.3, 0.2), headings near 0 (spacing 0.53 h and 0.32 h: the
    aliasing term 2 exp(−2 π² h² / Δ²) is below 1e-30; tails beyond 9 σ).  Q = 65 536 and 262 144: every tile of a long 1-D grid."""
    g = np.linspace(-5.0, 5.0, 256)
    grid = np.stack([a.ravel() for a in np.meshgrid(g, g, indexing="ij")])
    bel = np.array([[0.5, -1.0, 0.2], [0.1, 0.8, -0.6]])
    lp = R.kde_logpdf(bel, grid, bw=[0.3, 0.3])
    total = float(np.sum(np.exp(lp))) * (g[1] - g[0]) ** 2
    print("Point2 grid: Σ p Δx Δy − 1 = %.2e" % (total - 1.0))
    assert lp.shape == (65536,) and abs(total - 1.0) <= 1e-10
    g, gt = np.linspace(-5.0, 5.0, 64), np.linspace(-2.0, 2.0, 64)
    grid = np.stack([a.ravel() for a in np.meshgrid(g, g, gt, indexing="ij")])
    bel = np.array([[0.5, -1.0, 0.2], [0.1, 0.8, -0.6], [0.15, -0.2, 0.05]])
    lp = R.kde_logpdf(bel, grid, bw=[0.3, 0.3, 0.2])
    total = float(np.sum(np.exp(lp))) * (g[1] - g[0]) ** 2 * (gt[1] - gt[0])
    print("Pose2 grid: Σ p Δx Δy Δθ − 1 = %.2e" % (total - 1.0))
    assert abs(total - 1.0) <= 1e-10


def test_one_particle_is_the_gaussian_log_pdf():
    y, h = np.array([[0.7], [-1.1]]), (0.3, 0.5)
    x = np.array([[0.9, -2.0, 0.7, 40.7], [-1.0, 3.0, -1.1, -1.1]])
    want = np.array([-0.5 * (((x[0, i] - 0.7) / 0.3) ** 2 + ((x[1, i] + 1.1) / 0.5) ** 2) - math.log(0.3 * 0.5) - math.log(2 * math.pi)
                     for i in range(4)])
    got = R.kde_logpdf(y, x, bw=h)
    assert (np.abs(got - want) <= K.ULP64 * np.maximum(1.0, np.abs(want))).all(), (got, want)
    # where q itself overflows it is saturated at 1e300 (the header's "finite for every finite input"): −½·1e300 and the constants
    beyond = R.kde_logpdf(np.array([[0.0, 1.0], [0.0, 1.0]]), np.array([[1e200, -1e300], [0.0, 1e300]]), bw=h)
    assert np.isfinite(beyond).all() and np.array_equal(beyond, np.full(2, -5e299))


# ------------------------------------------------------------------------------------------------------------ layouts
@pytest.mark.parametrize("dim", K.DIMS)
def test_host_and_device_entries_agree_in_every_layout(dim):
    """the coordinates are the device conversion's own image of native points (as tests/test_gpu_capi_layouts.py), so the three layouts
    carry the same values and every entry must return the same bits"""
    rng = np.random.default_rng(77 + dim)
    P, N, Q = 2, 70, 33
    sets = []
    for n in (N, Q):
        x = rng.standard_normal((P * n, dim)) * (1.0 if dim != 6 else np.array([2.0, 2.0, 2.0, 0.6, 0.6, 0.6]))
        pts = R.coords_to_points(dim, x)
        sets.append((pts.reshape(P, n, -1), R.points_to_coords(dim, pts).reshape(P, n, dim)))
    (pb, cb), (pq, cq) = sets
    soa = lambda c: np.ascontiguousarray(c.transpose(0, 2, 1))
    bw = np.abs(rng.standard_normal((P, dim))) * 0.5 + 0.1
    rc, want = _dev(dim, P, N, soa(cb), None, bw, Q, soa(cq), None)
    rc2, want_self = _dev(dim, P, N, soa(cb), None, bw, N, None, None, loo=1)
    assert rc == 0 and rc2 == 0 and np.isfinite(want).all() and np.isfinite(want_self).all()
    for layout, b, q in ((_lib.LAYOUT_SOA, soa(cb), soa(cq)), (_lib.LAYOUT_AOS, np.ascontiguousarray(cb), np.ascontiguousarray(cq)),
                         (_lib.LAYOUT_AOS_POINTS, np.ascontiguousarray(pb), np.ascontiguousarray(pq))):
        rc, out = _host(layout, dim, P, N, b, None, bw, Q, q, None)
        assert rc == 0 and np.array_equal(_bits(out), _bits(want)), layout
        rc, out = _host(layout, dim, P, N, b, None, bw, N, None, None, loo=1)
        assert rc == 0 and np.array_equal(_bits(out), _bits(want_self)), layout


# ------------------------------------------------------------------------------------------------------------ wrappers
@pytest.mark.parametrize("dim", (2, 3))
def test_kde_mode_returns_a_particle_of_the_heavier_cluster(dim):
    name = "mode/%d" % dim
    x, light = K.two_clusters(dim)
    ref = K.reference(name, "h03")
    best = int(np.argmax([float(v) for v in ref["mp"]]))
    gap = sorted(float(v) for v in ref["mp"])
    assert gap[-1] - gap[-2] > 2.0 * ref["tol"] * max(1.0, abs(gap[-1]))     # the mp argmax is not a tie the device could break otherwise
    pt, lp = R.kde_mode(x, bw=K.H03[dim])
    assert np.array_equal(pt, x[:, best]) and not light[best]
    assert abs(lp - float(ref["mp"][best])) <= ref["tol"] * max(1.0, abs(lp))
    pts, lps = R.kde_mode(np.stack([x, x[:, ::-1]]), bw=K.H03[dim])
    assert pts.shape == (2, dim) and lps.shape == (2,) and np.array_equal(pts[0], pt) and np.array_equal(pts[1], pt)
    # the coordinate-wise maximum need not be a particle; the joint mode always is
    assert any(np.array_equal(pt, x[:, j]) for j in range(x.shape[1]))


@pytest.mark.parametrize("dim", K.DIMS)
def test_kld_against_mp(dim):
    """kld(a, a) is exactly 0 (self-evaluation and evaluation at pts = a give the same bits); kld(a, b) within the mean of the per-point
    bounds of its two log-densities, plus (Na + 2) eps·mean |terms| for the float64 subtraction and mean"""
    a, b = K.kld_pair(dim)
    h = K.H03[dim]
    assert R.kld(a, a, bw_a=h, bw_b=h) == 0.0 and R.kld(a, a) == 0.0
    raa, rba = K.reference("kld_aa/%d" % dim, "h03"), K.reference("kld_ba/%d" % dim, "h03")
    with K.mpm.workdps(K.DPS):
        terms = [x - y for x, y in zip(raa["mp"], rba["mp"])]
        want = K.mpm.fsum(terms) / len(terms)
        bound = float(K.mpm.fsum(raa["tol"] * max(1, abs(x)) + rba["tol"] * max(1, abs(y)) for x, y in zip(raa["mp"], rba["mp"])) / len(terms))
        bound += (len(terms) + 2) * K.EPS * float(K.mpm.fsum(abs(t) for t in terms) / len(terms))
        got = R.kld(a, b, bw_a=h, bw_b=h)
        err = abs(float(K.mpm.mpf(got) - want))
    print("kld dim %d: %.12g (mp %s)  |Δ| = %.2e  bound %.2e" % (dim, got, K.mpm.nstr(want, 15), err, bound))
    assert got > 0.0 and err <= bound
    part = np.ascontiguousarray(b[:, :a.shape[1]])
    both = R.kld(np.stack([a, part]), np.stack([b, b]), bw_a=h, bw_b=h)
    assert both.shape == (2,) and _bits(both[0]) == _bits(got) and _bits(both[1]) == _bits(R.kld(part, b, bw_a=h, bw_b=h))
    assert np.isfinite(R.kld(a, b, leave_one_out=True))


def test_device_graph_logpdf_agrees_with_api_kde_logpdf():
    N = 100
    fg = R.generateGraph_Hexagonal(N=N)
    R.dead_reckon_init(fg, seed=3)
    fg.initVariable("l1", np.array([[20.0], [0.0]]) + np.random.default_rng(3).standard_normal((2, N)))
    dg = R.DeviceGraph(fg)
    dg.upload_beliefs(fg)
    rng = np.random.default_rng(8)
    for vt in (R.Pose2, R.Point2):
        labels = dg.packed.labels[vt]
        V, d, _ = dg.bel[vt].shape
        host = dg.bel[vt].cpu().numpy()
        Q = 37
        q = host[:, :, :Q] + 0.1 * rng.standard_normal((V, d, Q))
        tq = torch.as_tensor(q, device=dg.bel[vt].device)
        res, own, loo = dg.logpdf(vt, tq), dg.logpdf(vt), dg.logpdf(vt, leave_one_out=True)
        assert res.shape == (V, Q) and own.shape == (V, N) and res.is_cuda
        res, own, loo = res.cpu().numpy(), own.cpu().numpy(), loo.cpu().numpy()
        n = len(labels)
        assert np.array_equal(_bits(res[:n]), _bits(R.kde_logpdf(host[:n], q[:n])))
        assert np.array_equal(_bits(own[:n]), _bits(R.kde_logpdf(host[:n])))
        assert np.array_equal(_bits(loo[:n]), _bits(R.kde_logpdf(host[:n], leave_one_out=True)))
        assert np.array_equal(_bits(res[0]), _bits(R.evalBelief(fg, labels[0], q[0])))
        assert np.allclose(R.evalBelief(fg, labels[0], q[0], log=False), np.exp(res[0]), rtol=1e-15, atol=0)
        # capturable: with bandwidths and `out` given it is one launch and no allocation
        bw = dg.kde_bandwidths(vt)
        out = torch.zeros((V, Q), dtype=torch.float64, device=tq.device)
        g = dg.capture(lambda: dg.logpdf(vt, tq, bw=bw, out=out))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(out.cpu().numpy()[:n]), _bits(res[:n]))
        for bad in (dict(queries=tq[:, :, ::2]), dict(queries=tq[:, :d - 1].contiguous()), dict(queries=tq, leave_one_out=True),
                    dict(bw=bw[:, :d - 1].contiguous()), dict(out=out)):
            with pytest.raises(ValueError, match="DeviceGraph.logpdf"):
                dg.logpdf(vt, **bad)


def test_belief_log_likelihood_prefers_the_true_poses_of_a_solved_chain():
    """x0 (prior) -> x1 -> x2 by Pose2Pose2 (10, 0, π/3), N = 64, solved: the log-likelihood of the generator's poses under the solved
    beliefs is higher than that of the same poses moved by 3 m, variable by variable; one library call per variable type"""
    fg = R.initfg(64)
    fg.addVariable("x0", R.Pose2)
    fg.addFactor(["x0"], R.PriorPose2(R.MvNormal(np.zeros(3), 0.01 * np.eye(3))))
    for i in range(2):
        fg.addVariable("x%d" % (i + 1), R.Pose2)
        fg.addFactor(["x%d" % i, "x%d" % (i + 1)], R.Pose2Pose2(R.MvNormal([10.0, 0.0, math.pi / 3], np.diag([0.1, 0.1, 0.1]) ** 2)))
    R.solveGraph(fg, n_sweeps=6, seed=5)
    truth = {"x0": [0.0, 0.0, 0.0], "x1": [10.0, 0.0, math.pi / 3], "x2": [15.0, 10.0 * math.sin(math.pi / 3), 2 * math.pi / 3]}
    ll = R.beliefLogLikelihood(fg, truth)
    moved = R.beliefLogLikelihood(fg, {l: [x + 3.0, y, th] for l, (x, y, th) in truth.items()})
    print("log-likelihood at the true poses %s, moved by 3 m %s" % (ll, moved))
    assert list(ll) == list(truth) and all(np.isfinite(v) for v in ll.values()) and all(np.isfinite(v) for v in moved.values())
    assert all(ll[l] > moved[l] for l in truth)
    assert _bits(ll["x1"]) == _bits(R.evalBelief(fg, "x1", np.array(truth["x1"])[:, None])[0])
    k = R.kldBeliefs(fg, fg)
    assert list(k) == fg.ls() and all(v == 0.0 for v in k.values())


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    rng = np.random.default_rng(9)
    bel, q, bw = rng.standard_normal((2, 3, 8)), rng.standard_normal((2, 3, 5)), np.full((2, 3), 0.3)
    ok = lambda **kw: dict(dict(layout=_lib.LAYOUT_SOA, dim=3, P=2, N=8, bel=bel, bel_rows=None, bw=bw, Q=5, queries=q, query_rows=None), **kw)
    both = lambda **kw: [_host(**ok(**kw))[0], _dev(**{k: v for k, v in ok(**kw).items() if k not in ("layout", "n_bel", "n_q")})[0]]
    INV, UNS = _lib.ERR_INVALID_ARG, _lib.ERR_UNSUPPORTED_N
    assert both() == [0, 0] and both(Q=8, queries=None, loo=1) == [0, 0]
    assert both(dim=4) == [INV, INV] and both(dim=1) == [INV, INV]
    assert both(loo=1) == [INV, INV]                                            # leave-one-out with queries
    one = rng.standard_normal((2, 3, 1))
    assert both(N=1, bel=one, Q=1, queries=None, loo=1) == [INV, INV]           # ... or with one particle
    assert both(N=1, bel=one, Q=1, queries=None) == [0, 0]
    assert both(Q=5, queries=None) == [INV, INV]                                # self-evaluation needs Q == N
    assert both(P=-1) == [INV, INV] and both(N=0) == [INV, INV] and both(Q=-1) == [INV, INV]
    # P = 0 or Q = 0: a no-op that writes nothing
    for kw in (dict(P=0), dict(Q=0)):
        for rc, out in (_host(**ok(**kw)), _dev(**{k: v for k, v in ok(**kw).items() if k != "layout"})):
            assert rc == 0 and np.isnan(out).all()
    # N = 513: refused before any launch, by both entries
    big = rng.standard_normal((1, 3, 513))
    assert both(P=1, N=513, bel=big, bw=bw[:1]) == [UNS, UNS]
    assert both(P=1, N=513, bel=big, bw=bw[:1], Q=513, queries=None) == [UNS, UNS]
    assert _host(**ok(P=1, N=512, bel=rng.standard_normal((1, 3, 512)), bw=bw[:1], queries=q[:1]))[0] == 0
    # host entry only: bandwidths, layout, and row tables (or P without them) that leave the arrays
    for v in (0.0, -0.3, float("nan"), float("inf")):
        h = bw.copy(); h[1, 2] = v
        assert _host(**ok(bw=h))[0] == INV
    assert _host(**ok(layout=3))[0] == INV
    assert _host(**ok(bel_rows=[0, 2]))[0] == INV and _host(**ok(query_rows=[-1, 0]))[0] == INV and _host(**ok(P=3))[0] == INV
    assert _host(**ok(n_q=1))[0] == INV and _host(**ok(n_bel=1))[0] == INV
    # needed pointers
    lib, ctx = _lib.load(), R.default_context()
    out = np.zeros((2, 5))
    assert lib.rome_kde_eval(ctx.handle, 0, 3, 2, 8, 2, None, None, _p(bw), 5, 2, _p(q), None, 0, _p(out)) == INV
    assert lib.rome_kde_eval(ctx.handle, 0, 3, 2, 8, 2, _p(bel), None, None, 5, 2, _p(q), None, 0, _p(out)) == INV
    assert lib.rome_kde_eval(ctx.handle, 0, 3, 2, 8, 2, _p(bel), None, _p(bw), 5, 2, _p(q), None, 0, None) == INV
    assert lib.rome_kde_eval_dev(ctx.handle, 3, 2, 8, None, None, None, 5, None, None, 0, None) == INV
    assert lib.rome_kde_eval(None, 0, 3, 2, 8, 2, _p(bel), None, _p(bw), 5, 2, _p(q), None, 0, _p(out)) == INV
    with pytest.raises(R.RomeError) as e:       # the wrapper refuses N = 513 itself; the library's own code comes through the raw entry
        _lib.check(lib.rome_kde_eval(ctx.handle, 0, 3, 1, 513, 1, _p(big), None, _p(bw), 513, 0, None, None, 0, _p(np.zeros(513))), ctx.handle)
    assert e.value.code == UNS
