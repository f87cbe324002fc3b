"""numpy-facing wrappers of the host-pointer C-ABI entry points (include/rome_mi355.h).

`calcFactorResidualTemporary` mirrors the IIF helper the reference's known-answer tests use
(test/testBearingRange2D.jl:64, test/testParametricSimulated.jl:40, test/testPartialPose3.jl:430).
"""
import ctypes as C

import numpy as np

from . import _lib
from .factors import (Pose2, Point2, Pose3, Pose2Pose2, PriorPose2, Pose2Point2BearingRange, Pose3Pose3,
                      PriorPose3, Point2Point2Range, Pose2Point2Range, Pose2Point2Bearing, Pose3Pose3XYYaw, Pose3Pose3Rotation, getCoordinates)

_PD = C.POINTER(C.c_double)
_PI = C.POINTER(C.c_int32)

_default_ctx = None


def default_context():
    """Process-wide Context on device 0 (raises without a GPU: no CPU fallback)."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = _lib.Context(0)
    return _default_ctx


def _d(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError("expected array of shape %s, got %s" % (tuple(shape), a.shape))
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(_PD)


def _pi(a):
    return None if a is None else a.ctypes.data_as(_PI)


# ------------------------------------------------------------------ residuals
def _rows(fn, ctx, ins, widths, out_w):
    ctx = ctx or default_context()
    arrs = [np.atleast_2d(_d(a)) for a in ins]
    n = arrs[0].shape[0]
    for a, w in zip(arrs, widths):
        if a.shape != (n, w):
            raise ValueError("expected (%d,%d) rows, got %s" % (n, w, a.shape))
    out = np.empty((n, out_w))
    _lib.check(fn(ctx.handle, n, *[_p(a) for a in arrs], _p(out)), ctx.handle)
    return out


def residual_pose2pose2(z, p, q, ctx=None):
    return _rows(_lib.load().rome_residual_pose2pose2, ctx, (z, p, q), (3, 3, 3), 3)


def residual_priorpose2(m, p, ctx=None):
    return _rows(_lib.load().rome_residual_priorpose2, ctx, (m, p), (3, 3), 3)


def residual_pose2point2br(z, p, l, ctx=None):
    return _rows(_lib.load().rome_residual_pose2point2br, ctx, (z, p, l), (2, 3, 2), 2)


def residual_pose2point2br_pt(z, p_pt, l, ctx=None):
    return _rows(_lib.load().rome_residual_pose2point2br_pt, ctx, (z, p_pt, l), (2, 6, 2), 2)


def residual_pose3pose3(z, p, q, ctx=None):
    return _rows(_lib.load().rome_residual_pose3pose3, ctx, (z, p, q), (6, 6, 6), 6)


def residual_pose3pose3_pt(z, p_pt, q_pt, ctx=None):
    return _rows(_lib.load().rome_residual_pose3pose3_pt, ctx, (z, p_pt, q_pt), (6, 12, 12), 6)


def residual_priorpose3(m, p, ctx=None):
    return _rows(_lib.load().rome_residual_priorpose3, ctx, (m, p), (6, 6), 6)


def residual_point2point2range(z, xi, lm, ctx=None):
    """r = ρ − ‖lm − xi‖ per row (Range2D.jl:14-17): z (n,) ranges, xi / lm (n, 2) -> (n,)"""
    z = np.atleast_1d(_d(z)).reshape(-1, 1)
    return _rows(_lib.load().rome_residual_point2point2range, ctx, (z, xi, lm), (1, 2, 2), 1)[:, 0]


def residual_pose2point2range(z, p, lm, ctx=None):
    """r = ρ − ‖lm − p.t‖ per row (Range2D.jl:51-54): z (n,), p (n, 3) pose coordinates (heading not read), lm (n, 2) -> (n,)"""
    z = np.atleast_1d(_d(z)).reshape(-1, 1)
    return _rows(_lib.load().rome_residual_pose2point2range, ctx, (z, p, lm), (1, 3, 2), 1)[:, 0]


def residual_pose2point2bearing(z, p, l, ctx=None):
    """r = sym_rem(b − atan2(pl)), pl = R(θp)ᵀ (l − p.t) per row (Bearing2D.jl:23-32): z (n,) bearings, p (n, 3), l (n, 2) -> (n,)"""
    z = np.atleast_1d(_d(z)).reshape(-1, 1)
    return _rows(_lib.load().rome_residual_pose2point2bearing, ctx, (z, p, l), (1, 3, 2), 1)[:, 0]


def residual_pose2point2bearing_pt(z, p_pt, l, ctx=None):
    """the same with the poses as native points (n, 6)"""
    z = np.atleast_1d(_d(z)).reshape(-1, 1)
    return _rows(_lib.load().rome_residual_pose2point2bearing_pt, ctx, (z, p_pt, l), (1, 6, 2), 1)[:, 0]


def residual_pose3pose3xyyaw(z, p, q, ctx=None):
    """the Pose2Pose2 residual of the SE(2) projections (t_xy, yaw) of p and q per row (PartialPose3.jl:116-136): z (n, 3) = (x, y, θ),
    p / q (n, 6) Pose3 coordinates -> (n, 3)"""
    return _rows(_lib.load().rome_residual_pose3pose3xyyaw, ctx, (z, p, q), (3, 6, 6), 3)


def residual_pose3pose3xyyaw_pt(z, p_pt, q_pt, ctx=None):
    """the same with the poses as native points (n, 12)"""
    return _rows(_lib.load().rome_residual_pose3pose3xyyaw_pt, ctx, (z, p_pt, q_pt), (3, 12, 12), 3)


def residual_pose3pose3rotation(z, p, q, ctx=None):
    """z − Log(R_pᵀ R_q) per row (PartialPose3.jl:212-227): z (n, 3) rotation vectors, p / q (n, 6) Pose3 coordinates -> (n, 3)"""
    return _rows(_lib.load().rome_residual_pose3pose3rotation, ctx, (z, p, q), (3, 6, 6), 3)


def residual_pose3pose3rotation_pt(z, p_pt, q_pt, ctx=None):
    """the same with the poses as native points (n, 12)"""
    return _rows(_lib.load().rome_residual_pose3pose3rotation_pt, ctx, (z, p_pt, q_pt), (3, 12, 12), 3)


def _same(m):
    return m


def _se2_tangent(m):     # ((x, y), [0 -θ; θ 0]) column-major
    return np.array([m[0], m[1], m[3]])


def _se3_tangent(m):     # (t, skew) -> (X32, X13, X21)
    return np.array([m[0], m[1], m[2], m[3 + 5], m[3 + 6], m[3 + 1]])


# factor class -> ({measurement length: its coordinates}, variable types, residual on rows of coordinates, residual on rows of native
# points or None).  The lengths are the plain coordinates and the reference's tangent container (hat form).  A factor with a native-point
# residual is given its points as they come (the first point's length selects the function); for the others a native point is converted
# to coordinates.  Looked up along the factor's classes (_residual_entry), as isinstance would.
_RESIDUALS = {
    Pose2Pose2: ({3: _same, 6: _se2_tangent}, (Pose2, Pose2), residual_pose2pose2, None),
    # the prior residual is evaluated between the sampled measurement POINT and the variable
    PriorPose2: ({3: _same, 6: _se2_tangent}, (Pose2,), residual_priorpose2, None),
    Pose2Point2BearingRange: ({2: _same, 5: lambda m: np.array([m[1], m[4]])},     # ([0 -b; b 0], [ρ])
                              (Pose2, Point2), residual_pose2point2br, residual_pose2point2br_pt),
    Point2Point2Range: ({1: _same}, (Point2, Point2), residual_point2point2range, None),     # the range sample ρ
    Pose2Point2Range: ({1: _same}, (Pose2, Point2), residual_pose2point2range, None),
    Pose2Point2Bearing: ({1: _same, 4: lambda m: m[1:2]},     # [0 -b; b 0] column-major (the so(2) tangent the reference samples)
                         (Pose2, Point2), residual_pose2point2bearing, residual_pose2point2bearing_pt),
    # an SE(2) tangent (getManifold PartialPose3.jl:112)
    Pose3Pose3XYYaw: ({3: _same, 6: _se2_tangent}, (Pose3, Pose3), residual_pose3pose3xyyaw, residual_pose3pose3xyyaw_pt),
    # an SO(3) tangent (getManifold PartialPose3.jl:210): skew matrix column-major -> (X32, X13, X21)
    Pose3Pose3Rotation: ({3: _same, 9: lambda m: np.array([m[5], m[6], m[1]])},
                         (Pose3, Pose3), residual_pose3pose3rotation, residual_pose3pose3rotation_pt),
    Pose3Pose3: ({6: _same, 12: _se3_tangent}, (Pose3, Pose3), residual_pose3pose3, residual_pose3pose3_pt),
    PriorPose3: ({6: _same, 12: _se3_tangent}, (Pose3,), residual_priorpose3, None),
}


def _residual_entry(factor):
    for cls in type(factor).__mro__:
        if cls in _RESIDUALS:
            return _RESIDUALS[cls]
    return {}, (), None, None


def _meas_coords(factor, meas):
    """Accepts the reference's tangent containers (hat form) or plain coordinates."""
    m = np.asarray(meas, dtype=np.float64).ravel()
    coords = _residual_entry(factor)[0].get(m.size)
    if coords is None:
        raise ValueError("measurement of unexpected length %d for %s" % (m.size, type(factor).__name__))
    return coords(m)


def calcFactorResidualTemporary(factor, vartypes, meas, points, ctx=None):
    """Residual of `factor` for one measurement and one point per variable (native point layouts,
    or coordinate vectors of the variable's dimension)."""
    z = _meas_coords(factor, meas)
    _, types, on_coords, on_points = _residual_entry(factor)
    pts = [np.asarray(p, dtype=np.float64).ravel() for p in points][:len(types)]
    if on_points is not None:
        fn = on_points if pts[0].size == types[0].point_len else on_coords
    else:
        fn, pts = on_coords, [p if p.size == t.dim else getCoordinates(t, p) for t, p in zip(types, pts)]
    return fn([z], *[[p] for p in pts], ctx)[0]


# ------------------------------------------------------------------ parametric linearisation
_LIN_DIMS = {_lib.FACTOR_PRIORPOSE2: (3, 3, 3, 0), _lib.FACTOR_POSE2POSE2: (3, 3, 3, 3), _lib.FACTOR_POSE2POINT2BR: (2, 2, 3, 2),
             _lib.FACTOR_PRIORPOINT2: (2, 2, 2, 0), _lib.FACTOR_POSE3POSE3: (6, 6, 6, 6), _lib.FACTOR_PRIORPOSE3: (6, 6, 6, 0),
             _lib.FACTOR_POSE2POINT2BEARING: (1, 1, 3, 2)}


def linearize(kind, mu, W, xa, xb=None, ctx=None):
    """Whitened residuals and Jacobians of F factors of one kind (rome_linearize):
    -> r (F,dr), Ja (F,dr,da), Jb (F,dr,db) or None."""
    ctx = ctx or default_context()
    dz, dr, da, db = _LIN_DIMS[kind]
    mu = np.atleast_2d(_d(mu)); F = mu.shape[0]
    mu = _d(mu, (F, dz)); W = _d(W, (F, dr, dr)); xa = _d(xa, (F, da))
    r = np.empty((F, dr)); Ja = np.empty((F, dr, da))
    if db:
        xb = _d(xb, (F, db)); Jb = np.empty((F, dr, db))
    else:
        xb = None; Jb = None
    _lib.check(_lib.load().rome_linearize(ctx.handle, int(kind), F, _p(mu), _p(W), _p(xa), _p(xb), _p(r), _p(Ja), _p(Jb)), ctx.handle)
    return r, Ja, Jb


def belief_stats(bel, ctx=None):
    """bel (V, dim, N) host array -> (mean (V,dim), std (V,dim)) via rome_belief_stats."""
    ctx = ctx or default_context()
    bel = _d(bel)
    V, d, N = bel.shape
    mean = np.empty((V, d)); sd = np.empty((V, d))
    _lib.check(_lib.load().rome_belief_stats(ctx.handle, d, V, N, _p(bel), _p(mean), _p(sd)), ctx.handle)
    return mean, sd


def _mmd_call(a, b, bw, scale, want_sums, ctx):
    """a (Va, dim, Na), b (Vb, dim, Nb) host SoA blocks, pair v = (a[v], b[v]) -> out (V,), sums (V, 3) or None: one rome_mmd call"""
    ctx = ctx or default_context()
    (V, d, Na), (Vb, db, Nb) = a.shape, b.shape
    if Vb != V or db != d:
        raise ValueError("mmd: the two sets must have the same number of blocks and coordinates, got %s and %s" % (a.shape, b.shape))
    sc = None if scale is None else _d(scale, (d,))
    out = np.empty(V)
    sums = np.empty((V, 3)) if want_sums else None
    _lib.check(_lib.load().rome_mmd(ctx.handle, _lib.LAYOUT_SOA, d, V, Na, V, _p(a), None, Nb, V, _p(b), None, _p(sc), float(bw), _p(out), _p(sums)),
               ctx.handle)
    return out, sums


def mmd(a, b, bw=0.001, scale=None, return_sums=False, ctx=None):
    """⚠AMP `mmd(M, a, b; bw=[bw])`: maximum mean discrepancy (biased V-statistic of MMD², include/rome_mi355.h rome_mmd) between two
    particle sets of one variable type.  a (dim, Na) and b (dim, Nb) host coordinates -> a float; a (V, dim, Na) and b (V, dim, Nb) ->
    (V,) values, block v against block v.  dim 2: Point2, 3: Pose2, 6: Pose3 coordinates (t, ω).  scale: (dim,) per-coordinate weights,
    None = ones.  return_sums: also the three kernel sums (S_aa, S_ab, S_bb) per pair."""
    a, b = _d(a), _d(b)
    if a.ndim != b.ndim or a.ndim not in (2, 3):
        raise ValueError("mmd: expected two (dim, N) or two (V, dim, N) arrays, got %s and %s" % (a.shape, b.shape))
    single = a.ndim == 2
    out, sums = _mmd_call(a[None] if single else a, b[None] if single else b, bw, scale, return_sums, ctx)
    if single:
        return (float(out[0]), sums[0]) if return_sums else float(out[0])
    return (out, sums) if return_sums else out


def mmdBeliefs(fg_a, fg_b, labels=None, bw=0.001, scale=None, ctx=None):
    """{label: mmd(belief of label in fg_a, belief of label in fg_b)} for `labels` (default: every variable of fg_a), one library call
    per variable type.  scale: None, (dim,) weights, or {vartype: (dim,) weights}.  A label that is missing or uninitialised in either
    graph raises, by name."""
    labels = list(fg_a.ls() if labels is None else labels)
    by_type = {}
    for l in labels:
        for name, fg in (("first", fg_a), ("second", fg_b)):
            if not fg.exists(l) or not fg.isInitialized(l):
                raise ValueError("mmdBeliefs: variable %s is not initialised in the %s graph" % (l, name))
        if fg_a.variables[l] is not fg_b.variables[l]:
            raise ValueError("mmdBeliefs: variable %s has different types in the two graphs" % l)
        by_type.setdefault(fg_a.variables[l], []).append(l)
    res = {}
    for vt, ls in by_type.items():
        a = np.stack([fg_a.getVal(l) for l in ls])
        b = np.stack([fg_b.getVal(l) for l in ls])
        out, _ = _mmd_call(_d(a), _d(b), bw, scale.get(vt) if isinstance(scale, dict) else scale, False, ctx)
        res.update(zip(ls, out.tolist()))
    return {l: res[l] for l in labels}


def _kde_eval_call(name, bel, pts, bw, leave_one_out, ctx):
    """bel (V, dim, N), pts (V, dim, Q) or None (self-evaluation), bw (V, dim), (dim,) or None (kde_bandwidth) -> (V, Q) log-densities:
    one rome_kde_eval call.  Everything the library would refuse is refused here first, by name and without a device."""
    V, d, N = bel.shape
    if d not in (2, 3, 6):
        raise ValueError("%s: beliefs must have 2 (Point2), 3 (Pose2) or 6 (Pose3) coordinates, got %d" % (name, d))
    if N < 1 or N > _lib.MAX_PARTICLES_KDE_EVAL:
        raise ValueError("%s: 1 <= N <= %d particles, got %d" % (name, _lib.MAX_PARTICLES_KDE_EVAL, N))
    if pts is not None and (pts.shape[0] != V or pts.shape[1] != d):
        raise ValueError("%s: the query points must be (%d, %d, Q) like the beliefs %s, got %s" % (name, V, d, bel.shape, pts.shape))
    if leave_one_out and (pts is not None or N < 2):
        raise ValueError("%s: leave_one_out applies to self-evaluation (pts=None) of at least 2 particles" % name)
    if bw is not None:
        bw = _d(bw)
        if bw.shape not in ((d,), (V, d)):
            raise ValueError("%s: bandwidths must be (%d,) or (%d, %d), got %s" % (name, d, V, d, bw.shape))
        bw = np.ascontiguousarray(np.broadcast_to(bw, (V, d)))
        if not (np.isfinite(bw) & (bw > 0.0)).all():
            raise ValueError("%s: bandwidths must be finite and positive" % name)
    ctx = ctx or default_context()
    if bw is None:
        bw = kde_bandwidth(bel, ctx=ctx)
    Q = N if pts is None else pts.shape[2]
    out = np.empty((V, Q))
    _lib.check(_lib.load().rome_kde_eval(ctx.handle, _lib.LAYOUT_SOA, d, V, N, V, _p(bel), None, _p(bw), Q, 0 if pts is None else V, _p(pts), None,
                                         1 if leave_one_out else 0, _p(out)), ctx.handle)
    return out


def _eval_blocks(name, a, what):
    a = _d(a)
    if a.ndim not in (2, 3):
        raise ValueError("%s: %s must be (dim, N) or (V, dim, N), got %s" % (name, what, a.shape))
    return (a[None], True) if a.ndim == 2 else (a, False)


def kde_logpdf(bel, pts=None, bw=None, leave_one_out=False, ctx=None):
    """⚠the belief called as a function (`getBelief(fg, :x)(pts)`, AMP `evaluateDualTree`): log-density of the kernel density estimate
    of bel at pts (include/rome_mi355.h rome_kde_eval: tangent coordinates, normalisation not checked against AMP).  bel (dim, N) and pts
    (dim, Q) -> (Q,); bel (V, dim, N) and pts (V, dim, Q) -> (V, Q), block v at block v.  pts=None: at the belief's own particles;
    leave_one_out then leaves each particle out of its own density.  bw (dim,) or (V, dim) kernel bandwidths; None selects them with
    kde_bandwidth, as kde_max does."""
    bel, single = _eval_blocks("kde_logpdf", bel, "bel")
    if pts is not None:
        pts, psingle = _eval_blocks("kde_logpdf", pts, "pts")
        if psingle != single:
            raise ValueError("kde_logpdf: bel and pts must both be one block or both be stacks of blocks")
    out = _kde_eval_call("kde_logpdf", bel, pts, bw, leave_one_out, ctx)
    return out[0] if single else out


def kde_mode(bel, bw=None, ctx=None):
    """Joint mode estimate of V beliefs: each belief's own particle of highest joint density (first on ties), the argmax of the
    self-evaluation without leave-one-out -- unlike kde_max (getKDEMax), which works coordinate by coordinate and can return a point
    that belongs to no mode.  bel (V, dim, N) -> (V, dim) points, (V,) log-densities; bel (dim, N) -> (dim,), float."""
    bel, single = _eval_blocks("kde_mode", bel, "bel")
    lp = _kde_eval_call("kde_mode", bel, None, bw, False, ctx)
    k = np.argmax(lp, axis=1)
    v = np.arange(bel.shape[0])
    pts, best = bel[v, :, k], lp[v, k]
    return (pts[0], float(best[0])) if single else (pts, best)


def kld(a, b, bw_a=None, bw_b=None, leave_one_out=False, ctx=None):
    """⚠unvendored: KDE.jl's direct estimate of the Kullback-Leibler divergence, written from recollection and NOT CHECKED against
    KDE.jl: kld(a, b) = mean_i [log p_a(a_i) − log p_b(a_i)] with both densities evaluated by kde_logpdf, each with its own
    bandwidths (bw_a, bw_b; None = kde_bandwidth).  leave_one_out leaves a_i out of p_a.  a (dim, Na), b (dim, Nb) -> float;
    (V, dim, Na), (V, dim, Nb) -> (V,).  Not symmetric; an estimate, so it can be slightly negative."""
    a, single = _eval_blocks("kld", a, "a")
    b, bsingle = _eval_blocks("kld", b, "b")
    if bsingle != single or b.shape[:2] != a.shape[:2]:
        raise ValueError("kld: the two sets must have the same number of blocks and coordinates, got %s and %s" % (a.shape, b.shape))
    la = _kde_eval_call("kld", a, None, bw_a, leave_one_out, ctx)
    lb = _kde_eval_call("kld", b, a, bw_b, False, ctx)
    out = np.mean(la - lb, axis=1)
    return float(out[0]) if single else out


def _initialised(name, fg, label, which=""):
    if not fg.exists(label) or not fg.isInitialized(label):
        raise ValueError("%s: variable %s is not initialised%s" % (name, label, which))


def evalBelief(fg, label, pts, log=True):
    """The belief of `label` called as a function, `getBelief(fg, label)(pts)`: its density at pts (dim, Q) -> (Q,); log=True returns
    the log-density (kde_logpdf, bandwidths by kde_bandwidth), which does not underflow far from the particles."""
    _initialised("evalBelief", fg, label)
    lp = kde_logpdf(fg.getVal(label), pts)
    return lp if log else np.exp(lp)


def beliefLogLikelihood(fg, truth):
    """{label: log-density of the belief of label at truth[label]} for truth = {label: coordinates (dim,)} -- what
    examples/RangesExampleTwo.jl:388-400 prints after every solve.  One kde_bandwidth and one rome_kde_eval call per variable type.
    A label that is missing or uninitialised raises, by name."""
    by_type = {}
    for l in truth:
        _initialised("beliefLogLikelihood", fg, l)
        vt = fg.variables[l]
        x = _d(truth[l]).reshape(-1)
        if x.shape != (vt.dim,):
            raise ValueError("beliefLogLikelihood: truth[%s] must have %d coordinates, got %s" % (l, vt.dim, x.shape))
        by_type.setdefault(vt, []).append((l, x))
    res = {}
    for vt, items in by_type.items():
        bel = _d(np.stack([fg.getVal(l) for l, _ in items]))
        pts = _d(np.stack([x for _, x in items])[:, :, None])
        lp = _kde_eval_call("beliefLogLikelihood", bel, pts, None, False, None)
        res.update((l, float(v)) for (l, _), v in zip(items, lp[:, 0]))
    return {l: res[l] for l in truth}


def kldBeliefs(fg_a, fg_b, labels=None):
    """{label: kld(belief of label in fg_a, belief of label in fg_b)} for `labels` (default: every variable of fg_a), by variable type.
    A label that is missing or uninitialised in either graph raises, by name."""
    labels = list(fg_a.ls() if labels is None else labels)
    by_type = {}
    for l in labels:
        _initialised("kldBeliefs", fg_a, l, " in the first graph")
        _initialised("kldBeliefs", fg_b, l, " in the second graph")
        if fg_a.variables[l] is not fg_b.variables[l]:
            raise ValueError("kldBeliefs: variable %s has different types in the two graphs" % l)
        by_type.setdefault(fg_a.variables[l], []).append(l)
    res = {}
    for vt, ls in by_type.items():
        out = kld(np.stack([fg_a.getVal(l) for l in ls]), np.stack([fg_b.getVal(l) for l in ls]))
        res.update(zip(ls, out.tolist()))
    return {l: res[l] for l in labels}


def kde_bandwidth(bel, circular_mask=None, tol_euclid=0.0, tol_circular=0.0, ctx=None):
    """bel (V, dim, N) host array -> (V, dim) bandwidths as `manikde!` selects them (leave-one-out likelihood
    cross-validation per coordinate), via rome_kde_bandwidth.  circular_mask: bit k set = coordinate k is an angle
    (default: 0b100 for dim 3 -- Pose2 --, 0 otherwise); tol_* = 0 selects the reference's stopping rules."""
    ctx = ctx or default_context()
    bel = _d(bel)
    V, d, N = bel.shape
    if circular_mask is None:
        circular_mask = 0b100 if d == 3 else 0
    bw = np.empty((V, d))
    _lib.check(_lib.load().rome_kde_bandwidth(ctx.handle, d, V, N, _p(bel), int(circular_mask), float(tol_euclid),
                                              float(tol_circular), _p(bw)), ctx.handle)
    return bw


def manifoldProduct(proposals, circular_mask=None, bandwidths=None, Niter=1, opts=None, ctx=None):
    """⚠AMP `manifoldProduct(ff, manifold; Niter=1)`: N samples from the product of K kernel density estimates by multiscale Gibbs
    sampling (rome_product_gibbs_dev).  proposals (K, dim, N) host array (dim 2: Point2, 3: Pose2, 6: Pose3 coordinates (t, ω));
    bandwidths (K, dim) or None = the `manikde!` rule (kde_bandwidth; Pose3: rotation-vector coordinates as circular).
    -> (dim, N).  K = 1 returns the density's own points, as AMP does."""
    import torch
    ctx = ctx or default_context()
    P = _d(proposals)
    K, d, N = P.shape
    if circular_mask is None:
        circular_mask = 0b100 if d == 3 else 0
    bw = kde_bandwidth(P, 0b111000 if d == 6 else circular_mask, ctx=ctx) if bandwidths is None else _d(bandwidths, (K, d))
    if d == 6:
        circular_mask = 0     # rotations live in the chart of each density: no wrapped coordinate
    o = opts if opts is not None else make_opts(N=N)
    dev = torch.device("cuda", ctx.device if hasattr(ctx, "device") else 0)
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=dev)
    tp, tb = t(P, torch.float64), t(bw, torch.float64)
    ptr, rows = t([0, K], torch.int32), t(np.arange(K), torch.int32)
    bin_, out = torch.zeros((1, d, N), dtype=torch.float64, device=dev), torch.empty((1, d, N), dtype=torch.float64, device=dev)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(_lib.load().rome_product_gibbs_dev(ctx.handle, C.byref(o), d, 1, ptr.data_ptr(), rows.data_ptr(), tp.data_ptr(), tb.data_ptr(), K,
                                                  bin_.data_ptr(), out.data_ptr(), int(circular_mask), int(Niter), max(1, K)), ctx.handle)
    torch.cuda.synchronize(dev)
    return out[0].cpu().numpy()


def product_partial(opts, dim, tasks, prop, bel, prop_bw=None, joint_bw=None, circular_mask=None, ctx=None):
    """Stage 2 of the partial-aware product on host arrays, via rome_product_partial.  tasks: the dict of
    device.partial_tasks (task_var, task_coord, task_ptr, task_rows, task_joint); prop (rows, dim, N) the proposals; bel (V, dim, N)
    the stage-1 result J; prop_bw (rows, dim) / joint_bw (V, dim) kernel bandwidths or None = Silverman's rule; circular_mask: bit c
    set = coordinate c is an angle (default 0b100 for dim 3, 0b111000 for dim 6).  -> the new bel (V, dim, N): every task's line
    replaced by the 1-D product of its densities, every other line J's, bit for bit.  The tables are validated here: the library
    trusts them."""
    prop, bel = _d(prop), _d(bel).copy()
    (n_rows, V), N = (prop.shape[0], bel.shape[0]), opts.n_particles
    if prop.shape[1:] != (dim, N) or bel.shape[1:] != (dim, N):
        raise ValueError("product_partial: prop / bel must be (rows, %d, %d) / (V, %d, %d), got %s / %s" % (dim, N, dim, N, prop.shape, bel.shape))
    tv, tc, tp, tr, tj = (np.ascontiguousarray(tasks[k], dtype=np.int32) for k in ("task_var", "task_coord", "task_ptr", "task_rows", "task_joint"))
    T = len(tv)
    if not (len(tc) == T and len(tj) == T and len(tp) == T + 1):
        raise ValueError("product_partial: task tables of different lengths")
    if T:
        if tp[0] != 0 or (np.diff(tp) < 1).any() or tp[-1] != len(tr):
            raise ValueError("product_partial: task_ptr must start at 0, give every task at least one row and end at len(task_rows)")
        if tv.min() < 0 or tv.max() >= V or tc.min() < 0 or tc.max() >= dim or tr.min() < 0 or tr.max() >= n_rows:
            raise ValueError("product_partial: a task names a variable, coordinate or row outside the arrays")
        if len(set(zip(tv.tolist(), tc.tolist()))) != T:
            raise ValueError("product_partial: a (variable, coordinate) line has more than one task")
    if circular_mask is None:
        circular_mask = 0b100 if dim == 3 else (0b111000 if dim == 6 else 0)
    pbw = None if prop_bw is None else _d(prop_bw, (n_rows, dim))
    jbw = None if joint_bw is None else _d(joint_bw, (V, dim))
    one = lambda a: a if len(a) else np.zeros(1, np.int32)
    tv, tc, tr, tj = one(tv), one(tc), one(tr), one(tj)
    ctx = ctx or default_context()
    _lib.check(_lib.load().rome_product_partial(ctx.handle, C.byref(opts), int(dim), V, T, _pi(tv), _pi(tc), _pi(tp), _pi(tr), _pi(tj), _p(prop),
                                                _p(pbw), _p(jbw), int(circular_mask), _p(bel), n_rows), ctx.handle)
    return bel


def kde_max(bel, bw=None, grid_points=0, ctx=None):
    """bel (V, dim, N) host array -> (V, dim) max-density coordinates as IIF's getKDEMax computes them (PPE `max`), via rome_kde_max.
    bw (V, dim): kernel bandwidths; None selects them with kde_bandwidth (what `manikde!` would have stored)."""
    ctx = ctx or default_context()
    bel = _d(bel)
    V, d, N = bel.shape
    bw = kde_bandwidth(bel, ctx=ctx) if bw is None else _d(bw, (V, d))
    out = np.empty((V, d))
    _lib.check(_lib.load().rome_kde_max(ctx.handle, d, V, N, _p(bel), _p(bw), int(grid_points), _p(out)), ctx.handle)
    return out


def calcPPE(bel, bw=None, ctx=None):
    """Point estimates of V beliefs as the reference's calcVariablePPE stores them: dict(mean, max, suggested), each (V, dim).
    `suggested` follows the solved graph the reference ships (examples/fg-after-solve.tar.gz): mean translation, max-density heading for
    Pose2; the mean otherwise."""
    bel = _d(bel)
    mean, _ = belief_stats(bel, ctx)
    mx = kde_max(bel, bw, ctx=ctx)
    sug = mean.copy()
    if bel.shape[1] == 3:
        sug[:, 2] = mx[:, 2]
    return {"mean": mean, "max": mx, "suggested": sug}


# ------------------------------------------------------------------ helpers
def cholesky_lower(cov):
    """n covariances (n,d,d) or one (d,d) -> packed lower factors (n, d(d+1)/2)."""
    cov = _d(cov)
    single = cov.ndim == 2
    if single:
        cov = cov[None]
    n, d, _ = cov.shape
    L = np.empty((n, d * (d + 1) // 2))
    _lib.check(_lib.load().rome_cholesky_lower(d, n, _p(cov), _p(L)))
    return L[0] if single else L


def make_opts(N=100, solver=_lib.SOLVER_NEWTON, max_iters=None, inflate_cycles=None, tol=None, inflation=None,
              seed=None, stream_offset=None, layout=None, spread_nh=None, nullhypo=None, presampled=None):
    """presampled=1 (NOISE_MEASUREMENTS): the `noise` argument of the conv_* calls holds the measurement samples themselves
    (any SamplableBelief sampled by the caller) instead of standard normals."""
    return _lib.default_opts(solver, n_particles=N, max_iters=max_iters, inflate_cycles=inflate_cycles, tol=tol,
                             inflation=inflation, seed=seed, stream_offset=stream_offset, layout=layout,
                             spread_nh=spread_nh, nullhypo=nullhypo, presampled=presampled)


def _blocks(a, C_, N, d, layout, points_ok=True):
    if layout == _lib.LAYOUT_AOS_POINTS and points_ok:
        d = {3: 6, 6: 12}.get(d, d)
    shape = (C_, d, N) if layout == _lib.LAYOUT_SOA else (C_, N, d)
    return _d(a, shape)


def points_to_coords(dim, pts, ctx=None):
    ctx = ctx or default_context()
    pts = np.atleast_2d(_d(pts)); n = pts.shape[0]
    out = np.empty((n, dim))
    _lib.check(_lib.load().rome_points_to_coords(ctx.handle, dim, n, _p(pts), _p(out)), ctx.handle)
    return out


def coords_to_points(dim, coords, ctx=None):
    ctx = ctx or default_context()
    coords = np.atleast_2d(_d(coords)); n = coords.shape[0]
    out = np.empty((n, {3: 6, 6: 12}.get(dim, dim)))
    _lib.check(_lib.load().rome_coords_to_points(ctx.handle, dim, n, _p(coords), _p(out)), ctx.handle)
    return out


# ------------------------------------------------------------------ host-pointer convolutions
def _override(opts, layout=None, nullhypo=None):
    """opts, or a copy with the layout / nullhypo a wrapper was given"""
    if layout is None and nullhypo is None:
        return opts
    o = _lib.Opts.from_buffer_copy(opts)
    if layout is not None:
        o.layout = int(layout)
    if nullhypo is not None:
        o.nullhypo = float(nullhypo)
    return o


_ABSENT = object()   # the entry point has no such argument


def _conv(entry, dims, opts, mu, prms, fixed, target, noise, ctx, layout=None, nullhypo=None, dirs=_ABSENT, direction=_ABSENT,
          want_status=None, alt=None, hypo_w=None):
    """THE call of a host-pointer convolution entry `entry`.  dims = (dz, d1, d2), the dimensions of the measurement and of the factor's
    first and second variable: direction 0 fixes the first and solves the second, another one swaps them.  prms: the noise parameters as
    (array, shape of one row).  fixed None: the entry takes no fixed blocks.  The direction is a column `dirs` (None: all 0; one value is
    repeated for every row; an array must have one value per row) or one scalar `direction`; want_status None: the entry has no status
    array; alt / hypo_w: a multihypo entry (the blocks of the other candidate for the second variable)."""
    ctx = ctx or default_context()
    opts = _override(opts, layout, nullhypo)
    dz, d1, d2 = dims
    df, dt = (d1, d2) if direction is _ABSENT or direction == 0 else (d2, d1)
    mu = np.atleast_2d(_d(mu)) if dz > 1 else np.atleast_1d(_d(mu)).reshape(-1, 1)
    C_, N = mu.shape[0], opts.n_particles
    mu = _d(mu, (C_, dz))
    prms = [_d(a if shape else np.atleast_1d(_d(a)).ravel(), (C_,) + shape) for a, shape in prms]
    args = [] if direction is _ABSENT else [int(direction)]
    if dirs is not _ABSENT:
        dirs = None if dirs is None else np.ascontiguousarray(np.broadcast_to(np.asarray(dirs, dtype=np.int32), (C_,)))
        args.append(_pi(dirs))
    args += [_p(mu)] + [_p(a) for a in prms]
    if fixed is not None:
        fixed = _blocks(fixed, C_, N, df, opts.layout)
        args.append(_p(fixed))
    out = _blocks(target, C_, N, dt, opts.layout).copy()
    if alt is not None:
        alt, hypo_w = _blocks(alt, C_, N, d2, opts.layout), _d(hypo_w, (C_,))
        args += [_p(alt), _p(hypo_w)]
    noise = None if noise is None else _blocks(noise, C_, N, dz, opts.layout, points_ok=False)
    args += [_p(noise), _p(out)]
    st = np.zeros((C_, N), dtype=np.int32) if want_status else None
    if want_status is not None:
        args.append(_pi(st))
    _lib.check(getattr(_lib.load(), entry)(ctx.handle, C.byref(opts), C_, *args), ctx.handle)
    return (out, st) if want_status else out


def conv_pose2pose2(opts, mu, cov, fixed, target, dirs=None, noise=None, want_status=False, ctx=None, alt=None, hypo_w=None):
    """alt / hypo_w: multihypo over two candidates for the factor's second pose (blocks of the other candidate, P(primary));
    `dirs` must then be one direction (0 or 1) for the whole call."""
    if alt is None:
        return _conv("rome_conv_pose2pose2", (3, 3, 3), opts, mu, [(cov, (3, 3))], fixed, target, noise, ctx, dirs=dirs, want_status=want_status)
    d = np.unique(np.asarray(0 if dirs is None else dirs, dtype=np.int32))
    if d.size != 1 or int(d[0]) not in (0, 1):
        raise ValueError("conv_pose2pose2 with multihypo: one direction (0 or 1) per call")
    return _conv("rome_conv_pose2pose2_mh", (3, 3, 3), opts, mu, [(cov, (3, 3))], fixed, target, noise, ctx, direction=int(d[0]),
                 want_status=want_status, alt=alt, hypo_w=hypo_w)


def conv_pose2point2br(opts, direction, mu, sigma, fixed, target, noise=None, want_status=False, ctx=None,
                       alt=None, hypo_w=None):
    """alt / hypo_w: multihypo over two landmark candidates (blocks of the other landmark, P(primary))."""
    return _conv("rome_conv_pose2point2br" if alt is None else "rome_conv_pose2point2br_mh", (2, 3, 2), opts, mu, [(sigma, (2,))], fixed, target,
                 noise, ctx, direction=direction, want_status=want_status, alt=alt, hypo_w=hypo_w)


def conv_point2point2range(opts, mu, sigma, fixed, target, dirs=None, noise=None, want_status=False, ctx=None, layout=None):
    """C Point2Point2Range convolutions (Range2D.jl:8-17): mu / sigma (C,) range means and sigmas (sigma < 0: Uniform(mu ± |sigma|)),
    dirs (C,) or None (0: solve lm from xi, 1: solve xi from lm), fixed / target C Point2 blocks, noise C blocks of one standard
    normal per particle (or the range samples themselves under presampled=NOISE_MEASUREMENTS)."""
    return _conv("rome_conv_point2point2range", (1, 2, 2), opts, mu, [(sigma, ())], fixed, target, noise, ctx, layout, dirs=dirs,
                 want_status=want_status)


def conv_pose2point2range(opts, direction, mu, sigma, fixed, target, noise=None, want_status=False, ctx=None, layout=None):
    """C Pose2Point2Range convolutions (Range2D.jl:40-54), one direction per call: 0 solves the landmarks from the fixed poses, 1 the
    poses from the fixed landmarks -- (x, y) only, every particle's heading is returned unchanged."""
    return _conv("rome_conv_pose2point2range", (1, 3, 2), opts, mu, [(sigma, ())], fixed, target, noise, ctx, layout, direction=direction,
                 want_status=want_status)


def conv_pose2point2bearing(opts, direction, mu, sigma, fixed, target, noise=None, want_status=False, ctx=None, layout=None, nullhypo=None):
    """C Pose2Point2Bearing convolutions (Bearing2D.jl:10-32), one direction per call: 0 solves the landmarks from the fixed poses
    (each start point keeps its distance and is turned onto the ray), 1 the poses from the fixed landmarks (each start pose keeps its
    translation and is turned to the measured bearing).  mu / sigma (C,): the bearing belief (sigma < 0: Uniform(mu ± |sigma|));
    noise: C blocks of one standard normal per particle (or the bearings themselves under presampled=NOISE_MEASUREMENTS);
    nullhypo: the fraction of particles the factor does not apply to (opts.nullhypo when None)."""
    if direction not in (0, 1):
        raise ValueError("direction must be 0 (solve the landmark) or 1 (solve the pose)")
    return _conv("rome_conv_pose2point2bearing", (1, 3, 2), opts, mu, [(sigma, ())], fixed, target, noise, ctx, layout, nullhypo,
                 direction=direction, want_status=want_status)


def conv_pose3pose3(opts, mu, cov, fixed, target, dirs=None, noise=None, want_status=False, ctx=None):
    return _conv("rome_conv_pose3pose3", (6, 6, 6), opts, mu, [(cov, (6, 6))], fixed, target, noise, ctx, dirs=dirs, want_status=want_status)


def conv_pose3pose3xyyaw(opts, mu, cov, fixed, target, dirs=None, noise=None, want_status=False, ctx=None, layout=None, nullhypo=None):
    """C Pose3Pose3XYYaw convolutions (PartialPose3.jl:101-136): mu (C, 3), cov (C, 3, 3), dirs (C,) or None (0: solve q from p, 1: solve p
    from q), fixed / target C Pose3 blocks, noise C blocks of three standard normals per particle (or the (x, y, θ) samples themselves under
    presampled=NOISE_MEASUREMENTS).  Solves the target's (x, y, ω_z); every particle's z, ω_x, ω_y is returned unchanged (bit for bit
    in the coordinate layouts).  nullhypo: the fraction of particles the factor does not apply to (opts.nullhypo when None)."""
    return _conv("rome_conv_pose3pose3xyyaw", (3, 6, 6), opts, mu, [(cov, (3, 3))], fixed, target, noise, ctx, layout, nullhypo, dirs=dirs,
                 want_status=want_status)


def conv_pose3pose3rotation(opts, mu, cov, fixed, target, dirs=None, noise=None, want_status=False, ctx=None, layout=None, nullhypo=None):
    """C Pose3Pose3Rotation convolutions (PartialPose3.jl:204-227): mu (C, 3), cov (C, 3, 3), dirs (C,) or None (0: solve q from p, 1: solve p
    from q), fixed / target C Pose3 blocks, noise C blocks of three standard normals per particle (or the rotation-vector samples themselves
    under presampled=NOISE_MEASUREMENTS).  Solves the target's (ω_x, ω_y, ω_z); every particle's translation is returned unchanged (bit
    for bit in the coordinate layouts).  nullhypo: the fraction of particles the factor does not apply to (opts.nullhypo when None)."""
    return _conv("rome_conv_pose3pose3rotation", (3, 6, 6), opts, mu, [(cov, (3, 3))], fixed, target, noise, ctx, layout, nullhypo, dirs=dirs,
                 want_status=want_status)


def conv_priorpose3zrp(opts, mu, sigma_z, cov_rp, target, noise=None, ctx=None, layout=None, nullhypo=None):
    """C PriorPose3ZRP rows (PartialPose3.jl:12-46): mu (C, 3) = (μ_z, μ_roll, μ_pitch), sigma_z (C,), cov_rp (C, 2, 2), target C Pose3
    blocks -> the same blocks with coordinates 3, 4, 5 (z, ω_x, ω_y) replaced by the samples; x, y, ω_z unchanged (bit for bit in the
    coordinate layouts).  noise: C blocks of three standard normals per particle (or the three sample coordinates themselves under
    presampled=NOISE_MEASUREMENTS)."""
    return _conv("rome_conv_priorpose3zrp", (3, 6, 6), opts, mu, [(sigma_z, ()), (cov_rp, (2, 2))], None, target, noise, ctx, layout, nullhypo)


# ------------------------------------------------------------------ deconvolution
# factor class -> (ROME_DECONV_*, dz, dimension of the first / second variable, shape of one row of the noise parameters): the relative
# factors the library convolves.  Looked up along the factor's classes; anything else is refused by name (deconv_family).
_DECONV = {
    Pose2Pose2: (_lib.DECONV_POSE2POSE2, 3, 3, 3, (3, 3)),
    Pose2Point2BearingRange: (_lib.DECONV_POSE2POINT2BR, 2, 3, 2, (2,)),
    Pose2Point2Bearing: (_lib.DECONV_POSE2POINT2BEARING, 1, 3, 2, ()),
    Point2Point2Range: (_lib.DECONV_POINT2POINT2RANGE, 1, 2, 2, ()),
    Pose2Point2Range: (_lib.DECONV_POSE2POINT2RANGE, 1, 3, 2, ()),
    Pose3Pose3: (_lib.DECONV_POSE3POSE3, 6, 6, 6, (6, 6)),
    Pose3Pose3XYYaw: (_lib.DECONV_POSE3POSE3XYYAW, 3, 6, 6, (3, 3)),
    Pose3Pose3Rotation: (_lib.DECONV_POSE3POSE3ROTATION, 3, 6, 6, (3, 3)),
}


def deconv_family(family):
    """(ROME_DECONV_*, dz, da, db, noise-parameter row shape) of a factor class, a factor, or a class name; TypeError, by name, for
    what a deconvolution is not defined on here: priors (their deconvolution is the belief itself) and Point2Point2 (host side only)."""
    cls = family if isinstance(family, type) else type(family)
    if isinstance(family, str):
        cls = next((c for c in _DECONV if c.__name__ == family), None)
        if cls is None:
            raise TypeError("deconv: no deconvolution for factor type %s (priors: the belief itself; Point2Point2: host side only)" % family)
    for c in cls.__mro__:
        if c in _DECONV:
            return _DECONV[c]
    raise TypeError("deconv: no deconvolution for factor type %s (priors: the belief itself; Point2Point2: host side only)" % cls.__name__)


def deconv(family, opts, mu, cov, a, b, noise=None, want=("pred", "meas"), ctx=None):
    """C deconvolutions of one factor family (rome_deconv; ⚠IIF approxDeconv restated, include/rome_mi355.h): row c pairs particle i of
    block c of `a` (the factor's first variable) with particle i of block c of `b` (the second).  family: a factor class, a factor or
    a class name; mu (C, dz) and cov as the family's conv_* wrapper takes them (covariances (C, dz, dz), or sigmas); a / b: C blocks
    in opts.layout; noise: C blocks of standard normals, or of the samples themselves under presampled=NOISE_MEASUREMENTS.
    -> (pred, meas), each C blocks of dz coordinates ((C, dz, N) in LAYOUT_SOA, else (C, N, dz)), None for an output not in `want`:
    pred = the measurement each pair predicts, meas = the sample the convolution of row c (stream opts.stream_offset + c) draws."""
    fam, dz, da, db, shape = deconv_family(family)
    want = tuple(want)
    if not want or any(w not in ("pred", "meas") for w in want):
        raise ValueError("deconv: want must name 'pred', 'meas' or both, got %r" % (want,))
    ctx = ctx or default_context()
    mu = np.atleast_2d(_d(mu)) if dz > 1 else np.atleast_1d(_d(mu)).reshape(-1, 1)
    C_, N = mu.shape[0], opts.n_particles
    mu = _d(mu, (C_, dz))
    cov = _d(cov if shape else np.atleast_1d(_d(cov)).ravel(), (C_,) + shape)
    a, b = _blocks(a, C_, N, da, opts.layout), _blocks(b, C_, N, db, opts.layout)
    noise = None if noise is None else _blocks(noise, C_, N, dz, opts.layout, points_ok=False)
    oshape = (C_, dz, N) if opts.layout == _lib.LAYOUT_SOA else (C_, N, dz)
    pred = np.empty(oshape) if "pred" in want else None
    meas = np.empty(oshape) if "meas" in want else None
    _lib.check(_lib.load().rome_deconv(ctx.handle, C.byref(opts), fam, C_, _p(mu), _p(cov), _p(a), _p(b), _p(noise), _p(pred), _p(meas)), ctx.handle)
    return pred, meas


def _sample_prior(fn, d, opts, mu, cov, noise, ctx):
    ctx = ctx or default_context()
    mu = np.atleast_2d(_d(mu)); C_ = mu.shape[0]; N = opts.n_particles
    cov = _d(cov, (C_, d, d))
    noise = None if noise is None else _blocks(noise, C_, N, d, opts.layout, points_ok=False)
    pl = {2: 2, 3: 6, 6: 12}[d] if opts.layout == _lib.LAYOUT_AOS_POINTS else d
    out = np.empty((C_, d, N) if opts.layout == _lib.LAYOUT_SOA else (C_, N, pl))
    _lib.check(fn(ctx.handle, C.byref(opts), C_, _p(mu), _p(cov), _p(noise), _p(out)), ctx.handle)
    return out


def sample_priorpose2(opts, mu, cov, noise=None, ctx=None):
    return _sample_prior(_lib.load().rome_sample_priorpose2, 3, opts, mu, cov, noise, ctx)


def sample_priorpose3(opts, mu, cov, noise=None, ctx=None):
    return _sample_prior(_lib.load().rome_sample_priorpose3, 6, opts, mu, cov, noise, ctx)


def sample_priorpoint2(opts, mu, cov, noise=None, ctx=None):
    """N samples of `PriorPoint2(MvNormal(mu, cov))` (src/factors/Point2D.jl:8-18): the proposal a landmark prior contributes"""
    return _sample_prior(_lib.load().rome_sample_priorpoint2, 2, opts, mu, cov, noise, ctx)
