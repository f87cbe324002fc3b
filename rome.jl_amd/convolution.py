"""`approxConvBelief` / `approxConv` mirror (IIF API as used by the reference:
test/testBasicPose2Conv.jl:25, test/TestPoseAndPoint2Constraints.jl:36,97)."""
import numpy as np

from . import _lib, api
from .factors import Pose2Pose2, PriorPose2, Pose2Point2BearingRange, Pose3Pose3, PriorPose3, PriorPoint2, Point2Point2Range, Pose2Point2Range, Pose2Point2Bearing, Pose3Pose3XYYaw, PriorPose3ZRP, Pose3Pose3Rotation


def approxConv(fg, flabel, target, solver=_lib.SOLVER_NEWTON, seed=None, ctx=None, **optkw):
    """N proposal points (dim, N) for variable `target` through factor `flabel`, convolving the
    factor's measurement model with the current belief of its other variable."""
    _, labels, f = fg.getFactor(flabel)
    if target not in labels:
        raise KeyError("%s is not connected to factor %s" % (target, flabel))
    opts = api.make_opts(N=fg.N, solver=solver, seed=seed, **optkw)
    if isinstance(f, PriorPose2):
        return api.sample_priorpose2(opts, [f.Z.mu], [f.Z.cov], ctx=ctx)[0]
    if isinstance(f, PriorPose3):
        return api.sample_priorpose3(opts, [f.Z.mu], [f.Z.cov], ctx=ctx)[0]
    if isinstance(f, PriorPoint2):
        return api.sample_priorpoint2(opts, [f.Z.mu], [f.Z.cov], ctx=ctx)[0]
    if isinstance(f, PriorPose3ZRP):   # a partial prior: the target's own belief with z, ω_x, ω_y replaced (zeros before it has one)
        u0 = fg.getVal(target)[None] if fg.isInitialized(target) else np.zeros((1, 6, fg.N))
        return api.conv_priorpose3zrp(opts, [[f.z.mu, f.rp.mu[0], f.rp.mu[1]]], [f.z.sigma], [f.rp.cov], u0, ctx=ctx)[0]
    mh = fg.multihypo.get(flabel)
    if mh is not None and isinstance(f, Pose2Pose2):   # Pose2Pose2 over [a, b1, b2]
        a, b1, b2 = labels
        opts.layout = _lib.LAYOUT_SOA
        z3 = lambda l: fg.getVal(l)[None] if fg.isInitialized(l) else np.zeros((1, 3, fg.N))
        if target == a:
            return api.conv_pose2pose2(opts, [f.Z.mu], [f.Z.cov], z3(b1), z3(a), dirs=[1], alt=z3(b2), hypo_w=[mh[0]], ctx=ctx)[0]
        prim, alt, w = (b1, b2, mh[0]) if target == b1 else (b2, b1, mh[1])
        return api.conv_pose2pose2(opts, [f.Z.mu], [f.Z.cov], fg.getVal(a)[None], z3(prim), dirs=[0], alt=z3(alt), hypo_w=[w], ctx=ctx)[0]
    if mh is not None:   # Pose2Point2BearingRange over [pose, l1, l2]
        pose, l1, l2 = labels
        opts.layout = _lib.LAYOUT_SOA
        z2 = lambda l: fg.getVal(l)[None] if fg.isInitialized(l) else np.zeros((1, 2, fg.N))
        args = ([[f.bearing.mu, f.range.mu]], [[f.bearing.sigma, f.range.sigma]])
        if target == pose:
            u0 = fg.getVal(pose)[None] if fg.isInitialized(pose) else np.zeros((1, 3, fg.N))
            return api.conv_pose2point2br(opts, 1, *args, z2(l1), u0, alt=z2(l2), hypo_w=[mh[0]], ctx=ctx)[0]
        prim, alt, w = (l1, l2, mh[0]) if target == l1 else (l2, l1, mh[1])
        return api.conv_pose2point2br(opts, 0, *args, fg.getVal(pose)[None], z2(prim), alt=z2(alt), hypo_w=[w], ctx=ctx)[0]
    direction = 0 if labels[1] == target else 1
    other = labels[0] if direction == 0 else labels[1]
    if not fg.isInitialized(other):
        raise ValueError("approxConv: variable %s has no belief yet" % other)
    fixed = fg.getVal(other)[None]
    tt = fg.variables[target]
    u0 = fg.getVal(target)[None] if fg.isInitialized(target) else np.zeros((1, tt.dim, fg.N))
    if isinstance(f, Pose2Pose2):
        return api.conv_pose2pose2(opts, [f.Z.mu], [f.Z.cov], fixed, u0, dirs=[direction], ctx=ctx)[0]
    if isinstance(f, Pose3Pose3):
        return api.conv_pose3pose3(opts, [f.Z.mu], [f.Z.cov], fixed, u0, dirs=[direction], ctx=ctx)[0]
    if isinstance(f, Pose3Pose3XYYaw):
        return api.conv_pose3pose3xyyaw(opts, [f.Z.mu], [f.Z.cov], fixed, u0, dirs=[direction], ctx=ctx)[0]
    if isinstance(f, Pose3Pose3Rotation):
        return api.conv_pose3pose3rotation(opts, [f.Z.mu], [f.Z.cov], fixed, u0, dirs=[direction], ctx=ctx)[0]
    if isinstance(f, Pose2Point2BearingRange):
        return api.conv_pose2point2br(opts, direction, [[f.bearing.mu, f.range.mu]], [[f.bearing.sigma, f.range.sigma]],
                                      fixed, u0, ctx=ctx)[0]
    if isinstance(f, Point2Point2Range):
        return api.conv_point2point2range(opts, [f.Z.mu], [f.Z.sigma], fixed, u0, dirs=[direction], ctx=ctx)[0]
    if isinstance(f, Pose2Point2Range):
        return api.conv_pose2point2range(opts, direction, [f.Z.mu], [f.Z.sigma], fixed, u0, ctx=ctx)[0]
    if isinstance(f, Pose2Point2Bearing):
        return api.conv_pose2point2bearing(opts, direction, [f.Z.mu], [f.Z.sigma], fixed, u0, ctx=ctx)[0]
    raise TypeError("unsupported factor type %s" % type(f).__name__)


approxConvBelief = approxConv


def _deconv_rows(fg, flabels, who):
    """(factor, mu row, noise-parameter row, first / second variable's label) of each factor label; refusals by name, before any device
    call: priors and Point2Point2 (api.deconv_family), multihypo factors, variables without a belief"""
    rows = []
    for flabel in flabels:
        _, labels, f = fg.getFactor(flabel)
        api.deconv_family(f)
        if fg.multihypo.get(flabel) is not None:
            raise TypeError("%s: factor %s carries multihypo; a deconvolution pairs one first with one second variable" % (who, flabel))
        for l in labels[:2]:
            if not fg.isInitialized(l):
                raise ValueError("%s: variable %s has no belief yet" % (who, l))
        if isinstance(f, Pose2Point2BearingRange):
            mu, prm = [f.bearing.mu, f.range.mu], [f.bearing.sigma, f.range.sigma]
        elif isinstance(f, (Point2Point2Range, Pose2Point2Range, Pose2Point2Bearing)):
            mu, prm = f.Z.mu, f.Z.sigma
        else:
            mu, prm = f.Z.mu, f.Z.cov
        rows.append((f, mu, prm, labels[0], labels[1]))
    return rows


def approxDeconv(fg, flabel, seed=None, ctx=None, **optkw):
    """⚠IIF `approxDeconv(fg, flabel)` as the reference calls it (test/testBasicPose2Conv.jl:51; restated from that call site, not checked
    against IIF): -> (pred, meas), each (dz, N) measurement coordinates.  pred[:, i] is the measurement at which the factor's residual
    vanishes on particle i of its first and particle i of its second variable; meas holds N samples of the measurement the factor
    carries, drawn as approxConv draws them.  nullhypo is ignored (a deconvolution has no null branch).  TypeError, by name: priors,
    Point2Point2, multihypo factors."""
    (f, mu, prm, a, b), = _deconv_rows(fg, [flabel], "approxDeconv")
    opts = api.make_opts(N=fg.N, seed=seed, **optkw)
    opts.layout = _lib.LAYOUT_SOA
    pred, meas = api.deconv(f, opts, [mu], [prm], fg.getVal(a)[None], fg.getVal(b)[None], ctx=ctx)
    return pred[0], meas[0]


_MMD_FAMILIES = (Pose2Pose2, Pose3Pose3XYYaw, Pose3Pose3)   # measurement manifolds rome_mmd serves: SE(2) (dim 3), SE(3) (dim 6)


def factorMMD(fg, labels=None, bw=0.001, seed=None, ctx=None, **optkw):
    """{flabel: mmd(pred, meas)} of approxDeconv for the factors `labels`: how well each factor's measurement model agrees with the
    current beliefs of its variables (the reference accepts a convolution at < 0.001, test/testBasicPose2Conv.jl:56); a factor at odds
    with the solve stands out.  labels None: every Pose2Pose2, Pose3Pose3XYYaw and Pose3Pose3 factor of the graph without multihypo.
    A named factor of another family raises TypeError: its measurement manifold (R, the circle, circle x R, SO(3)) is not one `mmd`
    serves.  One deconv and one mmd call per family; factor k of a family draws Philox stream stream_offset + k."""
    if labels is None:
        labels = [fl for fl, _, f in fg.factors if isinstance(f, _MMD_FAMILIES) and fg.multihypo.get(fl) is None]
    labels = list(labels)
    for fl in labels:   # (the family first: a refusal does not depend on what has a belief)
        f = fg.getFactor(fl)[2]
        api.deconv_family(f)
        if not isinstance(f, _MMD_FAMILIES):
            raise TypeError("factorMMD: the measurement manifold of %s (factor %s) is not one mmd serves" % (type(f).__name__, fl))
    rows = _deconv_rows(fg, labels, "factorMMD")
    opts = api.make_opts(N=fg.N, seed=seed, **optkw)
    opts.layout = _lib.LAYOUT_SOA
    res = {}
    for cls in _MMD_FAMILIES:
        sel = [(fl, r) for fl, r in zip(labels, rows) if next(c for c in type(r[0]).__mro__ if c in _MMD_FAMILIES) is cls]
        if not sel:
            continue
        pred, meas = api.deconv(cls, opts, [r[1] for _, r in sel], [r[2] for _, r in sel], np.stack([fg.getVal(r[3]) for _, r in sel]),
                                np.stack([fg.getVal(r[4]) for _, r in sel]), ctx=ctx)
        res.update(zip([fl for fl, _ in sel], api.mmd(pred, meas, bw=bw, ctx=ctx).tolist()))
    return {fl: res[fl] for fl in labels}
