"""Bearing-only factor on the device: Pose2Point2Bearing (RoME src/factors/Bearing2D.jl).

The residual entries against the reference's KATs and the oracle; the convolutions against bearing_ref (a per-row restatement over the
oracle's primitives) for both directions, every solver, particle count (PPL 1/2/4/8 and k_conv_big) and noise source; layouts, the
_dev twin and refusals; one whole-graph sweep against bearing_ref and against the same graph without bearing-only factors; the
parametric row (rome_linearize kind 6) and three solves of test/testBearing2D.jl; the example."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import bearing_ref
import oracle as ro

pytestmark = pytest.mark.gpu
R = None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "bearing2d_kats.json")))


@pytest.fixture(scope="module", autouse=True)
def _pkg():
    global R
    import rome_jl_amd
    R = rome_jl_amd
    R.default_context()
    yield


SEED, SOFF, CYC, INFL = 23, 7, 3, 5.0
wrap = lambda a: np.arctan2(np.sin(a), np.cos(a))


def _opts(N, solver, cycles=CYC, inflation=INFL, **kw):
    o = R.make_opts(N=N, solver=solver, seed=SEED, stream_offset=SOFF, inflate_cycles=cycles, inflation=inflation, **kw)
    oo = ro.make_opts(N=N, solver=0, seed=SEED, stream_offset=SOFF, inflate_cycles=cycles, inflation=inflation)
    return o, oo


def _inputs(kind, C_, N, seed):
    """kind: "pb0" (pose fixed -> landmark), "pb1" (landmark fixed -> pose)"""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-3, 3, C_); sigma = rng.uniform(0.01, 0.2, C_)
    df, dt = {"pb0": (3, 2), "pb1": (2, 3)}[kind]
    centre = rng.uniform(-40, 40, (C_, 2, 1))
    fixed = np.zeros((C_, df, N)); fixed[:, :2] = centre + 0.5 * rng.standard_normal((C_, 2, N))
    target = np.zeros((C_, dt, N)); target[:, :2] = centre + rng.uniform(-25, 25, (C_, 2, 1)) + 2.0 * rng.standard_normal((C_, 2, N))
    if df == 3:
        fixed[:, 2] = rng.uniform(-3, 3, (C_, 1)) + 0.1 * rng.standard_normal((C_, N))
    if dt == 3:
        target[:, 2] = rng.uniform(-3, 3, (C_, 1)) + 0.1 * rng.standard_normal((C_, N))
    noise = rng.standard_normal((C_, 1, N))
    return mu, sigma, fixed, target, noise


def _run(kind, o, mu, sigma, fixed, target, noise=None, want_status=True, layout=None, nullhypo=None):
    return R.conv_pose2point2bearing(o, int(kind[-1]), mu, sigma, fixed, target, noise=noise, want_status=want_status, layout=layout,
                                     nullhypo=nullhypo)


def _delta(out, ref):
    d = out - ref
    if d.shape[1] == 3:
        d[:, 2] = wrap(d[:, 2])
    return np.abs(d)


def _own_residual(kind, b, fixed, out):
    """|r| of every output particle against its own bearing sample b [C][N], from the oracle's residual"""
    C_ = out.shape[0]
    r = []
    for c in range(C_):
        pose, lm = (fixed[c].T, out[c].T) if kind == "pb0" else (out[c].T, fixed[c].T)
        r.append(bearing_ref.residual(b[c], pose, lm))
    return np.abs(np.array(r))


# ------------------------------------------------------------------ 1. residual entries
def test_residual_reference_kats():
    g = KATS["grid"]
    poses = np.array(g["poses"])
    n = len(poses)
    r = R.residual_pose2point2bearing(np.full(n, g["b"]), poses, np.tile(g["q"], (n, 1)))
    d = np.array([ro.sym_rem(x) for x in r - np.array(g["expected"])])
    assert n == 11 and np.abs(d).max() <= g["atol"]
    for k in ("sign", "pm_pi"):
        c = KATS[k]
        r = R.residual_pose2point2bearing([c["b"]], [c["pose"]], [c["l"]])[0]
        assert abs(r - c["expected"]) <= c["atol"], (k, r)
    f = R.Pose2Point2Bearing(R.Normal(math.pi / 4, 0.05))
    m = [0.0, math.pi / 4, -math.pi / 4, 0.0]        # hat(SO2, [π/4]), column-major
    r = R.calcFactorResidualTemporary(f, (R.Pose2, R.Point2), m, (R.getPoint(R.Pose2, [1.0, 2.0, 0.0]), [5.0, 5.0]))
    assert abs(r - g["expected"][10]) <= g["atol"]


def test_residual_vs_oracle_and_pt_twin():
    rng = np.random.default_rng(4)
    n = 1000
    z = rng.uniform(-4, 4, n); p = np.column_stack([rng.uniform(-30, 30, (n, 2)), rng.uniform(-3.2, 3.2, n)]); lm = rng.uniform(-30, 30, (n, 2))
    r = R.residual_pose2point2bearing(z, p, lm)
    ref = ro.residual_pose2point2br(np.column_stack([z, np.zeros(n)]), p, lm)[:, 0]
    d = np.abs(r - ref)
    print("residual entry vs oracle: max |Δ| = %.3e" % d.max())
    assert d.max() <= 1e-12
    rp = R.residual_pose2point2bearing_pt(z, R.getPoint(R.Pose2, p), lm)
    assert np.abs(rp - r).max() <= 1e-12
    both = R.residual_pose2point2br(np.column_stack([z, np.zeros(n)]), p, lm)[:, 0]
    assert np.array_equal(both, r)                  # the bearing row of the bearing-range entry, bit for bit


# ------------------------------------------------------------------ 2. convolution parity against bearing_ref
@pytest.mark.parametrize("kind", ["pb0", "pb1"])
@pytest.mark.parametrize("solver", [0, 1, 3])
@pytest.mark.parametrize("N", [50, 100, 256, 400, 700])
@pytest.mark.parametrize("given_noise", [False, True])
def test_conv_vs_bearing_ref(kind, solver, N, given_noise):
    C_ = 3
    mu, sigma, fixed, target, noise = _inputs(kind, C_, N, 100 + N + solver)
    sigma[0] = -sigma[0]                    # one Uniform row
    o, oo = _opts(N, solver)
    nz = noise if given_noise else None
    out, st = _run(kind, o, mu, sigma, fixed, target, noise=nz)
    ref, rst = bearing_ref.conv(oo, mu, sigma, fixed, target, solver, noise=nz)
    d = _delta(out, ref)
    print("%s solver %d N %d: max |Δ| = %.3e" % (kind, solver, N, d.max()))
    assert d.max() <= 1e-9, d.max()
    if solver != 0:
        assert np.array_equal(st, rst)
    else:
        assert not st.any()
    # independent of the restatement: every particle satisfies its own sampled bearing
    b = np.array([[bearing_ref.measurement(mu[c], sigma[c], nz[c, 0, i] if given_noise else ro.rng_normals(SEED, SOFF + c, i, 1)[0])
                   for i in range(N)] for c in range(C_)])
    assert _own_residual(kind, b, fixed, out).max() <= 1e-9


@pytest.mark.parametrize("solver", [0, 1, 3])
def test_pose_translation_is_the_jittered_start(solver):
    """pb1 returns (x, y) of the jittered start bit for bit.  After ONE cycle two runs that differ only in mu return identical (x, y)
    (from the second cycle on, the compose-form jitter is rotated by the heading the first solve set, which depends on mu); with no
    inflation the start translations themselves come back after three cycles."""
    N = 100
    mu, sigma, fixed, target, _ = _inputs("pb1", 3, N, 12)
    o1, _ = _opts(N, solver, cycles=1)
    a = _run("pb1", o1, mu, sigma, fixed, target, want_status=False)
    b = _run("pb1", o1, mu + 1.3, sigma, fixed, target, want_status=False)
    assert np.array_equal(a[:, :2], b[:, :2]) and not np.array_equal(a[:, 2], b[:, 2])
    assert not np.array_equal(a[:, :2], target[:, :2])
    o0, _ = _opts(N, solver, cycles=3, inflation=0.0)
    c = _run("pb1", o0, mu, sigma, fixed, target, want_status=False)
    assert np.array_equal(c[:, :2], target[:, :2])


# ------------------------------------------------------------------ 3. the in-kernel RNG
def test_in_kernel_rng_is_the_oracle_d1_rule():
    """zero inflation, one cycle: the bearing of the output landmark about the fixed pose is μ + σ ξ with ξ = ro.rng_normals(..., 1)"""
    N = 100
    mu, sigma, fixed, target, _ = _inputs("pb0", 2, N, 9)
    o = R.make_opts(N=N, solver=0, seed=SEED, stream_offset=SOFF, inflate_cycles=1, inflation=0.0)
    out = R.conv_pose2point2bearing(o, 0, mu, sigma, fixed, target)
    world = np.arctan2(out[:, 1] - fixed[:, 1], out[:, 0] - fixed[:, 0])
    xi = np.array([[ro.rng_normals(SEED, SOFF + c, i, 1)[0] for i in range(N)] for c in range(2)])
    d = wrap(world - fixed[:, 2] - (mu[:, None] + sigma[:, None] * xi))
    assert np.abs(d).max() < 1e-11


# ------------------------------------------------------------------ 4. Nelder-Mead
@pytest.mark.parametrize("kind", ["pb0", "pb1"])
def test_nelder_mead_vs_bearing_ref(kind):
    """pb0: a 1-D valley, the bar of the range rows (median |Δ| < 1e-9, >= 95 % within 1e-6).  pb1 minimises over a 2-D valley in
    three coordinates; the share within 1e-6 measured on these inputs on an MI355X is 0.9650 (pb0: 1.0000;
    profiles/bearing_factors_trace.md), so the same 0.95 is asserted.  The 99th percentile of |r| stays below 1e-3 in both."""
    C_, N = 4, 100
    mu, sigma, fixed, target, noise = _inputs(kind, C_, N, 31)
    o, oo = _opts(N, 2)
    out = _run(kind, o, mu, sigma, fixed, target, noise=noise, want_status=False)
    ref, _ = bearing_ref.conv(oo, mu, sigma, fixed, target, 2, noise=noise)
    d = _delta(out, ref).max(axis=1)
    share = np.mean(d < 1e-6)
    b = mu[:, None] + sigma[:, None] * noise[:, 0]
    r = _own_residual(kind, b, fixed, out)
    print("nelder-mead %s: median |Δ| = %.3e, share within 1e-6 = %.4f, max |Δ| = %.3e, p99 |r| = %.3e"
          % (kind, np.median(d), share, d.max(), np.percentile(r, 99)))
    assert np.median(d) < 1e-9
    assert share >= 0.95
    assert np.percentile(r, 99) < 1e-3


# ------------------------------------------------------------------ 5. edge rows, nullhypo, layouts, _dev twin, refusals
def test_edge_rows_start_on_the_anchor():
    N = 64
    rng = np.random.default_rng(1)
    pose = np.zeros((2, 3, N)); pose[:, 0] = 5.0; pose[:, 1] = -2.0; pose[:, 2] = rng.uniform(-3, 3, (2, N))
    pt = np.array(pose[:, :2])                       # every landmark start ON the pose's translation
    meas = rng.uniform(-4, 4, (2, 1, N))
    for solver in (0, 1, 3):
        o = R.make_opts(N=N, solver=solver, inflate_cycles=1, inflation=0.0, presampled=1)
        out, st = R.conv_pose2point2bearing(o, 0, np.zeros(2), np.ones(2), pose, pt, noise=meas, want_status=True)
        assert np.array_equal(out, pt)               # no direction can be given a length: unchanged
        if solver != 0:
            assert (st == (np.abs(wrap(meas[:, 0])) > 1e-12)).all()     # r there = sym_rem(b − 0)
        start = np.array(pose); start[:, 2] = rng.uniform(-3, 3, (2, N))   # every pose start ON the landmark
        out, st = R.conv_pose2point2bearing(o, 1, np.zeros(2), np.ones(2), pt, start, noise=meas, want_status=True)
        assert np.array_equal(out[:, :2], pt)
        assert np.abs(wrap(out[:, 2] + meas[:, 0])).max() < 1e-14      # θ = wrap(−b)
        if solver != 0:                                                # the residual ON the landmark is sym_rem(b − 0) as well
            assert (st == (np.abs(wrap(meas[:, 0])) > 1e-12)).all()
        else:
            assert not st.any()


@pytest.mark.parametrize("kind", ["pb0", "pb1"])
def test_nullhypo_row(kind):
    C_, N = 2, 100
    mu, sigma, fixed, target, _ = _inputs(kind, C_, N, 77)
    o, oo = _opts(N, 1, spread_nh=3.0)
    out, st = _run(kind, o, mu, sigma, fixed, target, nullhypo=0.3)
    ref, rst = bearing_ref.conv(oo, mu, sigma, fixed, target, 1, nullhypo=0.3, spread_nh=3.0)
    assert _delta(out, ref).max() <= 1e-9 and np.array_equal(st, rst)
    b = np.array([[mu[c] + sigma[c] * ro.rng_normals(SEED, SOFF + c, i, 1)[0] for i in range(N)] for c in range(C_)])
    on = _own_residual(kind, b, fixed, out) < 1e-9
    assert 0.5 < on.mean() < 0.9            # ~30 % of the particles are left off the constraint


@pytest.mark.parametrize("kind", ["pb0", "pb1"])
def test_layouts_agree(kind):
    C_, N = 3, 100
    mu, sigma, fixed, target, noise = _inputs(kind, C_, N, 55)
    o, _ = _opts(N, 1)
    soa = _run(kind, o, mu, sigma, fixed, target, noise=noise, want_status=False)
    aos = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
    out = _run(kind, o, mu, sigma, aos(fixed), aos(target), noise=aos(noise), want_status=False, layout=R.LAYOUT_AOS)
    assert np.array_equal(aos(soa), out)
    pts = lambda a: np.ascontiguousarray(R.getPoint(R.Pose2, aos(a))) if a.shape[1] == 3 else aos(a)
    outp = _run(kind, o, mu, sigma, pts(fixed), pts(target), noise=aos(noise), want_status=False, layout=R.LAYOUT_AOS_POINTS)
    back = R.getCoordinates(R.Pose2, outp) if target.shape[1] == 3 else outp
    d = back - aos(soa)
    if target.shape[1] == 3:
        d[..., 2] = wrap(d[..., 2])
    assert np.abs(d).max() < 1e-12


@pytest.mark.parametrize("kind", ["pb0", "pb1"])
@pytest.mark.parametrize("N", [100, 700])
def test_dev_entry_equals_host_twin(kind, N):
    import torch
    from rome_jl_amd import _lib
    lib = _lib.load()
    ctx = R.default_context()
    C_ = 5
    mu, sigma, fixed, target, _ = _inputs(kind, C_, N, 61)
    o, _ = _opts(N, 1)
    host, hst = _run(kind, o, mu, sigma, fixed, target)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")
    out = torch.zeros((C_, target.shape[1], N), dtype=torch.float64, device="cuda:0")
    st = torch.zeros((C_, N), dtype=torch.int32, device="cuda:0")
    keep = [t(mu), t(sigma), t(fixed), t(target)]
    cd = _lib.ConvDev()
    cd.n_conv = C_
    cd.mu, cd.L, cd.bel_fixed, cd.bel_target = (k.data_ptr() for k in keep)
    cd.out, cd.status = out.data_ptr(), st.data_ptr()
    cd.dir_all = int(kind[-1])
    fn = lib.rome_conv_pose2point2bearing_dev
    torch.cuda.synchronize()
    _lib.check(fn(ctx.handle, C.byref(o), C.byref(cd)), ctx.handle)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(st.cpu().numpy(), hst)
    # a dir column and multihypo columns are refused
    dirs = t(np.zeros(C_), torch.int32)
    cd.dir = dirs.data_ptr()
    assert fn(ctx.handle, C.byref(o), C.byref(cd)) == _lib.ERR_INVALID_ARG
    cd.dir = None
    w = t(np.full(C_, 0.5)); alt = t(np.arange(C_), torch.int32)
    cd.hypo_w, cd.alt_var = w.data_ptr(), alt.data_ptr()
    assert fn(ctx.handle, C.byref(o), C.byref(cd)) == _lib.ERR_INVALID_ARG


def test_refuse_n_above_limit():
    from rome_jl_amd import _lib
    N = _lib.MAX_PARTICLES + 1
    o = R.make_opts(N=N, solver=1)
    for d, df, dt in ((0, 3, 2), (1, 2, 3)):
        with pytest.raises(_lib.RomeError) as e:
            R.conv_pose2point2bearing(o, d, [0.3], [0.1], np.zeros((1, df, N)), np.zeros((1, dt, N)))
        assert e.value.code == _lib.ERR_UNSUPPORTED_N


# ------------------------------------------------------------------ 6. whole-graph sweep
def _mixed_graph(N, with_bearing=True, seed=5):
    rng = np.random.default_rng(seed)
    fg = R.initfg(N=N)
    for k in range(3):
        fg.addVariable("x%d" % k, R.Pose2)
    for k in range(3):
        fg.addVariable("l%d" % k, R.Point2)
    cov = np.diag([0.1, 0.1, 0.01])
    fg.addFactor(["x0"], R.PriorPose2(R.MvNormal([0.0, 0.0, 0.0], cov)))
    fg.addFactor(["x0", "x1"], R.Pose2Pose2(R.MvNormal([10.0, 0.0, 0.3], cov)))
    fg.addFactor(["x1", "x2"], R.Pose2Pose2(R.MvNormal([10.0, 0.0, 0.3], cov)))
    fg.addFactor(["x0", "l0"], R.Pose2Point2BearingRange(R.Normal(1.2, 0.05), R.Normal(21.0, 0.3)))
    fg.addFactor(["x2", "l0"], R.Pose2Point2BearingRange(R.Normal(1.6, 0.05), R.Normal(22.0, 0.3)))
    fg.addFactor(["l1"], R.PriorPoint2(R.MvNormal([25.0, 15.0], np.diag([0.1, 0.1]))))
    if with_bearing:
        fg.addFactor(["x0", "l2"], R.Pose2Point2Bearing(R.Normal(0.9, 0.05)))
        fg.addFactor(["x1", "l2"], R.Pose2Point2Bearing(R.Uniform(0.8, 1.4)), nullhypo=0.2)
        fg.addFactor(["x2", "l1"], R.Pose2Point2Bearing(R.Normal(0.4, 0.02)))
    means = {"x0": [0, 0, 0], "x1": [10, 0, 0.3], "x2": [19.5, 3, 0.6], "l0": [5, 20], "l1": [25, 15], "l2": [14, 12]}
    for l, m in means.items():
        d = len(m)
        fg.initVariable(l, np.asarray(m, float)[:, None] + rng.standard_normal((d, N)) * (0.5 if d == 2 else np.array([[0.5], [0.5], [0.05]])))
    return fg


def test_whole_graph_conv_step():
    N = 100
    fg = _mixed_graph(N)
    dg = R.DeviceGraph(fg); dg.upload_beliefs(fg)
    o = R.make_opts(N=N, solver=1, seed=SEED, inflate_cycles=CYC, inflation=INFL)
    dg.conv_step(o, sweep=2)
    prop = {vt: dg.prop[vt].cpu().numpy() for vt in (R.Pose2, R.Point2)}
    fg0 = _mixed_graph(N, with_bearing=False)
    dg0 = R.DeviceGraph(fg0); dg0.upload_beliefs(fg0)
    dg0.conv_step(o, sweep=2)
    n2, npt = dg0.n_prop[R.Pose2], dg0.n_prop[R.Point2]
    assert n2 > 0 and npt > 0
    assert np.array_equal(prop[R.Pose2][:n2], dg0.prop[R.Pose2][:n2].cpu().numpy())       # every other family: bit-identical rows
    assert np.array_equal(prop[R.Point2][:npt], dg0.prop[R.Point2][:npt].cpu().numpy())
    pk = dg.packed
    bel = {vt: pk.beliefs(fg, vt) for vt in (R.Pose2, R.Point2)}
    base = 2 << 32
    pb = pk.pbear
    assert dg.n_prop[R.Point2] == npt + pb["F"] and dg.n_prop[R.Pose2] == n2 + pb["F"]
    for f in range(pb["F"]):
        nh = float(pb["nh"][f])
        oo = ro.make_opts(N=N, solver=0, seed=SEED, stream_offset=base + dg.STREAM_PB1 + f, inflate_cycles=CYC, inflation=INFL)
        ref, _ = bearing_ref.conv_row(oo, pb["mu"][f], pb["sigma"][f], bel[R.Point2][pb["point"][f]], bel[R.Pose2][pb["pose"][f]],
                                      oo.stream_offset, 1, nullhypo=nh, spread_nh=o.spread_nh)
        assert _delta(prop[R.Pose2][n2 + f][None], ref[None]).max() <= 1e-9
        oo = ro.make_opts(N=N, solver=0, seed=SEED, stream_offset=base + dg.STREAM_PB0 + f, inflate_cycles=CYC, inflation=INFL)
        ref, _ = bearing_ref.conv_row(oo, pb["mu"][f], pb["sigma"][f], bel[R.Pose2][pb["pose"][f]], bel[R.Point2][pb["point"][f]],
                                      oo.stream_offset, 1, nullhypo=nh, spread_nh=o.spread_nh)
        assert np.abs(prop[R.Point2][npt + f] - ref).max() <= 1e-9
    assert "pb" not in str(dg.families())


# ------------------------------------------------------------------ 7. the parametric row
def test_linearize_kind6_is_the_bearing_row_of_bearingrange():
    rng = np.random.default_rng(6)
    F = 500
    b = rng.uniform(-3, 3, F); w = rng.uniform(0.5, 30, F)
    xa = np.column_stack([rng.uniform(-20, 20, (F, 2)), rng.uniform(-3, 3, F)]); xb = rng.uniform(-20, 20, (F, 2))
    W2 = np.zeros((F, 2, 2)); W2[:, 0, 0] = w; W2[:, 1, 1] = 1.0
    r2, Ja2, Jb2 = R.linearize(R._lib.FACTOR_POSE2POINT2BR, np.column_stack([b, np.full(F, 7.0)]), W2, xa, xb)
    r, Ja, Jb = R.linearize(R._lib.FACTOR_POSE2POINT2BEARING, b[:, None], w[:, None, None], xa, xb)
    assert r.shape == (F, 1) and Ja.shape == (F, 1, 3) and Jb.shape == (F, 1, 2)
    assert np.abs(r[:, 0] - r2[:, 0]).max() <= 1e-12
    assert np.abs(Ja[:, 0] - Ja2[:, 0]).max() <= 1e-12 and np.abs(Jb[:, 0] - Jb2[:, 0]).max() <= 1e-12


def test_linearize_kind6_jacobians_vs_central_differences():
    rng = np.random.default_rng(7)
    F, h = 400, 1e-6
    b = rng.uniform(-3, 3, F)
    xa = np.column_stack([rng.uniform(-20, 20, (F, 2)), rng.uniform(-3, 3, F)])
    ang = rng.uniform(-math.pi, math.pi, F); dist = rng.uniform(1.0, 30.0, F)                      # ‖l − p.t‖ >= 1: O(1) derivatives
    xb = xa[:, :2] + dist[:, None] * np.column_stack([np.cos(ang), np.sin(ang)])
    r, Ja, Jb = R.linearize(R._lib.FACTOR_POSE2POINT2BEARING, b[:, None], np.ones((F, 1, 1)), xa, xb)
    keep = np.abs(np.abs(r[:, 0]) - math.pi) > 1e-3                                               # off the branch cut
    assert keep.sum() > 0.9 * F
    res = lambda a_, b_: R.residual_pose2point2bearing(b, a_, b_)
    for k in range(3):
        e = np.zeros(3); e[k] = h
        fd = (res(xa + e, xb) - res(xa - e, xb)) / (2 * h)
        assert np.abs(fd - Ja[:, 0, k])[keep].max() <= 1e-7
    for k in range(2):
        e = np.zeros(2); e[k] = h
        fd = (res(xa, xb + e) - res(xa, xb - e)) / (2 * h)
        assert np.abs(fd - Jb[:, 0, k])[keep].max() <= 1e-7


# ------------------------------------------------------------------ 8 - 10. the reference's solves (test/testBearing2D.jl)
def _triangulation_graph(N, x1_prior=None):
    """test/testBearing2D.jl:116-191: three beacons around (10, 0), sighted from x1 at bearings π/2, −π/6, −π + π/6"""
    fg = R.initfg(N=N)
    s = math.sqrt(3) / 2
    beacons = {"l1": (10.0, 1.0), "l2": (10.0 + s, -0.5), "l3": (10.0 - s, -0.5)}
    for l, p in beacons.items():
        fg.addVariable(l, R.Point2)
        fg.addFactor([l], R.PriorPoint2(R.MvNormal(list(p), np.diag([0.01 ** 2, 0.01 ** 2]))))
    fg.addVariable("x1", R.Pose2)
    for l, b in (("l1", math.pi / 2), ("l2", -math.pi / 6), ("l3", -math.pi + math.pi / 6)):
        fg.addFactor(["x1", l], R.Pose2Point2Bearing(R.Normal(b, 0.05)))
    return fg


def test_parametric_triangulation():
    import inspect
    fg = _triangulation_graph(100)
    init = {l: np.array(f.Z.mu, dtype=float) for _, (l, *_), f in fg.factors if isinstance(f, R.PriorPoint2)}
    init["x1"] = np.array([9.5, 0.3, 0.2])
    tol = inspect.signature(R.solveGraphParametric).parameters["tol"].default
    sol = R.solveGraphParametric(fg, init=init)
    x = sol["x1"]
    err = np.abs(np.array([x[0] - 10.0, x[1], wrap(x[2])]))
    print("parametric triangulation: x1 = %s, |error| = %s, solver tol %g" % (x, err, tol))
    assert err.max() <= 10 * tol


def test_narrow_vs_broad_solve():
    """test/testBearing2D.jl:72-114"""
    N = 100
    fg = R.initfg(N=N)
    fg.addVariable("x1", R.Pose2); fg.addVariable("x2", R.Pose2); fg.addVariable("l1", R.Point2)
    tight = np.diag([0.01 ** 2, 0.01 ** 2, 0.001 ** 2])
    fg.addFactor(["x1"], R.PriorPose2(R.MvNormal([10.0, 0.0, 0.0], tight)))
    fg.addFactor(["x2"], R.PriorPose2(R.MvNormal([0.0, 10.0, 0.0], tight)))
    fg.addFactor(["l1"], R.PriorPoint2(R.MvNormal([0.0, 0.0], np.diag([100.0, 100.0]))))
    fg.addFactor(["x1", "l1"], R.Pose2Point2Bearing(R.Normal(math.pi, 0.001)))
    fg.addFactor(["x2", "l1"], R.Pose2Point2Bearing(R.Normal(-math.pi / 2, 0.001)))
    R.initAll(fg)
    labels = [fl for fl, _, f in fg.factors if isinstance(f, R.Pose2Point2Bearing)]
    p1 = R.approxConv(fg, labels[0], "l1")       # from x1 looking along −x: y pinned near 0, x free
    p2 = R.approxConv(fg, labels[1], "l1")       # from x2 looking along −y: x pinned near 0, y free
    assert np.sum(np.abs(p1[0]) < 100) > 30 and np.sum(np.abs(p2[1]) < 100) > 30
    R.solveGraph(fg)
    L = fg.getVal("l1")
    nx, ny = int(np.sum(np.abs(L[0]) < 10)), int(np.sum(np.abs(L[1]) < 10))
    print("narrow-vs-broad: l1 particles with |x| < 10: %d, |y| < 10: %d of %d" % (nx, ny, N))
    assert nx > 60 and ny > 60


@pytest.fixture(scope="module")
def _pose_triangulation():
    N = 100
    fg = _triangulation_graph(N)
    R.initAll(fg)
    fg.initVariable("x1", np.array([[10.0], [0.0], [0.0]]) + np.random.default_rng(0).standard_normal((3, N)) * np.array([[3.0], [3.0], [1.0]]))
    dg = R.DeviceGraph(fg); dg.upload_beliefs(fg)
    o = R.make_opts(N=N, solver=1, seed=SEED)
    dg.conv_step(o, sweep=0)
    rec = dg.family_table("pb1")
    prop = rec["prop"].cpu().numpy()
    pk = dg.packed
    b = np.array([[pk.pbear["mu"][f] + pk.pbear["sigma"][f] * ro.rng_normals(SEED, dg.STREAM_PB1 + f, i, 1)[0] for i in range(N)]
                  for f in range(3)])
    lm = np.stack([pk.beliefs(fg, R.Point2)[pk.pbear["point"][f]] for f in range(3)])
    R.solveGraph(fg)
    X = fg.getVal("x1")
    near = float(np.mean(np.hypot(X[0] - 10.0, X[1]) < 0.3))
    head = float(np.mean(np.abs(wrap(X[2])) < 0.1))
    print("non-parametric pose triangulation: share within 0.3 m = %.2f, share of headings within 0.1 rad = %.2f" % (near, head))
    return dict(fg=fg, prop=prop, b=b, lm=lm, near=near, head=head)


def test_pose_triangulation_hard_assertions(_pose_triangulation):
    t = _pose_triangulation
    for l in t["fg"].ls():
        assert np.isfinite(t["fg"].getVal(l)).all()
    assert _own_residual("pb1", t["b"], t["lm"], t["prop"]).max() <= 1e-9


@pytest.mark.xfail(strict=False, reason="the reference marks this criterion broken too (test/testBearing2D.jl:184-186)")
def test_pose_triangulation_position(_pose_triangulation):
    assert _pose_triangulation["near"] > 0.8


@pytest.mark.xfail(strict=False, reason="the reference marks this criterion broken too (test/testBearing2D.jl:184-186)")
def test_pose_triangulation_heading(_pose_triangulation):
    assert _pose_triangulation["head"] > 0.8


# ------------------------------------------------------------------ 11. the example
def test_example_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "hexagonal_bearing_only.py"), "--sweeps", "3"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("l1 mean")][-1]
    print(line)
    vals = [float(v) for v in line.replace(",", " ").replace("(", " ").replace(")", " ").split() if v.replace(".", "").replace("-", "").replace("e", "").isdigit()]
    assert len(vals) >= 3 and np.isfinite(vals).all()
