"""Range-only factors on the device: Point2Point2Range and Pose2Point2Range (RoME src/factors/Range2D.jl).

Residual entries against hand values and numpy; the convolutions against range_ref (a per-row restatement over the oracle's primitives)
for every factor x direction, solver, particle count (PPL 1/2/4/8 and k_conv_big) and noise source; layouts, _dev twins and refusals;
one whole-graph sweep against range_ref and against the same graph without range factors; and two solves: the reference's bimodal
trilateration (test/testPoint2Point2.jl:44-98) and range-only Pose2 localisation."""
import ctypes as C

import numpy as np
import pytest

import oracle as ro
import range_ref

pytestmark = pytest.mark.gpu
R = None


@pytest.fixture(scope="module", autouse=True)
def _pkg():
    global R
    import rome_jl_amd
    R = rome_jl_amd
    R.default_context()
    yield


SEED, SOFF, CYC, INFL = 23, 7, 3, 5.0


def _opts(N, solver, **kw):
    o = R.make_opts(N=N, solver=solver, seed=SEED, stream_offset=SOFF, inflate_cycles=CYC, inflation=INFL, **kw)
    oo = ro.make_opts(N=N, solver=0, seed=SEED, stream_offset=SOFF, inflate_cycles=CYC, inflation=INFL)
    return o, oo


def _inputs(kind, C_, N, seed):
    """kind: "p2r" (both directions mixed), "ppr0" (pose -> landmark), "ppr1" (landmark -> pose)"""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(5, 30, C_); sigma = rng.uniform(0.1, 1.0, C_)
    df, dt = {"p2r": (2, 2), "ppr0": (3, 2), "ppr1": (2, 3)}[kind]
    centre = rng.uniform(-40, 40, (C_, 2, 1))
    fixed = np.zeros((C_, df, N)); fixed[:, :2] = centre + 0.5 * rng.standard_normal((C_, 2, N))
    target = np.zeros((C_, dt, N)); target[:, :2] = centre + rng.uniform(-25, 25, (C_, 2, 1)) + 2.0 * rng.standard_normal((C_, 2, N))
    if df == 3:
        fixed[:, 2] = rng.uniform(-3, 3, (C_, 1)) + 0.1 * rng.standard_normal((C_, N))
    if dt == 3:
        target[:, 2] = rng.uniform(-3, 3, (C_, 1)) + 0.1 * rng.standard_normal((C_, N))
    dirs = rng.integers(0, 2, C_).astype(np.int32)
    noise = rng.standard_normal((C_, 1, N))
    return mu, sigma, fixed, target, dirs, noise


def _run(kind, o, mu, sigma, fixed, target, dirs, noise=None, want_status=True, layout=None):
    if kind == "p2r":
        return R.conv_point2point2range(o, mu, sigma, fixed, target, dirs=dirs, noise=noise, want_status=want_status, layout=layout)
    return R.conv_pose2point2range(o, int(kind[-1]), mu, sigma, fixed, target, noise=noise, want_status=want_status, layout=layout)


# ------------------------------------------------------------------ residual entries
def test_residual_hand_values():
    r = R.residual_point2point2range([100.0, 5.0, 10.0], [[100.0, 0.0], [0.0, 0.0], [1.0, 2.0]], [[0.0, 0.0], [3.0, 4.0], [1.0, 2.0]])
    assert np.array_equal(r, [0.0, 0.0, 10.0])
    r = R.residual_pose2point2range([100.0, 7.0], [[100.0, 0.0, 1.3], [0.0, 0.0, -2.0]], [[0.0, 0.0], [0.0, 5.0]])
    assert np.array_equal(r, [0.0, 2.0])


def test_residual_pose_heading_independent_and_numpy():
    rng = np.random.default_rng(4)
    n = 1000
    z = rng.uniform(0, 50, n); p = rng.uniform(-30, 30, (n, 3)); lm = rng.uniform(-30, 30, (n, 2))
    r = R.residual_pose2point2range(z, p, lm)
    p2 = p.copy(); p2[:, 2] = rng.uniform(-10, 10, n)
    assert np.array_equal(r, R.residual_pose2point2range(z, p2, lm))
    ref = z - np.hypot(lm[:, 0] - p[:, 0], lm[:, 1] - p[:, 1])
    assert np.abs(r - ref).max() < 1e-12
    r2 = R.residual_point2point2range(z, p[:, :2], lm)
    assert np.abs(r2 - ref).max() < 1e-12
    assert R.calcFactorResidualTemporary(R.Point2Point2Range(R.Normal(100, 1)), (R.Point2, R.Point2), [100.0],
                                         ([100.0, 0.0], [0.0, 0.0])) == 0.0


# ------------------------------------------------------------------ convolution parity against range_ref
@pytest.mark.parametrize("kind", ["p2r", "ppr0", "ppr1"])
@pytest.mark.parametrize("solver", [0, 1, 3])
@pytest.mark.parametrize("N", [50, 100, 256, 400, 700])
@pytest.mark.parametrize("given_noise", [False, True])
def test_conv_vs_range_ref(kind, solver, N, given_noise):
    C_ = 3
    mu, sigma, fixed, target, dirs, noise = _inputs(kind, C_, N, 100 + N + solver)
    sigma[0] = -sigma[0]                    # one Uniform row
    o, oo = _opts(N, solver)
    nz = noise if given_noise else None
    out, st = _run(kind, o, mu, sigma, fixed, target, dirs, noise=nz)
    ref, rst = range_ref.conv(oo, mu, sigma, fixed, target, solver, noise=nz)
    d = np.abs(out - ref)
    assert d.max() <= 1e-9, d.max()
    if solver != 0:
        assert np.array_equal(st, rst)
    else:
        assert not st.any()
    if kind == "ppr1":
        assert np.array_equal(out[:, 2], target[:, 2])   # the heading passes through bit for bit
    # every particle lies on its ring
    a = fixed[:, :2]
    rho = np.array([[range_ref.measurement(mu[c], sigma[c], nz[c, 0, i] if given_noise else ro.rng_normals(SEED, SOFF + c, i, 1)[0])
                     for i in range(N)] for c in range(C_)])
    assert np.abs(np.hypot(out[:, 0] - a[:, 0], out[:, 1] - a[:, 1]) - rho).max() < 1e-9


def test_in_kernel_rng_is_the_oracle_d1_rule():
    """ρ of a row with zero inflation / one cycle from the start point itself: the radial projection with ξ = ro.rng_normals(..., 1)"""
    N = 100
    mu, sigma, fixed, target, dirs, _ = _inputs("p2r", 2, N, 9)
    o = R.make_opts(N=N, solver=0, seed=SEED, stream_offset=SOFF, inflate_cycles=1, inflation=0.0)
    out = R.conv_point2point2range(o, mu, sigma, fixed, target, dirs=dirs)
    rho = np.hypot(out[:, 0] - fixed[:, 0], out[:, 1] - fixed[:, 1])
    xi = np.array([[ro.rng_normals(SEED, SOFF + c, i, 1)[0] for i in range(N)] for c in range(2)])
    assert np.abs(rho - (mu[:, None] + sigma[:, None] * xi)).max() < 1e-11


@pytest.mark.parametrize("kind", ["p2r", "ppr0", "ppr1"])
def test_nelder_mead_vs_range_ref(kind):
    C_, N = 4, 100
    mu, sigma, fixed, target, dirs, noise = _inputs(kind, C_, N, 31)
    o, oo = _opts(N, 2)
    out = _run(kind, o, mu, sigma, fixed, target, dirs, noise=noise, want_status=False)
    ref, _ = range_ref.conv(oo, mu, sigma, fixed, target, 2, noise=noise)
    d = np.abs(out - ref).max(axis=1)
    assert np.median(d) < 1e-9
    assert np.mean(d < 1e-6) >= 0.95
    rho = mu[:, None] + sigma[:, None] * noise[:, 0]
    r = np.abs(rho - np.hypot(out[:, 0] - fixed[:, 0], out[:, 1] - fixed[:, 1]))
    assert np.percentile(r, 99) < 1e-3
    if kind == "ppr1":
        assert np.array_equal(out[:, 2], target[:, 2])


# ------------------------------------------------------------------ edge cases
def test_edge_rows_rho_nonpositive_and_start_on_anchor():
    N = 64
    fixed = np.zeros((3, 2, N)); fixed[:, 0] = 5.0; fixed[:, 1] = -2.0
    target = np.array(fixed)                              # every start point ON the anchor
    target[0] += np.random.default_rng(1).standard_normal((2, N))
    meas = np.zeros((3, 1, N)); meas[0] = -1.0; meas[1] = 0.0; meas[2] = 4.0   # ρ < 0, ρ = 0, ρ > 0 from t == a
    o = R.make_opts(N=N, solver=1, inflate_cycles=1, inflation=0.0, presampled=1)
    out, st = R.conv_point2point2range(o, np.zeros(3), np.ones(3), fixed, target, noise=meas, want_status=True)
    assert np.array_equal(out[0], fixed[0]) and np.array_equal(out[1], fixed[1])   # ρ <= 0: the anchor
    assert (st[0] == 1).all() and (st[1] == 1).all()
    assert np.array_equal(out[2, 0], fixed[2, 0] + 4.0) and np.array_equal(out[2, 1], fixed[2, 1])   # t == a: along +x
    assert not st[2].any()
    # the same rows under the other solvers (GAUSS_NEWTON: never converges for ρ < 0)
    for solver in (0, 3):
        o = R.make_opts(N=N, solver=solver, inflate_cycles=1, inflation=0.0, presampled=1)
        out2, st2 = R.conv_point2point2range(o, np.zeros(3), np.ones(3), fixed, target, noise=meas, want_status=True)
        assert np.array_equal(out2, out)
        if solver == 3:
            assert (st2[0] == 1).all() and not st2[2].any()


def test_pose_heading_passes_through_exactly():
    N = 100
    mu, sigma, fixed, target, _, _ = _inputs("ppr1", 3, N, 12)
    target[:, 2] = np.random.default_rng(2).uniform(-9, 9, (3, N))   # unwrapped headings too
    for solver in (0, 1, 2, 3):
        o, _ = _opts(N, solver)
        out = R.conv_pose2point2range(o, 1, mu, sigma, fixed, target)
        assert np.array_equal(out[:, 2], target[:, 2])


@pytest.mark.parametrize("kind", ["p2r", "ppr1"])
def test_nullhypo_row(kind):
    C_, N = 2, 100
    mu, sigma, fixed, target, dirs, _ = _inputs(kind, C_, N, 77)
    o, oo = _opts(N, 1, nullhypo=0.3, spread_nh=3.0)
    out, st = _run(kind, o, mu, sigma, fixed, target, dirs)
    ref, rst = range_ref.conv(oo, mu, sigma, fixed, target, 1, nullhypo=0.3, spread_nh=3.0)
    assert np.abs(out - ref).max() <= 1e-9 and np.array_equal(st, rst)
    rho_ok = np.abs(np.hypot(out[:, 0] - fixed[:, 0], out[:, 1] - fixed[:, 1]) - mu[:, None]) < 6 * sigma[:, None]
    assert 0.5 < rho_ok.mean() < 0.9          # ~30 % of the particles are left off the ring


# ------------------------------------------------------------------ layouts, _dev twins, refusals
@pytest.mark.parametrize("kind", ["p2r", "ppr0", "ppr1"])
def test_layouts_agree(kind):
    C_, N = 3, 100
    mu, sigma, fixed, target, dirs, noise = _inputs(kind, C_, N, 55)
    o, _ = _opts(N, 1)
    soa = _run(kind, o, mu, sigma, fixed, target, dirs, noise=noise, want_status=False)
    aos = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
    out = _run(kind, o, mu, sigma, aos(fixed), aos(target), dirs, noise=aos(noise), want_status=False, layout=R.LAYOUT_AOS)
    assert np.array_equal(aos(soa), out)
    pts = lambda a: np.ascontiguousarray(R.getPoint(R.Pose2, aos(a))) if a.shape[1] == 3 else aos(a)
    outp = _run(kind, o, mu, sigma, pts(fixed), pts(target), dirs, noise=aos(noise), want_status=False, layout=R.LAYOUT_AOS_POINTS)
    back = R.getCoordinates(R.Pose2, outp) if target.shape[1] == 3 else outp
    d = back - aos(soa)
    if target.shape[1] == 3:
        d[..., 2] = np.arctan2(np.sin(d[..., 2]), np.cos(d[..., 2]))
    assert np.abs(d).max() < 1e-12


@pytest.mark.parametrize("kind", ["p2r", "ppr0", "ppr1"])
@pytest.mark.parametrize("N", [100, 700])
def test_dev_entries_equal_host_twins(kind, N):
    import torch
    from rome_jl_amd import _lib
    lib = _lib.load()
    ctx = R.default_context()
    C_ = 5
    mu, sigma, fixed, target, dirs, _ = _inputs(kind, C_, N, 61)
    o, _ = _opts(N, 1)
    host, hst = _run(kind, o, mu, sigma, fixed, target, dirs)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")
    dt = target.shape[1]
    out = torch.zeros((C_, dt, N), dtype=torch.float64, device="cuda:0")
    st = torch.zeros((C_, N), dtype=torch.int32, device="cuda:0")
    keep = [t(mu), t(sigma), t(fixed), t(target), t(dirs, torch.int32)]
    cd = _lib.ConvDev()
    cd.n_conv = C_
    cd.mu, cd.L, cd.bel_fixed, cd.bel_target = (k.data_ptr() for k in keep[:4])
    cd.out, cd.status = out.data_ptr(), st.data_ptr()
    if kind == "p2r":
        cd.dir = keep[4].data_ptr()
        fn = lib.rome_conv_point2point2range_dev
    else:
        cd.dir_all = int(kind[-1])
        fn = lib.rome_conv_pose2point2range_dev
    torch.cuda.synchronize()
    _lib.check(fn(ctx.handle, C.byref(o), C.byref(cd)), ctx.handle)
    ctx.synchronize()
    assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(st.cpu().numpy(), hst)
    # multihypo columns are refused
    w = t(np.full(C_, 0.5)); alt = t(np.arange(C_), torch.int32)
    cd.hypo_w, cd.alt_var = w.data_ptr(), alt.data_ptr()
    assert fn(ctx.handle, C.byref(o), C.byref(cd)) == _lib.ERR_INVALID_ARG


def test_refuse_n_above_limit():
    from rome_jl_amd import _lib
    N = _lib.MAX_PARTICLES + 1
    o = R.make_opts(N=N, solver=1)
    with pytest.raises(_lib.RomeError) as e:
        R.conv_point2point2range(o, [10.0], [1.0], np.zeros((1, 2, N)), np.zeros((1, 2, N)))
    assert e.value.code == _lib.ERR_UNSUPPORTED_N
    with pytest.raises(_lib.RomeError) as e:
        R.conv_pose2point2range(o, 1, [10.0], [1.0], np.zeros((1, 2, N)), np.zeros((1, 3, N)))
    assert e.value.code == _lib.ERR_UNSUPPORTED_N


# ------------------------------------------------------------------ whole-graph sweep
def _mixed_graph(N, with_range=True, seed=5):
    rng = np.random.default_rng(seed)
    fg = R.initfg(N=N)
    for k in range(3):
        fg.addVariable("x%d" % k, R.Pose2)
    for k in range(4):
        fg.addVariable("l%d" % k, R.Point2)
    fg.addFactor(["x0"], R.PriorPose2(R.MvNormal([0.0, 0.0, 0.0], np.diag([0.1, 0.1, 0.01]))))
    fg.addFactor(["x0", "x1"], R.Pose2Pose2(R.MvNormal([10.0, 0.0, 0.3], np.diag([0.1, 0.1, 0.01]))))
    fg.addFactor(["x1", "x2"], R.Pose2Pose2(R.MvNormal([10.0, 0.0, 0.3], np.diag([0.1, 0.1, 0.01]))))
    fg.addFactor(["l0"], R.PriorPoint2(R.MvNormal([5.0, 20.0], np.diag([0.1, 0.1]))))
    fg.addFactor(["l1"], R.PriorPoint2(R.MvNormal([25.0, 15.0], np.diag([0.1, 0.1]))))
    if with_range:
        fg.addFactor(["l0", "l2"], R.Point2Point2Range(R.Normal(12.0, 0.5)))
        fg.addFactor(["l1", "l2"], R.Point2Point2Range(R.Uniform(10.0, 14.0)), nullhypo=0.2)
        fg.addFactor(["x1", "l3"], R.Pose2Point2Range(R.Normal(15.0, 0.3)))
        fg.addFactor(["x2", "l1"], R.Pose2Point2Range(R.Normal(9.0, 0.3)))
        fg.addFactor(["l2", "l3"], R.Point2Point2Range(R.Normal(7.0, 0.4)))
    means = {"x0": [0, 0, 0], "x1": [10, 0, 0.3], "x2": [19.5, 3, 0.6], "l0": [5, 20], "l1": [25, 15], "l2": [14, 12], "l3": [12, 15]}
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
    fg0 = _mixed_graph(N, with_range=False)
    dg0 = R.DeviceGraph(fg0); dg0.upload_beliefs(fg0)
    dg0.conv_step(o, sweep=2)
    n2, npt = dg0.n_prop[R.Pose2], dg0.n_prop[R.Point2]
    assert np.array_equal(prop[R.Pose2][:n2], dg0.prop[R.Pose2][:n2].cpu().numpy())
    assert np.array_equal(prop[R.Point2][:npt], dg0.prop[R.Point2][:npt].cpu().numpy())
    pk = dg.packed
    bel = {vt: pk.beliefs(fg, vt) for vt in (R.Pose2, R.Point2)}
    base = 2 << 32
    r2, rp = pk.p2rng, pk.pprng
    assert dg.n_prop[R.Point2] == npt + 2 * r2["F"] + rp["F"] and dg.n_prop[R.Pose2] == n2 + rp["F"]
    nh = lambda f: float(f)
    for f in range(r2["F"]):
        for dr in (0, 1):
            fx, tg = (r2["from"][f], r2["to"][f]) if dr == 0 else (r2["to"][f], r2["from"][f])
            oo = ro.make_opts(N=N, solver=0, seed=SEED, stream_offset=base + dg.STREAM_P2RNG + 2 * f + dr, inflate_cycles=CYC, inflation=INFL)
            ref, _ = range_ref.conv_row(oo, r2["mu"][f], r2["sigma"][f], bel[R.Point2][fx], bel[R.Point2][tg], oo.stream_offset, 1,
                                        nullhypo=nh(r2["nh"][f]), spread_nh=o.spread_nh)
            assert np.abs(prop[R.Point2][npt + 2 * f + dr] - ref).max() <= 1e-9
    for f in range(rp["F"]):
        oo = ro.make_opts(N=N, solver=0, seed=SEED, stream_offset=base + dg.STREAM_PPRNG1 + f, inflate_cycles=CYC, inflation=INFL)
        ref, _ = range_ref.conv_row(oo, rp["mu"][f], rp["sigma"][f], bel[R.Point2][rp["point"][f]], bel[R.Pose2][rp["pose"][f]],
                                    oo.stream_offset, 1)
        assert np.abs(prop[R.Pose2][n2 + f] - ref).max() <= 1e-9
        oo = ro.make_opts(N=N, solver=0, seed=SEED, stream_offset=base + dg.STREAM_PPRNG0 + f, inflate_cycles=CYC, inflation=INFL)
        ref, _ = range_ref.conv_row(oo, rp["mu"][f], rp["sigma"][f], bel[R.Pose2][rp["pose"][f]], bel[R.Point2][rp["point"][f]],
                                    oo.stream_offset, 1)
        assert np.abs(prop[R.Point2][npt + 2 * r2["F"] + f] - ref).max() <= 1e-9
    assert "p2rng" not in str(dg.families())


# ------------------------------------------------------------------ reference scenarios
def test_bimodal_trilateration():
    """test/testPoint2Point2.jl:44-98: two ranges of 100 from (100, 0) and (0, 100) put l1 near (0, 0) AND (100, 100)."""
    N = 100
    fg = R.initfg(N=N)
    for l in ("x0", "x1", "l1"):
        fg.addVariable(l, R.Point2)
    fg.addFactor(["x0"], R.PriorPoint2(R.MvNormal([100.0, 0.0], np.eye(2))))
    fg.addFactor(["x1"], R.PriorPoint2(R.MvNormal([0.0, 100.0], np.eye(2))))
    fg.addFactor(["x0", "l1"], R.Point2Point2Range(R.Normal(100.0, 1.0)))
    fg.addFactor(["x1", "l1"], R.Point2Point2Range(R.Normal(100.0, 1.0)))
    fg.initVariable("l1", np.random.default_rng(0).uniform(-50, 150, (2, N)))
    R.solveGraph(fg, product="gibbs", gibbs_iters=3, n_sweeps=10)
    L1 = fg.getVal("l1")
    near = lambda v, p: np.hypot(v[0] - p[0], v[1] - p[1]) < 20
    f00, f11 = near(L1, (0, 0)).mean(), near(L1, (100, 100)).mean()
    far = (np.abs(L1) > 120).any(axis=0).mean()
    fx0, fx1 = near(fg.getVal("x0"), (100, 0)).mean(), near(fg.getVal("x1"), (0, 100)).mean()
    print("bimodal trilateration: l1 near (0,0) %.2f, near (100,100) %.2f, beyond 120 %.2f; x0 %.2f, x1 %.2f" % (f00, f11, far, fx0, fx1))
    assert f00 > 0.05 and f11 > 0.05
    assert far < 0.35
    assert fx0 > 0.8 and fx1 > 0.8


def test_range_only_pose2_localisation():
    N = 100
    truth = np.array([20.0, 15.0, 0.3])
    beacons = {"b1": (0.0, 0.0), "b2": (50.0, 0.0), "b3": (0.0, 50.0)}
    fg = R.initfg(N=N)
    fg.addVariable("x0", R.Pose2)
    fg.addFactor(["x0"], R.PriorPose2(R.MvNormal([35.0, 5.0, 0.3], np.diag([30.0 ** 2, 30.0 ** 2, 0.01 ** 2]))))
    for b, p in beacons.items():
        fg.addVariable(b, R.Point2)
        fg.addFactor([b], R.PriorPoint2(R.MvNormal(list(p), np.diag([0.01, 0.01]))))
        fg.addFactor(["x0", b], R.Pose2Point2Range(R.Normal(float(np.hypot(truth[0] - p[0], truth[1] - p[1])), 0.3)))
    R.solveGraph(fg, product="gibbs")
    X = fg.getVal("x0")
    err = np.hypot(X[0].mean() - truth[0], X[1].mean() - truth[1])
    dth = abs(np.arctan2(np.sin(X[2]), np.cos(X[2])).mean() - 0.3)
    print("range-only Pose2 localisation: |mean - truth| = %.3f m, heading offset %.4f rad" % (err, dth))
    assert err < 1.0
    assert dth < 0.1
