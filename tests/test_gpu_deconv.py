"""Deconvolution on the device (k_deconv<Policy> of rome.jl_amd/csrc/rome_conv.hpp behind rome_deconv / rome_deconv_dev, api.deconv,
R.approxDeconv, R.factorMMD, DeviceGraph.deconv / factor_mmd) against the references of tests/deconv_ref.py.

Bounds are deconv_ref.Reference's (8 x the float64 restatement's deviation from mpmath, floor 64 ulp, times max(1, largest |reference
entry| of the row)), computed on the CPU; angular entries modulo 2 pi.  Figures: profiles/deconv_reference_errors.md.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import deconv_ref as dr

pytestmark = pytest.mark.gpu

FAMS = sorted(dr.FAMILIES)
SHAPES = [(N, Cn) for N in (1, 2, 63, 64, 65, 100, 128, 129, 513) for Cn in (1, 3, 7)] + [(4096, 1)]
SEED = 0x524F4D45


@pytest.fixture(scope="module", autouse=True)
def _pkg():
    global R, _lib, torch
    import torch as T
    import rome_jl_amd
    from rome_jl_amd import _lib as L
    R, _lib, torch = rome_jl_amd, L, T
    R.default_context()
    yield


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _cls(fam):
    return getattr(R, dr.FAMILIES[fam][0])


def _params(fam, Cn, seed=0):
    """mu (C, dz), the noise parameters as the host entries take them, and the device table L"""
    rng = np.random.default_rng(500 + seed)
    dz = dr.FAMILIES[fam][1]
    mu = rng.uniform(-1.0, 1.0, (Cn, dz)) + (3.0 if fam in ("p2rng", "pprng") else 0.0)
    if fam in ("p2p2", "p3p3", "p3xyy", "p3rot"):
        Q = rng.standard_normal((Cn, dz, dz))
        cov = 0.01 * (Q @ np.swapaxes(Q, 1, 2) + dz * np.eye(dz))
        return mu, cov, R.cholesky_lower(cov)
    sig = rng.uniform(0.05, 0.2, (Cn, dz))
    if dz == 1:
        return mu[:, 0], sig[:, 0], sig
    return mu, sig, sig


def _opts(N, **kw):
    kw.setdefault("seed", SEED)
    return R.make_opts(N=N, solver=R.SOLVER_CLOSED_FORM, **kw)


def _dev(fam, opts, mu, L, A, B, rows4=None, noise=None, pred=True, meas=True, n_rows=None, cols=None):
    """rome_deconv_dev on device copies of host SoA arrays -> (code, pred, meas)"""
    ctx = R.default_context()
    dev = torch.device("cuda", 0)
    t = lambda x, dt=None: None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dt or torch.float64, device=dev)
    dz = dr.FAMILIES[fam][1]
    Cn = n_rows if n_rows is not None else (len(rows4) if rows4 is not None else len(A))
    N = opts.n_particles
    keep = [t(np.reshape(mu, (-1, dz))), t(L), t(A), t(B), t(noise), t(rows4, torch.int32)]
    keep += [t(c, torch.int32) for c in (cols or (None, None, None))]
    tp = torch.full((max(Cn, 1), dz, N), float("nan"), dtype=torch.float64, device=dev) if pred else None
    tm = torch.full((max(Cn, 1), dz, N), float("nan"), dtype=torch.float64, device=dev) if meas else None
    ptr = lambda x: None if x is None else x.data_ptr()
    tab = _lib.DeconvTable(n_rows=Cn, factor=ptr(keep[6]), var_a=ptr(keep[7]), var_b=ptr(keep[8]), rows4=ptr(keep[5]), mu=ptr(keep[0]), L=ptr(keep[1]),
                           bel_a=ptr(keep[2]), bel_b=ptr(keep[3]), noise=ptr(keep[4]), pred=ptr(tp), meas=ptr(tm))
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    rc = _lib.load().rome_deconv_dev(ctx.handle, C.byref(opts), getattr(_lib, "DECONV_" + dr.FAMILIES[fam][0].upper().replace("BEARINGRANGE", "BR")),
                                     C.byref(tab))
    torch.cuda.synchronize(dev)
    return rc, None if tp is None else tp.cpu().numpy(), None if tm is None else tm.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _geometry(fam):
    """the generic table of a family as 3 blocks of N = 43, its references (computed once) and the kernel's outputs on it"""
    A, B = dr.geometry_table(fam)
    ref = dr.Reference(fam, A, B, dr.subset_rows(len(A)))
    mu, _, L = _params(fam, 3)
    rc, pred, meas = _dev(fam, _opts(43), mu, L, dr.blocks(A, 3, 43), dr.blocks(B, 3, 43))
    assert rc == 0
    return A, B, ref, dr.rows_of(pred), meas


# ------------------------------------------------------------------------------------------------------------------ values, functor
@pytest.mark.parametrize("fam", FAMS)
def test_values_against_mp_and_numpy(fam):
    _, _, ref, pred, _ = _geometry(fam)
    d_mp, bound = ref.check_mp(pred)
    d_np, _ = ref.check_np(pred)
    print("%s: kernel - mp %.3e, kernel - numpy %.3e, bound %.3e (numpy - mp %.3e)" % (fam, d_mp, d_np, bound, ref.figure))
    assert np.isfinite(pred).all()
    assert d_mp <= bound and d_np <= bound


def _residual(fam, z, A, B):
    fn = {"p2p2": R.residual_pose2pose2, "br": R.residual_pose2point2br, "pbear": R.residual_pose2point2bearing,
          "p2rng": R.residual_point2point2range, "pprng": R.residual_pose2point2range, "p3p3": R.residual_pose3pose3,
          "p3xyy": R.residual_pose3pose3xyyaw, "p3rot": R.residual_pose3pose3rotation}[fam]
    r = fn(z[:, 0] if z.shape[1] == 1 else z, A, B)
    return np.reshape(r, (len(A), -1))


@pytest.mark.parametrize("fam", FAMS)
def test_functor_vanishes_at_the_prediction(fam):
    """the library's own residual functor (the coordinate entry rome_residual_*) at (pred; p, q)"""
    A, B, ref, pred, _ = _geometry(fam)
    r = np.abs(_residual(fam, pred, A, B)).max(axis=1) / dr.row_scale(ref.np)
    print("%s: max |r| / scale %.3e, bound %.3e" % (fam, r.max(), ref.rel_bound))
    assert r.max() <= ref.rel_bound


# ------------------------------------------------------------------------------------------------------------------ launch geometry
def _inputs(fam, Cn, N, seed):
    rng = np.random.default_rng(seed)
    _, dz, da, db, _ = dr.FAMILIES[fam]
    A, B = rng.uniform(-2.0, 2.0, (Cn, da, N)), rng.uniform(-2.0, 2.0, (Cn, db, N))
    for X in (A, B):
        if X.shape[1] == 6:
            X[:, 3:] *= 0.25   # rotation vectors of at most 0.87 rad: every relative rotation stays below 1.74, clear of pi
    return A, B


@pytest.mark.parametrize("fam", FAMS)
def test_launch_geometry(fam):
    mu7, _, L7 = _params(fam, 7, seed=1)
    dz = dr.FAMILIES[fam][1]
    mu7 = np.reshape(mu7, (7, dz))
    rc, _, _ = _dev(fam, _opts(4096), mu7[:1], L7[:1], *_inputs(fam, 1, 8, 0), n_rows=0)   # C == 0: a no-op whatever the arrays
    assert rc == 0
    o = _opts(4096); o.n_particles = 4097
    assert _lib.load().rome_deconv_dev(R.default_context().handle, C.byref(o), 0, C.byref(_lib.DeconvTable(n_rows=1))) == _lib.ERR_UNSUPPORTED_N
    for N, Cn in SHAPES:
        A, B = _inputs(fam, Cn, N, 31 * N + Cn)
        mu, L = mu7[:Cn], L7[:Cn]
        rc, pred, meas = _dev(fam, _opts(N, stream_offset=1000), mu, L, A, B)
        assert rc == 0 and np.isfinite(pred).all() and np.isfinite(meas).all(), (N, Cn)
        # pred against the restatement on every row (the same bound as the value test's: these inputs are inside its ranges)
        d = dr.deviation(fam, dr.rows_of(pred), dr.np_predict(fam, dr.rows_of(A), dr.rows_of(B))).max()
        assert d <= 64.0 * dr.EPS * 8.0, (N, Cn, d)   # (scale: |entries| <= 2 sqrt 2 x 2 < 8)
        # row c of the C-row call == the one-row call on the same inputs with stream_offset + c
        for c in range(Cn):
            rc, p1, m1 = _dev(fam, _opts(N, stream_offset=1000 + c), mu[c:c + 1], L[c:c + 1], A[c:c + 1], B[c:c + 1])
            assert rc == 0 and np.array_equal(_bits(p1[0]), _bits(pred[c])) and np.array_equal(_bits(m1[0]), _bits(meas[c])), (N, Cn, c)
        if Cn >= 3:
            # one row's inputs at positions 0, 2 and C - 1 (rows4 names the same blocks there): the same bits of pred, and of meas when the
            # samples are given (a position is a Philox stream otherwise)
            rows4 = np.stack([np.arange(Cn), np.zeros(Cn, int), np.arange(Cn), np.arange(Cn)], axis=1)
            for pos in (0, 2, Cn - 1):
                rows4[pos] = (1, 0, 1, 1)
            xi = np.random.default_rng(N).standard_normal((Cn, dz, N))
            for pos in (2, Cn - 1):
                xi[pos] = xi[0]
            rc, p3, m3 = _dev(fam, _opts(N), mu, L, A, B, rows4=rows4, noise=xi)
            assert rc == 0
            for pos in (2, Cn - 1):
                assert np.array_equal(_bits(p3[pos]), _bits(p3[0])) and np.array_equal(_bits(m3[pos]), _bits(m3[0])), (N, Cn, pos)
            assert np.array_equal(_bits(p3[0]), _bits(pred[1]))
            # repeated and permuted variable blocks, through rows4 and through the three columns
            rng = np.random.default_rng(Cn + N)
            f, va, vb = rng.integers(0, Cn, Cn + 2), rng.integers(0, Cn, Cn + 2), rng.permutation(np.arange(Cn + 2) % Cn)
            rows4 = np.stack([f, np.zeros(Cn + 2, int), va, vb], axis=1)
            rc, p4, m4 = _dev(fam, _opts(N, stream_offset=7), mu, L, A, B, rows4=rows4)
            rc2, p5, m5 = _dev(fam, _opts(N, stream_offset=7), mu[f], L[f], A[va], B[vb])
            rc3, p6, m6 = _dev(fam, _opts(N, stream_offset=7), mu, L, A, B, n_rows=Cn + 2, cols=(f, va, vb))
            assert rc == 0 and rc2 == 0 and rc3 == 0
            assert np.array_equal(_bits(p4), _bits(p5)) and np.array_equal(_bits(m4), _bits(m5)), (N, Cn)
            assert np.array_equal(_bits(p6), _bits(p5)) and np.array_equal(_bits(m6), _bits(m5)), (N, Cn)


# ------------------------------------------------------------------------------------------------------------------ edges
def _one_block(fam, A, B):
    mu, _, L = _params(fam, 1)
    rc, pred, _ = _dev(fam, _opts(len(A)), mu, L, dr.blocks(A, 1, len(A)), dr.blocks(B, 1, len(A)), meas=False)
    assert rc == 0
    return dr.rows_of(pred)


def test_edges_pose2_headings():
    A, B = dr.pose2_edge_table()
    ref = dr.Reference("p2p2", A, B)
    pred = _one_block("p2p2", A, B)
    d, bound = ref.check_mp(pred)
    print("heading edges: kernel - mp %.3e, bound %.3e; headings %s" % (d, bound, pred[:, 2]))
    assert d <= bound and (np.abs(pred[:, 2]) <= np.pi).all()


@pytest.mark.parametrize("fam", ["br", "pbear", "pprng"])
def test_edges_landmark_distances(fam):
    A, B = dr.landmark_edge_table()
    ref = dr.Reference(fam, A, B)
    d, bound = ref.check_mp(_one_block(fam, A, B))
    print("%s distances 1e-6 .. 1e6: kernel - mp %.3e, bound %.3e" % (fam, d, bound))
    assert d <= bound


@pytest.mark.parametrize("fam", ["br", "pbear", "pprng"])
def test_edges_landmark_on_the_pose(fam):
    """the row's own output is whatever the library's atan2(0, 0) gives (printed; 0 as measured), every other row is what it is with an
    ordinary row in that place"""
    A, B = dr.landmark_edge_table()
    B2 = B.copy(); B2[4] = A[4, :2]
    got, base = _one_block(fam, A, B2), _one_block(fam, A, B)
    print("%s with the landmark on the pose: %s" % (fam, got[4]))
    assert np.isfinite(got[4]).all() and got[4][-1 if fam == "br" else 0] == 0.0
    keep = np.arange(len(A)) != 4
    assert np.array_equal(_bits(got[keep]), _bits(base[keep]))


@pytest.mark.parametrize("fam", ["p3p3", "p3rot", "p3xyy"])
def test_edges_pose3_rotations(fam):
    """relative rotations 0, 1e-9, 1 and pi - 1e-3 about coordinate and generic axes, rotation vectors beyond the principal range on the
    inputs.  Near pi the bound is the restatement's own deviation THERE (its matrix Log divides by sin), not a wider table"""
    A, B = dr.pose3_edge_table()
    near = dr.near_pi_rows(A, B)
    rest = np.setdiff1d(np.arange(len(A)), near)
    pred = _one_block(fam, A, B)
    for name, rows in (("near pi", near), ("elsewhere", rest)):
        ref = dr.Reference(fam, A[rows], B[rows])
        d, bound = ref.check_mp(pred[rows])
        print("%s %s: kernel - mp %.3e, bound %.3e (numpy - mp %.3e)" % (fam, name, d, bound, ref.figure))
        assert d <= bound
    if fam != "p3xyy":
        assert (np.linalg.norm(pred[:, -3:], axis=1) <= np.pi * (1 + 4 * dr.EPS)).all()   # the principal rotation vector


# ------------------------------------------------------------------------------------------------------------------ samples
@pytest.mark.parametrize("fam", FAMS)
def test_samples_given_and_from_normals(fam):
    import mpmath as mp
    Cn, N = 3, 43
    dz = dr.FAMILIES[fam][1]
    mu, _, L = _params(fam, Cn, seed=2)
    A, B = _inputs(fam, Cn, N, 5)
    xi = np.random.default_rng(9).standard_normal((Cn, dz, N))
    rc, _, m = _dev(fam, _opts(N, presampled=_lib.NOISE_MEASUREMENTS), mu, L, A, B, noise=xi, pred=False)
    assert rc == 0 and np.array_equal(_bits(m), _bits(xi))
    rc, _, m = _dev(fam, _opts(N), mu, L, A, B, noise=xi, pred=False)
    assert rc == 0
    # z = mu + L xi: NumPy against mp (exact products and sums at 50 digits) gives the rule's figure; the kernel within 8 x, floor 64 ulp
    mu2 = np.reshape(mu, (Cn, dz))
    Lm = np.zeros((Cn, dz, dz))
    if L.shape[1] == dz * (dz + 1) // 2 and dz > 1 and fam != "br":
        il = np.tril_indices(dz)
        Lm[:, il[0], il[1]] = L
    else:
        Lm[:, np.arange(dz), np.arange(dz)] = np.reshape(L, (Cn, dz))
    z_np = mu2[:, :, None] + np.einsum("cij,cjn->cin", Lm, xi)
    z_mp = np.array([[[float(mp.mpf(mu2[c, i]) + sum(mp.mpf(Lm[c, i, j]) * mp.mpf(xi[c, j, n]) for j in range(dz))) for n in range(N)]
                      for i in range(dz)] for c in range(Cn)])
    scale = np.maximum(1.0, np.abs(z_mp).max(axis=1, keepdims=True))
    figure = (np.abs(z_np - z_mp) / scale).max()
    bound = max(8.0 * figure, 64.0 * dr.EPS)
    d = (np.abs(m - z_mp) / scale).max()
    print("%s: mu + L xi kernel - mp %.3e, numpy - mp %.3e, bound %.3e" % (fam, d, figure, bound))
    assert d <= bound


@pytest.mark.parametrize("fam", ["p2p2", "p3p3"])
def test_samples_are_the_draw_of_the_convolution(fam):
    """noise = NULL: the convolution of the row, and the convolution fed deconv's `meas` as pre-sampled measurements, give the same proposals
    bit for bit (CLOSED_FORM): the kernel shares the draw (seed, stream_offset + c, particle) with the sweeps"""
    for N in (100, 33):
        Cn = 5
        mu, cov, L = _params(fam, Cn, seed=3)
        A, B = _inputs(fam, Cn, N, 6)
        conv = R.conv_pose2pose2 if fam == "p2p2" else R.conv_pose3pose3
        rc, _, meas = _dev(fam, _opts(N, stream_offset=40), mu, L, A, B, pred=False)
        assert rc == 0
        own = conv(_opts(N, stream_offset=40), mu, cov, A, B)
        fed = conv(_opts(N, stream_offset=40, presampled=_lib.NOISE_MEASUREMENTS), mu, cov, A, B, noise=meas)
        assert np.array_equal(_bits(own), _bits(fed)), (fam, N)


# ------------------------------------------------------------------------------------------------------------------ round trip
def _conv_dir0(fam, o, mu, prm, A, B0, z):
    if fam == "p2p2":
        return R.conv_pose2pose2(o, mu, prm, A, B0, noise=z)
    if fam == "br":
        return R.conv_pose2point2br(o, 0, mu, prm, A, B0, noise=z)
    if fam == "pbear":
        return R.conv_pose2point2bearing(o, 0, mu, prm, A, B0, noise=z)
    if fam == "p2rng":
        return R.conv_point2point2range(o, mu, prm, A, B0, noise=z)
    if fam == "pprng":
        return R.conv_pose2point2range(o, 0, mu, prm, A, B0, noise=z)
    if fam == "p3p3":
        return R.conv_pose3pose3(o, mu, prm, A, B0, noise=z)
    if fam == "p3xyy":
        return R.conv_pose3pose3xyyaw(o, mu, prm, A, B0, noise=z)
    return R.conv_pose3pose3rotation(o, mu, prm, A, B0, noise=z)


@pytest.mark.parametrize("fam", FAMS)
def test_round_trip(fam):
    """q' = conv(p; z) for given measurement rows z (CLOSED_FORM, direction 0), then deconv(p, q') returns z.  Every family's direction 0
    determines what the measurement constrains: the unique root (Pose2Pose2, bearing-range, Pose3Pose3; the partial Pose3 factors on
    their coordinates, the start belief upright so that the yaw root is exact), or a member of the ring / ray of roots whose range /
    bearing IS the measurement.  The round trip passes through q', which is rounded at its own magnitude: the row scale is
    max(1, largest |entry| of z, p, q'), the bound 64 ulp of it (the floor of the rule; both closed forms are a few operations each)."""
    Cn, N = 3, 43
    _, dz, da, db, ang = dr.FAMILIES[fam]
    rng = np.random.default_rng(12)
    mu, prm, L = _params(fam, Cn, seed=4)
    A = dr.blocks(dr.geometry_table(fam, Cn * N, seed=3)[0], Cn, N)
    z = rng.uniform(-1.5, 1.5, (Cn, dz, N))
    if fam in ("p2rng", "pprng"):
        z = rng.uniform(0.5, 8.0, (Cn, dz, N))
    if fam == "br":
        z[:, 1] = rng.uniform(0.5, 8.0, (Cn, N))
    B0 = rng.uniform(-3.0, 3.0, (Cn, db, N))   # start points: they select the member of a ring / ray, and carry the untouched coordinates
    if db == 6:
        B0[:, 3:] = 0.0
    o = _opts(N, presampled=_lib.NOISE_MEASUREMENTS, inflate_cycles=1, inflation=0.0)
    Bq = _conv_dir0(fam, o, mu, prm, A, B0, z)
    rc, pred, _ = _dev(fam, _opts(N), mu, L, A, Bq, meas=False)
    assert rc == 0
    d = pred - z
    for k in ang:
        d[:, k] = np.arctan2(np.sin(d[:, k]), np.cos(d[:, k]))
    scale = np.maximum(1.0, np.maximum(np.abs(z).max(axis=1), np.maximum(np.abs(A).max(axis=1), np.abs(Bq).max(axis=1))))
    worst = (np.abs(d).max(axis=1) / scale).max()
    print("%s: round trip |pred - z| / scale %.3e, bound %.3e" % (fam, worst, 64.0 * dr.EPS))
    assert worst <= 64.0 * dr.EPS


# ------------------------------------------------------------------------------------------------------------------ optional outputs, layouts
@pytest.mark.parametrize("fam", FAMS)
def test_optional_outputs_and_layouts(fam):
    Cn, N = 3, 43
    _, dz, da, db, _ = dr.FAMILIES[fam]
    mu, prm, L = _params(fam, Cn, seed=5)
    A, B = _inputs(fam, Cn, N, 8)
    o = _opts(N, stream_offset=3)
    rc, pred, meas = _dev(fam, o, mu, L, A, B)
    rc1, p1, m1 = _dev(fam, o, mu, L, A, B, meas=False)
    rc2, p2, m2 = _dev(fam, o, mu, L, A, B, pred=False)
    assert (rc, rc1, rc2) == (0, 0, 0) and m1 is None and p2 is None
    assert np.array_equal(_bits(p1), _bits(pred)) and np.array_equal(_bits(m2), _bits(meas))
    assert _dev(fam, o, mu, L, A, B, pred=False, meas=False)[0] == _lib.ERR_INVALID_ARG
    PD = C.POINTER(C.c_double)
    hptr = [np.ascontiguousarray(x, dtype=np.float64).ctypes.data_as(PD) for x in (np.reshape(mu, (Cn, dz)), prm, A, B)]
    assert _lib.load().rome_deconv(R.default_context().handle, C.byref(o), R.deconv_family(_cls(fam))[0], Cn, *hptr, None, None, None) == _lib.ERR_INVALID_ARG
    assert _lib.load().rome_deconv(R.default_context().handle, C.byref(o), 8, Cn, *hptr, None, None, None) == _lib.ERR_INVALID_ARG
    # the host entry in the three layouts == the device entry, bit for bit
    hp, hm = R.deconv(_cls(fam), o, mu, prm, A, B)
    assert np.array_equal(_bits(hp), _bits(pred)) and np.array_equal(_bits(hm), _bits(meas))
    only_p, none_m = R.deconv(_cls(fam), o, mu, prm, A, B, want=("pred",))
    assert none_m is None and np.array_equal(_bits(only_p), _bits(pred))
    aos = lambda X: np.ascontiguousarray(X.transpose(0, 2, 1))
    oa = _opts(N, stream_offset=3, layout=R.LAYOUT_AOS)
    ap, am = R.deconv(_cls(fam), oa, mu, prm, aos(A), aos(B))
    assert np.array_equal(_bits(ap), _bits(aos(pred))) and np.array_equal(_bits(am), _bits(aos(meas)))
    # native points: the device entry on the coordinates the library itself reads from the points
    pts = lambda X, d: X if d == 2 else R.coords_to_points(d, X.reshape(-1, d)).reshape(Cn, N, -1)
    back = lambda P, d: P if d == 2 else R.points_to_coords(d, P.reshape(Cn * N, -1)).reshape(Cn, N, d)
    PA, PB = pts(aos(A), da), pts(aos(B), db)
    op = _opts(N, stream_offset=3, layout=R.LAYOUT_AOS_POINTS)
    pp, pm = R.deconv(_cls(fam), op, mu, prm, PA, PB)
    rc, pred2, _ = _dev(fam, o, mu, L, aos(back(PA, da)), aos(back(PB, db)), meas=False)
    assert rc == 0 and np.array_equal(_bits(pp), _bits(aos(pred2))) and np.array_equal(_bits(pm), _bits(aos(meas)))


# ------------------------------------------------------------------------------------------------------------------ graph level
def _hexagon(seed=3):
    fg = R.generateGraph_Hexagonal(N=100)
    R.dead_reckon_init(fg, seed=seed)
    fg.initVariable("l1", np.array([[20.0], [0.0]]) + np.random.default_rng(0).standard_normal((2, 100)))
    return fg


def test_graph_level():
    fg = _hexagon()
    dg = R.DeviceGraph(fg)
    dg.upload_beliefs(fg)
    o = _opts(100, seed=7, stream_offset=11)
    pred, meas = dg.deconv(o, "p2p2")
    torch.cuda.synchronize()
    pk = dg.packed
    assert dg.deconv_labels("p2p2") == pk.p2p2["labels"] and tuple(pred.shape) == (6, 3, 100)
    bel = pk.beliefs(fg, R.Pose2)
    hp, hm = R.deconv(R.Pose2Pose2, o, pk.p2p2["mu"], pk.p2p2["cov"], bel[pk.p2p2["var_from"]], bel[pk.p2p2["var_to"]])
    assert np.array_equal(_bits(pred.cpu().numpy()), _bits(hp)) and np.array_equal(_bits(meas.cpu().numpy()), _bits(hm))
    for k, fl in enumerate(pk.p2p2["labels"]):   # the per-factor wrapper: the same pairs (its stream is the call's own)
        ap, _ = R.approxDeconv(fg, fl, seed=7)
        assert np.array_equal(_bits(ap), _bits(hp[k]))
    # the bearing-range record, either name: each factor once
    bp, bm = dg.deconv(o, "br0", meas=False)
    assert bm is None and tuple(bp.shape) == (2, 2, 100) and torch.equal(bp, dg.deconv(o, "br1")[0])
    # factor_mmd == R.mmd on the downloaded arrays
    score = dg.factor_mmd(o, "p2p2")
    torch.cuda.synchronize()
    want = R.mmd(hp, hm, bw=0.001)
    assert np.array_equal(_bits(score.cpu().numpy()), _bits(want))
    assert R.factorMMD(fg, seed=7, stream_offset=11) == dict(zip(pk.p2p2["labels"], want.tolist()))
    # captured once, replayed once: the eager bits
    out = torch.zeros(6, dtype=torch.float64, device=dg.device)
    g = dg.capture(lambda: dg.factor_mmd(o, "p2p2", out=out))
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, score)
    # refusals
    with pytest.raises(TypeError, match="br1"):
        dg.factor_mmd(o, "br1")
    with pytest.raises(TypeError, match="prior"):
        dg.deconv(o, "prior2")
    with pytest.raises(KeyError):
        dg.deconv(o, "p3p3")
    with pytest.raises(ValueError):
        dg.deconv(o, "p2p2", pred=False, meas=False)
    fg2 = R.initfg(N=100)
    for l in ("x0", "x1", "x2"):
        fg2.addVariable(l, R.Pose2)
        fg2.initVariable(l, np.zeros((3, 100)))
    fg2.addFactor(["x0", "x1", "x2"], R.Pose2Pose2(R.MvNormal([1.0, 0, 0], 0.01 * np.eye(3))), multihypo=[1.0, 0.5, 0.5])
    dg2 = R.DeviceGraph(fg2)
    with pytest.raises(ValueError, match="multihypo"):
        dg2.deconv(o, "p2p2")
    with pytest.raises(ValueError, match="multihypo"):
        dg2.factor_mmd(o, "p2p2")


def test_the_reference_test_on_the_device():
    """test/testBasicPose2Conv.jl:20-56: x0 = 100 points of 0.01 randn, approxConv through Pose2Pose2(MvNormal([10, 0, pi], 0.1 I)) gives
    x1, approxDeconv on the pair, and `mmd(M, pts, meas) < 0.001`"""
    fg = R.initfg(N=100)
    fg.addVariable("x0", R.Pose2)
    fg.addVariable("x1", R.Pose2)
    fl = fg.addFactor(["x0", "x1"], R.Pose2Pose2(R.MvNormal([10.0, 0.0, np.pi], 0.1 * np.eye(3))))
    fg.initVariable("x0", 0.01 * np.random.default_rng(0).standard_normal((3, 100)))
    fg.initVariable("x1", R.approxConv(fg, fl, "x1", seed=1))
    pred, meas = R.approxDeconv(fg, fl, seed=2)
    assert pred.shape == (3, 100) and meas.shape == (3, 100)
    v = R.mmd(pred, meas)
    print("mmd(pred, meas) = %.3e" % v)
    assert v < 0.001
    assert R.factorMMD(fg, [fl], seed=2)[fl] == v
