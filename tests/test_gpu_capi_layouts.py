"""The one layout staging path of the C API's host side (stage_blocks / fetch_blocks): a store window and every host-pointer
convolution give, in the three host layouts, the SAME coordinates -- exactly.  SoA <-> AoS is a copy; the native-point layout runs the
device conversion kernels of rome_points_to_coords / rome_coords_to_points on the same values, so it is exact too once the coordinates
under test are those kernels' own image of the points."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PD = C.POINTER(C.c_double)
DIMS = (3, 2, 6)   # Pose2, Point2, Pose3


@pytest.fixture(scope="module", autouse=True)
def _pkg():
    global R, _lib
    import rome_jl_amd
    from rome_jl_amd import _lib as L
    R, _lib = rome_jl_amd, L
    R.default_context()
    yield


def _canonical(rng, n, N, dim):
    """n blocks: native points [n][N][pl] and the coordinates [n][N][dim] the device conversion gives for exactly those points."""
    x = rng.standard_normal((n * N, dim)) * (1.0 if dim != 6 else np.array([2.0, 2.0, 2.0, 0.6, 0.6, 0.6]))
    pts = R.coords_to_points(dim, x)
    return pts.reshape(n, N, -1), R.points_to_coords(dim, pts).reshape(n, N, dim)


def _in_layout(layout, pts, coords):
    if layout == _lib.LAYOUT_AOS_POINTS:
        return np.ascontiguousarray(pts)
    return np.ascontiguousarray(coords.transpose(0, 2, 1) if layout == _lib.LAYOUT_SOA else coords)


def _expect(layout, coords):
    """what a download / a convolution must return in `layout` when the SoA coordinates are coords^T"""
    if layout == _lib.LAYOUT_AOS_POINTS:
        n, N, dim = coords.shape
        return R.coords_to_points(dim, coords.reshape(n * N, dim)).reshape(n, N, -1)
    return np.ascontiguousarray(coords.transpose(0, 2, 1) if layout == _lib.LAYOUT_SOA else coords)


@pytest.mark.parametrize("N", [33, 64])
def test_store_window_roundtrip_in_every_layout(N):
    """Store (3 Pose2, 2 Point2, 2 Pose3): upload a window (first in {0, 1}, count in {0, 1, rest}) in each layout, download it in each
    layout: exact, and nothing outside the window is written."""
    lib, ctx = _lib.load(), R.default_context()
    nv = (3, 2, 2)
    h = C.c_void_p()
    _lib.check(lib.rome_store_create(ctx.handle, N, nv[0], nv[1], nv[2], C.byref(h)), ctx.handle)
    layouts = (_lib.LAYOUT_SOA, _lib.LAYOUT_AOS, _lib.LAYOUT_AOS_POINTS)
    rng = np.random.default_rng(100 + N)
    try:
        for t, dim in enumerate(DIMS):
            pts, coords = _canonical(rng, nv[t], N, dim)
            for first in (0, 1):
                for count in (0, 1, nv[t] - first):
                    w = slice(first, first + count)
                    for up in layouts:
                        zero = np.zeros((nv[t], dim, N))
                        _lib.check(lib.rome_store_upload(h, _lib.LAYOUT_SOA, t, 0, nv[t], zero.ctypes.data_as(PD)), ctx.handle)
                        src = _in_layout(up, pts[w], coords[w]) if count else np.zeros(1)
                        _lib.check(lib.rome_store_upload(h, up, t, first, count, src.ctypes.data_as(PD)), ctx.handle)
                        whole = np.full((nv[t], dim, N), np.nan)
                        _lib.check(lib.rome_store_download(h, _lib.LAYOUT_SOA, t, 0, nv[t], whole.ctypes.data_as(PD)), ctx.handle)
                        want = np.zeros((nv[t], dim, N)); want[w] = coords[w].transpose(0, 2, 1)
                        assert np.array_equal(whole, want), (t, first, count, up)
                        for down in layouts:
                            ref = _expect(down, coords[w]) if count else np.zeros(1)
                            got = np.full(ref.shape, np.nan)
                            _lib.check(lib.rome_store_download(h, down, t, first, count, got.ctypes.data_as(PD)), ctx.handle)
                            assert np.array_equal(got, ref) if count else np.isnan(got).all(), (t, first, count, up, down)
    finally:
        lib.rome_store_destroy(h)


def _conv_cases(N, rng):
    """(name, call(opts, layout-aware blocks) -> output) for every host-pointer convolution, C = 3; blocks are made per layout by `B`"""
    Cn = 3
    P2, X2 = _canonical(rng, 2 * Cn, N, 3)     # Pose2: blocks 0..2 fixed, 3..5 target / alternative
    PL, XL = _canonical(rng, 2 * Cn, N, 2)     # Point2
    P3, X3 = _canonical(rng, 2 * Cn, N, 6)     # Pose3
    blk = {"p2": (P2, X2), "pt": (PL, XL), "p3": (P3, X3)}
    a, b = slice(0, Cn), slice(Cn, 2 * Cn)
    mu3 = rng.standard_normal((Cn, 3)); cov3 = np.tile(np.diag([0.1, 0.1, 0.05]) ** 2, (Cn, 1, 1))
    mu6 = rng.standard_normal((Cn, 6)) * 0.5; cov6 = np.tile(np.diag([0.1] * 3 + [0.05] * 3) ** 2, (Cn, 1, 1))
    mubr = np.stack([rng.uniform(-1, 1, Cn), rng.uniform(5, 20, Cn)], 1); sgbr = np.tile([0.03, 0.3], (Cn, 1))
    mur = rng.uniform(5, 20, Cn); sgr = np.full(Cn, 0.3); mub = rng.uniform(-1, 1, Cn); sgb = np.full(Cn, 0.03)
    mu2 = rng.standard_normal((Cn, 2)); cov2 = np.tile(np.diag([0.5, 0.7]) ** 2, (Cn, 1, 1))
    hw = np.array([0.5, 0.3, 0.9])
    nz3 = rng.standard_normal((Cn, N, 3)); nz6 = rng.standard_normal((Cn, N, 6))

    def B(lay, kind, s):
        return _in_layout(lay, blk[kind][0][s], blk[kind][1][s])

    def Z(lay, nz):   # noise rows are measurement coordinates in every layout: AoS unless the layout is SoA
        return np.ascontiguousarray(nz.transpose(0, 2, 1)) if lay == _lib.LAYOUT_SOA else nz

    return [
        ("pose2pose2", 3, lambda o, l: R.conv_pose2pose2(o, mu3, cov3, B(l, "p2", a), B(l, "p2", b), dirs=[0, 1, 0], noise=Z(l, nz3))),
        ("pose2pose2_mh", 3, lambda o, l: R.conv_pose2pose2(o, mu3, cov3, B(l, "p2", a), B(l, "p2", b), dirs=1, alt=B(l, "p2", b), hypo_w=hw)),
        ("pose2point2br_0", 2, lambda o, l: R.conv_pose2point2br(o, 0, mubr, sgbr, B(l, "p2", a), B(l, "pt", a))),
        ("pose2point2br_1", 3, lambda o, l: R.conv_pose2point2br(o, 1, mubr, sgbr, B(l, "pt", a), B(l, "p2", a))),
        ("pose2point2br_mh", 3, lambda o, l: R.conv_pose2point2br(o, 1, mubr, sgbr, B(l, "pt", a), B(l, "p2", a), alt=B(l, "pt", b), hypo_w=hw)),
        ("pose3pose3", 6, lambda o, l: R.conv_pose3pose3(o, mu6, cov6, B(l, "p3", a), B(l, "p3", b), dirs=[1, 0, 0], noise=Z(l, nz6))),
        ("point2point2range", 2, lambda o, l: R.conv_point2point2range(o, mur, sgr, B(l, "pt", a), B(l, "pt", b), dirs=[0, 1, 0])),
        ("pose2point2range_0", 2, lambda o, l: R.conv_pose2point2range(o, 0, mur, sgr, B(l, "p2", a), B(l, "pt", a))),
        ("pose2point2range_1", 3, lambda o, l: R.conv_pose2point2range(o, 1, mur, sgr, B(l, "pt", a), B(l, "p2", a))),
        ("pose2point2bearing_0", 2, lambda o, l: R.conv_pose2point2bearing(o, 0, mub, sgb, B(l, "p2", a), B(l, "pt", a))),
        ("pose2point2bearing_1", 3, lambda o, l: R.conv_pose2point2bearing(o, 1, mub, sgb, B(l, "pt", a), B(l, "p2", a))),
        ("priorpose2", 3, lambda o, l: R.sample_priorpose2(o, mu3, cov3)),
        ("priorpose3", 6, lambda o, l: R.sample_priorpose3(o, mu6, cov6)),
        ("priorpoint2", 2, lambda o, l: R.sample_priorpoint2(o, mu2, cov2)),
    ]


@pytest.mark.parametrize("N", [33, 100])
def test_host_convolution_is_the_same_in_every_layout(N):
    """Every host-pointer convolution (multihypo Pose2Pose2 and bearing-range included), C = 3, seeded: the AoS result is the SoA
    result transposed and the native-point result is rome_coords_to_points of it -- exactly."""
    for name, dim, call in _conv_cases(N, np.random.default_rng(7 + N)):
        soa = call(R.make_opts(N=N, solver=1, seed=11, layout=_lib.LAYOUT_SOA), _lib.LAYOUT_SOA)
        assert soa.shape == (3, dim, N) and np.isfinite(soa).all(), name
        coords = np.ascontiguousarray(soa.transpose(0, 2, 1))
        for lay in (_lib.LAYOUT_AOS, _lib.LAYOUT_AOS_POINTS):
            got = call(R.make_opts(N=N, solver=1, seed=11, layout=lay), lay)
            assert np.array_equal(got, _expect(lay, coords)), (name, lay, np.abs(got - _expect(lay, coords)).max())


def test_blockop_plan_created_run_and_destroyed_on_a_non_current_device():
    """A block-operation plan of a context on device 0, created, run and destroyed while ANOTHER device is the caller's current one."""
    import torch
    lib = _lib.load()
    if lib.rome_device_count() < 2:
        pytest.skip("needs two visible devices")
    ctx = R.default_context()
    N = 33
    rng = np.random.default_rng(3)
    bel = rng.standard_normal((2, 3, N))
    st, plan = C.c_void_p(), C.c_void_p()
    _lib.check(lib.rome_store_create(ctx.handle, N, 2, 0, 0, C.byref(st)), ctx.handle)
    prev = torch.cuda.current_device()
    try:
        _lib.check(lib.rome_store_upload(st, _lib.LAYOUT_SOA, 0, 0, 2, bel.ctypes.data_as(PD)), ctx.handle)
        torch.cuda.set_device((ctx.device + 1) % lib.rome_device_count())
        i32 = lambda v: np.array([v], dtype=np.int32)
        ty, a, dst = i32(0), i32(0), i32(1)
        PI = C.POINTER(C.c_int32)
        _lib.check(lib.rome_blockop_plan_create(ctx.handle, st, 0, 1, ty.ctypes.data_as(PI), a.ctypes.data_as(PI), None, dst.ctypes.data_as(PI),
                                                C.byref(plan)), ctx.handle)
        torch.cuda.set_device((ctx.device + 1) % lib.rome_device_count())
        _lib.check(lib.rome_blockop_plan_run(plan), ctx.handle)
        torch.cuda.set_device((ctx.device + 1) % lib.rome_device_count())
        lib.rome_blockop_plan_destroy(plan)
        got = np.zeros((2, 3, N))
        _lib.check(lib.rome_store_download(st, _lib.LAYOUT_SOA, 0, 0, 2, got.ctypes.data_as(PD)), ctx.handle)
        assert np.array_equal(got[1], bel[0]) and np.array_equal(got[0], bel[0])
    finally:
        lib.rome_store_destroy(st)
        torch.cuda.set_device(prev)
