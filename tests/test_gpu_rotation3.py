"""Pose3Pose3Rotation on the device (RoME src/factors/PartialPose3.jl:204-227).

The residual entries against mpmath in both layouts; the closed form / NEWTON / GAUSS_NEWTON roots against the mp root at every launch
shape (every particles-per-lane instantiation and k_conv_big), with given noise and the device's own draws; Nelder-Mead against the
restatement; nullhypo, layouts, the _dev twin, argument errors; solveGraph with the partial-aware product.  References and bounds come
from tests/rotation3_ref.py: 8x the float64 restatement's own deviation from mp with a floor of 64 ulp, relative to max(1, largest
|reference entry| of the row).  Every convolution test also asserts the pass-through rule: the translation comes back bit for bit."""
import ctypes as C
import functools
import json
import math
import os

import numpy as np
import pytest

import oracle as ro
import rotation3_ref as r3

pytestmark = pytest.mark.gpu
R = None
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "rotation3_kats.json")))


@pytest.fixture(scope="module", autouse=True)
def _pkg():
    global R
    import rome_jl_amd
    R = rome_jl_amd
    R.default_context()
    yield


SEED, SOFF = 23, 7
NS = [1, 64, 65, 100, 129, 256, 257, 512, 513]     # PPL 1 | 1, 2 | 2, 4 | 4, 8 | 8, k_conv_big
DIRS = [0, 1, 0]


def _opts(N, solver, **kw):
    o = R.make_opts(N=N, solver=solver, seed=SEED, stream_offset=SOFF, **kw)
    oo = ro.make_opts(N=N, solver=0, seed=SEED, stream_offset=SOFF, inflate_cycles=o.inflate_cycles, inflation=o.inflation)
    return o, oo


def _unit(rng, shape):
    v = rng.standard_normal(shape + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _poses(rng, C_, N, max_angle):
    """[C_][6][N]: translations within +-40, rotation vectors of norm <= max_angle about random axes"""
    w = _unit(rng, (C_, N)) * rng.uniform(0, max_angle, (C_, N, 1))
    return np.concatenate([rng.uniform(-40, 40, (C_, 3, N)), w.transpose(0, 2, 1)], axis=1)


def _frozen(*arrs):
    for a in arrs:
        if a is not None:
            a.setflags(write=False)
    return arrs


# ------------------------------------------------------------------ 1. residual rows
@pytest.mark.parametrize("group", ["phi_tiny", "phi_mid", "near_pi_1e-3", "pose_coords", "generic"])
def test_residual_rows_against_mp(group):
    """both layouts; residual rotations 0, 1e-12, 1e-6, 0.1, 1, 3, pi - 1e-3 about generic and coordinate axes; pose rotation vectors of
    norm 0, 1e-9, pi - 1e-6, 4, 7"""
    t, co, pt = r3.residual_references()[group]
    dev, bound = co.check(R.residual_pose3pose3rotation(t["z"], t["p"], t["q"]))
    print("%s coordinates: %.3e of %.3e (restatement %.3e)" % (group, dev, bound, co.figure))
    devp, boundp = pt.check(R.residual_pose3pose3rotation_pt(t["z"], t["p_pt"], t["q_pt"]))
    print("%s points:      %.3e of %.3e (restatement %.3e)" % (group, devp, boundp, pt.figure))
    assert dev <= bound and devp <= boundp


def test_residual_reference_kats():
    """test/testPartialPose3.jl:520-547: p = identity, q = RotXYZ(rpy), z = rpy, |r| < 1e-10; through both entries and
    calcFactorResidualTemporary with the hat-form measurement"""
    cases = KATS["kats"]["cases"]
    z, p, q = (np.array([c[k] for c in cases]) for k in ("z", "p", "q"))
    assert (np.linalg.norm(R.residual_pose3pose3rotation_pt(z, p, q), axis=1) < 1e-10).all()
    pc, qc = R.getCoordinates(R.Pose3, p), R.getCoordinates(R.Pose3, q)
    assert (np.linalg.norm(R.residual_pose3pose3rotation(z, pc, qc), axis=1) < 1e-10).all()
    f = R.Pose3Pose3Rotation(R.MvNormal(z[1], 0.001 * np.eye(3)))
    for c in cases:
        x, y, w = c["z"]
        hat = np.array([[0, -w, y], [w, 0, -x], [-y, x, 0]]).flatten(order="F")
        assert np.linalg.norm(R.calcFactorResidualTemporary(f, (R.Pose3, R.Pose3), hat, (c["p"], c["q"]))) < 1e-10
        assert np.linalg.norm(R.calcFactorResidualTemporary(f, (R.Pose3, R.Pose3), c["z"], (pc[0], R.getCoordinates(R.Pose3, c["q"])))) < 1e-10
    g = KATS["residual_rows"]                                # the stored mp rows
    d = np.abs(R.residual_pose3pose3rotation(g["z"], g["p"], g["q"]) - np.array(g["mp"])).max()
    assert d <= r3.residual_references()["generic"][1].rel_bound * max(1.0, np.abs(g["mp"]).max())


# ------------------------------------------------------------------ 2. closed form and NEWTON
@functools.lru_cache(maxsize=None)
def _root_case(N, given):
    """C = 3 rows, both directions: rows 0 and 1 with |mu| <= 1.6 and sigma about 0.05, row 2 with |mu| = 4 and sigma = 1e-3 (the functor has
    no zero there).  The fixed rotations are kept small enough that every root rotation stays below 2.7 rad, where the restatement's
    log formula is good to rounding.  -> inputs, the restatement on every particle, the mp root on a subset, the Table of that subset"""
    rng = np.random.default_rng(3000 + N + (7 if given else 0))
    mu = np.concatenate([_unit(rng, (2,)) * rng.uniform(0.5, 1.6, (2, 1)), _unit(rng, (1,)) * 4.0])
    A = rng.uniform(-0.03, 0.03, (3, 3, 3))
    cov = A @ A.transpose(0, 2, 1) + (0.04 ** 2) * np.eye(3)
    cov[2] = (1e-3 ** 2) * np.eye(3)
    fixed = np.concatenate([_poses(rng, 2, N, 0.5), _poses(rng, 1, N, 0.3)])
    target = _poses(rng, 3, N, 1.0)
    noise = np.clip(rng.standard_normal((3, 3, N)), -3, 3) if given else None
    _, oo = _opts(N, 1)
    ref, rst, z = r3.rot_conv(oo, DIRS, mu, cov, fixed, target, r3.NEWTON, noise=noise)
    assert not rst[:2].any() and rst[2].all()
    sub = r3.subset(N, seed=N)
    mp = np.stack([r3.mp_root(DIRS[c], z[c][sub], fixed[c].T[sub]) for c in range(3)])            # [3][S][3]
    table = r3.Table(mp.reshape(-1, 3), ref[:, 3:, sub].transpose(0, 2, 1).reshape(-1, 3))
    assert np.linalg.norm(ref[:, 3:], axis=1).max() < 2.7
    return _frozen(mu, cov, fixed, target, ref, rst, noise) + (sub, table)


def _check_roots(out, ref, sub, table, rows=slice(None)):
    """the subset against mp within the bound; every particle against the restatement within bound + figure (the restatement itself
    lies within the figure of mp)"""
    got = out[rows][:, 3:, sub].transpose(0, 2, 1).reshape(-1, 3)
    n = len(got)
    d = np.abs(got - table.ref[:n]).max(axis=1) / table.scale[:n]
    dn = np.abs(out[rows][:, 3:] - ref[rows][:, 3:]).max(axis=1) / np.maximum(1.0, np.abs(ref[rows][:, 3:]).max(axis=1))
    return float(d.max()), table.rel_bound, float(dn.max()), table.rel_bound + table.figure


@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("solver", [0, 1])
def test_root_vs_mp(solver, N, given):
    mu, cov, fixed, target, ref, rst, noise, sub, table = _root_case(N, given)
    o, _ = _opts(N, solver)
    out, st = R.conv_pose3pose3rotation(o, mu, cov, fixed, target, dirs=DIRS, noise=noise, want_status=True)
    d, bound, dn, boundn = _check_roots(out, ref, sub, table)
    print("solver %d N %d given %d: mp %.3e of %.3e, restatement %.3e of %.3e" % (solver, N, given, d, bound, dn, boundn))
    assert d <= bound and dn <= boundn
    assert np.array_equal(out[:, :3], target[:, :3])                    # the translation: bit for bit
    if solver == 1:
        assert np.array_equal(st, rst)                                   # 0 on rows 0, 1; 1 on the |mu| = 4 row
    else:
        assert not st.any()


def test_stored_root_rows_and_status_up_to_3_rad():
    """the 48 stored rows (|z| <= 3, both directions, one particle each, the measurement given): the mp root, status 0"""
    rr = KATS["root_rows"]
    dirs, z, fixed, mp = np.array(rr["dirs"], dtype=np.int32), np.array(rr["z"]), np.array(rr["fixed"]), np.array(rr["mp"])
    table = r3.root_reference()[1]
    assert np.array_equal(table.ref, mp)
    o, _ = _opts(1, 1, presampled=1)
    target = np.random.default_rng(5).standard_normal((48, 6, 1))
    out, st = R.conv_pose3pose3rotation(o, np.zeros((48, 3)), np.stack([np.eye(3)] * 48), fixed[:, :, None], target, dirs=dirs,
                                        noise=z[:, :, None], want_status=True)
    dev, bound = table.check(out[:, 3:, 0])
    print("stored roots: %.3e of %.3e" % (dev, bound))
    assert dev <= bound and not st.any() and np.array_equal(out[:, :3], target[:, :3])
    assert np.linalg.norm(z, axis=1).max() > 2.9


def test_zero_covariance_row_through_the_dev_entry():
    """|mu| = 4 and 2.5 with a ZERO Cholesky factor: z = mu on every particle.  The host entry takes covariances and refuses a singular
    one (ROME_ERR_NOT_POSDEF, as the XYYaw entry does), so the row runs on device tables.  Status 1 on the |mu| = 4 row, 0 on the other;
    the same rotation Exp(mu) either way."""
    import torch
    from rome_jl_amd import _lib
    lib, ctx = _lib.load(), R.default_context()
    N = 100
    rng = np.random.default_rng(61)
    mu = np.array([[0.0, 2.4, -3.2], [1.5, -2.0, 0.0]])
    assert np.allclose(np.linalg.norm(mu, axis=1), [4.0, 2.5])       # (roots below 2.8 rad: the restatement good to rounding)
    dirs = np.array([0, 1], dtype=np.int32)
    fixed, target = _poses(rng, 2, N, 0.3), _poses(rng, 2, N, 1.0)
    o, _ = _opts(N, 1)
    assert lib.rome_conv_pose3pose3rotation(ctx.handle, C.byref(o), 2, None, mu.ctypes.data_as(C.POINTER(C.c_double)),
                                            np.zeros((2, 3, 3)).ctypes.data_as(C.POINTER(C.c_double)),
                                            fixed.ctypes.data_as(C.POINTER(C.c_double)), None,
                                            target.copy().ctypes.data_as(C.POINTER(C.c_double)), None) == _lib.ERR_NOT_POSDEF
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")
    out = torch.zeros((2, 6, N), dtype=torch.float64, device="cuda:0")
    st = torch.full((2, N), -1, dtype=torch.int32, device="cuda:0")
    keep = [t(mu), t(np.zeros((2, 6))), t(fixed), t(target), t(dirs, torch.int32)]
    cd = _lib.ConvDev()
    cd.n_conv = 2
    cd.mu, cd.L, cd.bel_fixed, cd.bel_target, cd.dir = (k.data_ptr() for k in keep)
    cd.out, cd.status = out.data_ptr(), st.data_ptr()
    torch.cuda.synchronize()
    _lib.check(lib.rome_conv_pose3pose3rotation_dev(ctx.handle, C.byref(o), C.byref(cd)), ctx.handle)
    ctx.synchronize()
    out, st = out.cpu().numpy(), st.cpu().numpy()
    assert st[0].all() and not st[1].any()
    z = np.repeat(mu[:, None, :], N, axis=1)
    mp = np.stack([r3.mp_root(int(dirs[c]), z[c], fixed[c].T) for c in range(2)])
    table = r3.Table(mp.reshape(-1, 3), np.stack([r3.np_root(int(dirs[c]), z[c], fixed[c].T) for c in range(2)]).reshape(-1, 3))
    dev, bound = table.check(out[:, 3:].transpose(0, 2, 1).reshape(-1, 3))
    print("zero covariance: %.3e of %.3e" % (dev, bound))
    assert dev <= bound and np.array_equal(out[:, :3], target[:, :3])


# ------------------------------------------------------------------ 3. GAUSS_NEWTON
@pytest.mark.parametrize("N", [64, 100, 256, 512, 513])
def test_gauss_newton_from_far_starts(N):
    """starts up to 3 rad from the root: the same root within the bound, status 0 (rows 0 and 1 of the root case; the given-noise table)"""
    mu, cov, fixed, target, ref, rst, noise, sub, table = _root_case(N, True)
    rng = np.random.default_rng(4000 + N)
    start = np.array(target[:2])
    delta = _unit(rng, (2, N)) * rng.uniform(0.0, 3.0, (2, N, 1))
    for c in range(2):                                                   # the root rotation times Exp(delta)
        start[c, 3:] = r3.np_root(0, delta[c], ref[c].T).T
    o, _ = _opts(N, 3)
    out, st = R.conv_pose3pose3rotation(o, mu[:2], cov[:2], fixed[:2], start, dirs=DIRS[:2], noise=noise[:2], want_status=True)
    d, bound, dn, boundn = _check_roots(out, ref, sub, table, rows=slice(0, 2))
    print("Gauss-Newton N %d: mp %.3e of %.3e, restatement %.3e of %.3e" % (N, d, bound, dn, boundn))
    assert d <= bound and dn <= boundn and not st.any()
    assert np.array_equal(out[:, :3], start[:, :3])


def test_gauss_newton_one_iteration_from_a_far_start():
    """max_iters = 1: the one iterate tests the functor at the start and fails: status 1, a finite result"""
    N = 100
    mu, cov, fixed, target, ref, rst, noise, sub, table = _root_case(N, True)
    rng = np.random.default_rng(4100)
    start = np.array(target[:2])
    delta = _unit(rng, (2, N)) * rng.uniform(1.0, 3.0, (2, N, 1))
    for c in range(2):
        start[c, 3:] = r3.np_root(0, delta[c], ref[c].T).T
    o, _ = _opts(N, 3, max_iters=1)
    out, st = R.conv_pose3pose3rotation(o, mu[:2], cov[:2], fixed[:2], start, dirs=DIRS[:2], noise=noise[:2], want_status=True)
    assert st.all() and np.isfinite(out).all() and np.array_equal(out[:, :3], start[:, :3])


# ------------------------------------------------------------------ 4. Nelder-Mead
NM_SHARE_FLOOR = 0.97          # the floor the project asserts for P3XYY


def nm_inputs():
    """C = 4, N = 100, belief-shaped: the fixed poses a belief around one pose (sd 0.5 m / 0.05 rad), the targets within a few sigma of the
    root (sd 0.05 rad around the root rotation of the mean measurement), as DESIGN §12c explains a minimiser over inflated starts needs"""
    rng = np.random.default_rng(51)
    C_, N = 4, 100
    dirs = [0, 1, 1, 0]
    mu = _unit(rng, (C_,)) * rng.uniform(0.2, 1.5, (C_, 1))
    cov = np.stack([(0.02 ** 2) * np.eye(3)] * C_)
    sd = np.array([0.5] * 3 + [0.05] * 3)[None, :, None]
    fixed = _poses(rng, C_, 1, 0.4) + rng.standard_normal((C_, 6, N)) * sd
    centre = np.stack([r3.np_root(dirs[c], mu[c], fixed[c].mean(axis=1)) for c in range(C_)])
    target = np.concatenate([rng.uniform(-40, 40, (C_, 3, 1)) + np.zeros((C_, 3, N)), centre[:, :, None] + np.zeros((C_, 3, N))], axis=1)
    target = target + rng.standard_normal((C_, 6, N)) * sd
    noise = rng.standard_normal((C_, 3, N))
    return dirs, mu, cov, fixed, target, noise


def nm_restatement(inflate_cycles=3, inflation=5.0):
    dirs, mu, cov, fixed, target, noise = nm_inputs()
    oo = ro.make_opts(N=100, solver=0, seed=SEED, stream_offset=SOFF, inflate_cycles=inflate_cycles, inflation=inflation)
    return r3.rot_conv(oo, dirs, mu, cov, fixed, target, r3.NELDER_MEAD, noise=noise)


def test_nelder_mead_vs_restatement():
    """The share of particles within 1e-6 of the restatement (ro.nelder_mead on a cost of ro.so3_exp / ro.so3_log) is printed and must
    reach the floor.  Measured on the CPU beforehand: the restatement alone converges on these inputs."""
    dirs, mu, cov, fixed, target, noise = nm_inputs()
    o, _ = _opts(100, 2)
    out, st = R.conv_pose3pose3rotation(o, mu, cov, fixed, target, dirs=dirs, noise=noise, want_status=True)
    ref, rst, z = nm_restatement(o.inflate_cycles, o.inflation)
    d = np.abs(out[:, 3:] - ref[:, 3:]).max(axis=1)
    own = np.stack([np.abs(R.residual_pose3pose3rotation(z[c], *((fixed[c].T, out[c].T) if dirs[c] == 0 else (out[c].T, fixed[c].T)))).max(axis=1)
                    for c in range(4)])
    share = float((d <= 1e-6).mean())
    print("Nelder-Mead: median |d| %.3e, p99 own |r| %.3e, share within 1e-6 %.4f, status set on %d / %d" %
          (np.median(d), np.quantile(own, 0.99), share, int(st.sum()), int(rst.sum())))
    assert share >= NM_SHARE_FLOOR
    assert np.array_equal(out[:, :3], target[:, :3])


# ------------------------------------------------------------------ 5. options, layouts, errors
def test_nullhypo_rows():
    """null particles keep all six coordinates up to the additive entropy spread_nh * std * (u - 1/2) on coordinates 3, 4, 5 only.  The
    spread is a sum over N = 100 particles formed in another order on the device: N * 64 ulp of an entropy below 2, 1e-12 to be safe."""
    N = 100
    rng = np.random.default_rng(71)
    mu = np.array([[0.3, -0.2, 0.5], [-0.7, 0.1, 0.4]])
    cov = np.stack([(0.02 ** 2) * np.eye(3)] * 2)
    sd = np.array([0.5] * 3 + [0.05] * 3)[None, :, None]
    fixed = _poses(rng, 2, 1, 0.4) + rng.standard_normal((2, 6, N)) * sd
    target = _poses(rng, 2, 1, 0.4) + rng.standard_normal((2, 6, N)) * sd
    o, oo = _opts(N, 1)
    out, st = R.conv_pose3pose3rotation(o, mu, cov, fixed, target, dirs=[0, 1], want_status=True, nullhypo=0.5)
    ref, rst, z = r3.rot_conv(oo, [0, 1], mu, cov, fixed, target, r3.NEWTON, nullhypo=0.5, spread_nh=o.spread_nh)
    assert np.array_equal(out[:, :3], target[:, :3])                              # every particle, null or not
    on = np.stack([np.abs(r3.np_residual(z[c], *((fixed[c].T, out[c].T) if c == 0 else (out[c].T, fixed[c].T)))).max(axis=1) for c in range(2)]) <= 1e-12
    assert 0.3 < on.mean() < 0.7 and np.array_equal(st != 0, np.zeros_like(on))  # about half of the particles are on the constraint
    d = np.abs(out[:, 3:] - ref[:, 3:]).max(axis=1)
    print("nullhypo: on-constraint max |d| %.3e, null particles max |d| %.3e" % (d[on].max(), d[~on].max()))
    assert d[on].max() <= 64 * 2.0 ** -52 * math.pi and d[~on].max() <= 1e-12
    moved = np.abs(out[:, 3:] - target[:, 3:]).min(axis=1)
    assert (moved[~on] > 0).all()                                                 # ... and the others moved on every rotation coordinate


def test_layouts_agree():
    N = 100
    mu, cov, fixed, target, ref, rst, noise, sub, table = _root_case(N, True)
    o, _ = _opts(N, 1)
    aos = lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))
    pts = lambda a: np.ascontiguousarray(R.getPoint(R.Pose3, aos(a)))
    soa = R.conv_pose3pose3rotation(o, mu, cov, fixed, target, dirs=DIRS, noise=noise)
    out = R.conv_pose3pose3rotation(o, mu, cov, aos(fixed), aos(target), dirs=DIRS, noise=aos(noise), layout=R.LAYOUT_AOS)
    assert np.array_equal(out, aos(soa))                                          # the same kernel on the same staged blocks
    # points: |w| <= 1 on the inputs and < 2.7 on the roots, where points -> coordinates (so3_log) is conditioned to 1e-15
    outp = R.conv_pose3pose3rotation(o, mu, cov, pts(fixed), pts(target), dirs=DIRS, noise=aos(noise), layout=R.LAYOUT_AOS_POINTS)
    assert np.abs(outp - pts(soa)).max() <= 1e-12
    assert np.array_equal(outp[:, :, :3], aos(target)[:, :, :3])


@pytest.mark.parametrize("N", [100, 700])
def test_dev_entry_equals_host_twin(N):
    import torch
    from rome_jl_amd import _lib
    lib, ctx = _lib.load(), R.default_context()
    rng = np.random.default_rng(75)
    C_ = 4
    dirs = np.array([0, 1, 1, 0], dtype=np.int32)
    mu = _unit(rng, (C_,)) * rng.uniform(0.2, 3.0, (C_, 1))
    cov = np.stack([(0.05 ** 2) * np.eye(3)] * C_)
    fixed, target = _poses(rng, C_, N, 1.0), _poses(rng, C_, N, 1.0)
    t = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")
    for solver in (1, 3):
        o, _ = _opts(N, solver)
        host, hst = R.conv_pose3pose3rotation(o, mu, cov, fixed, target, dirs=dirs, want_status=True)
        out = torch.zeros((C_, 6, N), dtype=torch.float64, device="cuda:0")
        st = torch.zeros((C_, N), dtype=torch.int32, device="cuda:0")
        keep = [t(mu), t(R.cholesky_lower(cov)), t(fixed), t(target), t(dirs, torch.int32)]
        cd = _lib.ConvDev()
        cd.n_conv = C_
        cd.mu, cd.L, cd.bel_fixed, cd.bel_target, cd.dir = (k.data_ptr() for k in keep)
        cd.out, cd.status = out.data_ptr(), st.data_ptr()
        torch.cuda.synchronize()
        _lib.check(lib.rome_conv_pose3pose3rotation_dev(ctx.handle, C.byref(o), C.byref(cd)), ctx.handle)
        ctx.synchronize()
        assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(st.cpu().numpy(), hst)
    w = t(np.full(C_, 0.5)); alt = t(np.arange(C_), torch.int32)
    cd.hypo_w, cd.alt_var = w.data_ptr(), alt.data_ptr()
    assert lib.rome_conv_pose3pose3rotation_dev(ctx.handle, C.byref(o), C.byref(cd)) == _lib.ERR_INVALID_ARG     # a multihypo table


def test_argument_errors():
    from rome_jl_amd import _lib
    lib, ctx = _lib.load(), R.default_context()
    N = 16
    o, _ = _opts(N, 1)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    mu, cov = np.zeros((1, 3)), np.eye(3)[None].copy()
    fixed, target = np.zeros((1, 6, N)), np.zeros((1, 6, N))
    z, p, r = np.zeros((2, 3)), np.zeros((2, 6)), np.zeros((2, 3))
    E = _lib.ERR_INVALID_ARG
    conv = lib.rome_conv_pose3pose3rotation
    assert conv(ctx.handle, C.byref(o), 1, None, None, P(cov), P(fixed), None, P(target), None) == E
    assert conv(ctx.handle, C.byref(o), 1, None, P(mu), None, P(fixed), None, P(target), None) == E
    assert conv(ctx.handle, C.byref(o), 1, None, P(mu), P(cov), None, None, P(target), None) == E
    assert conv(ctx.handle, C.byref(o), 1, None, P(mu), P(cov), P(fixed), None, None, None) == E
    assert conv(None, C.byref(o), 1, None, P(mu), P(cov), P(fixed), None, P(target), None) == E
    assert conv(ctx.handle, C.byref(o), -1, None, P(mu), P(cov), P(fixed), None, P(target), None) == E
    bad = np.array([2], dtype=np.int32)
    assert conv(ctx.handle, C.byref(o), 1, bad.ctypes.data_as(C.POINTER(C.c_int32)), P(mu), P(cov), P(fixed), None, P(target), None) == E
    assert conv(ctx.handle, C.byref(o), 0, None, None, None, None, None, None, None) == _lib.OK      # C = 0 is OK
    for fn in (lib.rome_residual_pose3pose3rotation, lib.rome_residual_pose3pose3rotation_pt):
        assert fn(ctx.handle, 2, None, P(p), P(p), P(r)) == E and fn(ctx.handle, 2, P(z), P(p), P(p), None) == E
        assert fn(ctx.handle, 0, None, None, None, P(r)) == _lib.OK
    assert lib.rome_conv_pose3pose3rotation_dev(ctx.handle, C.byref(o), None) == E
    cd = _lib.ConvDev()
    cd.n_conv = 0
    assert lib.rome_conv_pose3pose3rotation_dev(ctx.handle, C.byref(o), C.byref(cd)) == _lib.OK
    cd.n_conv = 1                                                                 # rows without tables
    assert lib.rome_conv_pose3pose3rotation_dev(ctx.handle, C.byref(o), C.byref(cd)) == E
    with pytest.raises(R.RomeError):
        R.conv_pose3pose3rotation(o, mu, np.zeros((1, 3, 3)), fixed, target)      # a singular covariance


# ------------------------------------------------------------------ 6. solveGraph
PRIOR_COV = np.diag([0.1] * 3 + [0.01] * 3) ** 2
ROT_MU, ROT_COV = np.array([0.0, 0.0, 0.5]), np.diag([0.02] * 3) ** 2


def _graph(N, more=False):
    fg = R.initfg(N=N)
    fg.addVariable("x0", R.Pose3); fg.addVariable("x1", R.Pose3)
    fg.addFactor(["x0"], R.PriorPose3(R.MvNormal(np.zeros(6), PRIOR_COV)))
    fg.addFactor(["x0", "x1"], R.Pose3Pose3Rotation(R.MvNormal(ROT_MU, ROT_COV)))
    if more:
        fg.addFactor(["x0", "x1"], R.Pose3Pose3XYYaw(R.MvNormal([10.0, 0.0, 0.5], np.diag([0.1, 0.1, 0.01]) ** 2)))
        fg.addFactor(["x1"], R.PriorPose3ZRP(R.Normal(1.0, 0.1), R.MvNormal([0.0, 0.0], np.diag([0.01, 0.01]) ** 2)))
    start = np.array([3.0, -2.0, 1.0, 0.0, 0.0, 0.0])[:, None] + np.random.default_rng(9).standard_normal((6, N)) * 0.3
    fg.initVariable("x1", start)
    return fg, start


def _frechet_mean(w):
    """Karcher mean of rotation vectors w [N][3]"""
    from scipy.spatial.transform import Rotation as Rot
    rs = Rot.from_rotvec(w)
    m = rs[0]
    for _ in range(20):
        step = (m.inv() * rs).as_rotvec().mean(axis=0)
        m = m * Rot.from_rotvec(step)
        if np.linalg.norm(step) < 1e-14:
            break
    return m


def test_solve_graph_with_the_partial_aware_product():
    """x0 with a PriorPose3, x0 -> x1 a Pose3Pose3Rotation with mu = (0, 0, 0.5).  The rotation of x1 is R_x0 Exp(z): its covariance is the
    prior's rotation block plus the measurement's, so the Frechet mean of N particles has the standard error sqrt(trace / N) as a
    vector.  The mean lies within five of them of Exp(mu), and x1's translation samples are the ones it started with."""
    from scipy.spatial.transform import Rotation as Rot
    N = 100
    fg, start = _graph(N)
    dg = R.solveGraph(fg, seed=SEED, partial_product="coordinate")
    x1 = fg.getVal("x1")
    assert np.isfinite(x1).all() and np.isfinite(fg.getVal("x0")).all() and dg.has_partial3()
    se = math.sqrt((np.trace(PRIOR_COV[3:, 3:]) + np.trace(ROT_COV)) / N)
    err = np.linalg.norm((Rot.from_rotvec(ROT_MU).inv() * _frechet_mean(x1[3:].T)).as_rotvec())
    print("solveGraph: Frechet mean of x1 is %.4e from Exp(mu); standard error %.4e" % (err, se))
    assert err <= 5 * se
    assert np.array_equal(x1[:3], start[:3])
    assert np.abs(x1[3:] - start[3:]).max() > 0.1


def test_solve_graph_with_all_three_partial_families_and_with_the_product_off():
    N = 100
    fg, _ = _graph(N, more=True)
    R.solveGraph(fg, seed=SEED, partial_product="coordinate")
    assert all(np.isfinite(fg.getVal(l)).all() for l in fg.variables)
    fg, _ = _graph(N)
    R.solveGraph(fg, seed=SEED, partial_product="off")
    assert all(np.isfinite(fg.getVal(l)).all() for l in fg.variables)
    fg, _ = _graph(N, more=True)
    R.solveGraph(fg, seed=SEED, partial_product="off")
    assert all(np.isfinite(fg.getVal(l)).all() for l in fg.variables)
