"""Device math of rome.jl_amd/csrc/rome_device_math.hpp (fast_sincos, wrap_pi, fast_sqrt, fast_log, fast_exp_neg, fast_atan2, quaternion
Exp/Log) against numpy on 2e5 random arguments spanning the magnitudes the kernels see: compiled on the fly with hipcc."""
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_math_against_numpy(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    exe = str(tmp_path / "math_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "-o", exe,
                           os.path.join(ROOT, "tests", "hip", "math_check.hip")])
    rng = np.random.default_rng(0)
    n = 200000
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2.5, n)
    y = rng.standard_normal(n) * 10.0 ** rng.uniform(-6, 2.5, n)
    x[8:2008] = rng.uniform(-1e5, 1e5, 2000)                                         # sin/cos: headings far from the principal range
    x[:8] = [0.0, np.pi, -np.pi, 1e-300, 3.0 * np.pi, -0.0, 745.0, 1.0]
    y[:8] = [0.0, 0.0, 1e-300, 1.0, -2.0, 5.0, 1e-12, 1.0]
    np.concatenate([x, y]).tofile(str(tmp_path / "in.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert out.returncode == 0 and "math_check ok" in out.stdout, out.stdout + out.stderr
    o = np.fromfile(str(tmp_path / "out.bin")).reshape(9, n)
    assert np.abs(o[0] - np.sin(x)).max() < 5e-16 + 1e-18 * np.abs(x).max() and np.abs(o[1] - np.cos(x)).max() < 5e-16 + 1e-18 * np.abs(x).max()
    w = np.arctan2(np.sin(x), np.cos(x))
    dw = np.abs(o[2] - w); dw = np.minimum(dw, np.abs(dw - 2 * np.pi))            # the ±π tie may land on either end
    assert dw.max() < 1e-13 and np.abs(o[2]).max() <= np.pi + 1e-15
    assert np.abs(o[3] - np.sqrt(np.abs(x))).max() <= 2e-16 * np.sqrt(np.abs(x)).max() and (np.abs(o[3] / np.maximum(np.sqrt(np.abs(x)), 1e-300) - 1.0)[np.abs(x) > 1e-290] < 4e-16).all()
    ref = np.log(np.abs(y) + 1e-300)
    assert (np.abs(o[4] - ref) <= 4e-16 * np.maximum(1.0, np.abs(ref))).all()
    ref = np.exp(-np.abs(x))
    assert (np.abs(o[5] - ref) <= 5e-16 * ref + 1e-320).all()
    ref = np.arctan2(y, x)
    keep = ~((x == 0) & (y == 0)) & ~(np.signbit(x) & (x == 0))                     # atan2(±0, -0) conventions are not reproduced
    assert np.abs(o[6] - ref)[keep].max() < 7e-16
    wn = 0.01 * np.sqrt(x * x + y * y + (x - y) ** 2)                               # |ω| of the quaternion round trip
    assert np.abs(o[7])[wn < 3.0].max() < 2e-15 and np.abs(o[8]).max() < 1e-15      # Log(Exp(ω)) = ω below π; unit norm always


# ---------------------------------------------------------------------------------------------------------------------------------
# The quaternion functions in full (k_quat of tests/hip/math_check.hip): quat_exp, quat_log∘quat_exp, quat_mul / quat_cmul / quat_mulc,
# quat_rot, and so3_exp / so3_log for comparison, on the SE(3) angle edges of tests/conv_ref.py and 2e4 random rotation vectors,
# against mpmath (the edges and 200 random points) and the float64 NumPy quaternion restatement of conv_ref (all points).
#
# Bounds, measured on the CPU (quat_reference; nothing from a GPU run): per block, dev = the largest deviation of the float64
# restatement from mp relative to the block's scale, bound = max(8·dev, 64 ulp) x scale.  Scales: 1 for the unit quaternions and
# the rotation matrix; max(1, |v|) for quat_rot; |ω| for the Log round trip below 1e-4 (RELATIVE there), max(1, |ω|) above.  Measured
# dev, in eps: exp 0.9, log 0.6, mul 1.3, cmul 0.9, mulc 1.0, rot 2.0, so3_exp 3.1 -- every bound is the 64 ulp floor.
# Snap zone (the reference's 2 q_w² <= √eps: the edges π − 1e-4 and π − 1e-6): |‖ω_out‖ − π| <= 4 ulp, axis = ±ω/‖ω‖ within the bound.
# so3_log∘so3_exp is compared for 1e-4 <= θ <= 3 only, at 16·eps·θ/sin²θ + 64 ulp -- the ONE bound here that is argued, not measured: cos θ = (tr R − 1)/2 carries about 5 eps from the
# rounded Rodrigues entries, which sqrt(1 − c²)/acos(c) turns into 5·eps·θ/sin²θ on the vector (cf. lin_ref.log_formula_error).
# ---------------------------------------------------------------------------------------------------------------------------------
QUAT_BLOCKS = {"exp": (0, 4), "log": (4, 7), "mul": (7, 11), "cmul": (11, 15), "mulc": (15, 19), "rot": (19, 22), "so3_exp": (22, 31)}


def quat_points():
    import conv_ref as CR
    rng = np.random.default_rng(11)
    axes = np.concatenate([np.eye(3), -np.eye(3)[:1], CR._unit(rng, (4,))])
    w1e = np.array([m * a for m in CR.P3_MAGS for a in axes])
    w2e = CR._unit(rng, (len(w1e),)) * rng.uniform(0, 3, (len(w1e), 1))
    w2e[::4] = w1e[::4] * 0.5                                                       # products on one axis
    n = 20000
    w1r = CR._unit(rng, (n,)) * 10.0 ** rng.uniform(-10, np.log10(3.0), (n, 1))
    w2r = CR._unit(rng, (n,)) * 10.0 ** rng.uniform(-6, np.log10(3.0), (n, 1))
    return np.concatenate([w1e, w1r]), np.concatenate([w2e, w2r]), len(w1e)


def _principal(w):
    """Log(Exp(ω)) for |ω| < 2π, in closed form: ω itself up to π, ω·(1 − 2π/|ω|) beyond"""
    n = np.sqrt((w * w).sum(-1, keepdims=True))
    return np.where(n > np.pi, w * (1.0 - 2.0 * np.pi / np.where(n > 0, n, 1.0)), w)


def quat_reference():
    """-> w1, w2, float64 blocks (m, width), mp subset indices, mp blocks, per-block scale (m,), dev, relative bound, zone mask"""
    import mpmath as mpm
    import conv_ref as CR
    import lin_ref as L
    w1, w2, n_edge = quat_points()
    m = len(w1)
    a, b = CR.q_exp(w1), CR.q_exp(w2)
    f64 = {"exp": a, "log": _principal(w1), "mul": CR.q_mul(a, b), "cmul": CR.q_mul(CR.q_conj(a), b), "mulc": CR.q_mul(a, CR.q_conj(b)),
           "rot": CR.q_rot(a, w2), "so3_exp": np.swapaxes(L._np_so3_exp(w1), 1, 2).reshape(m, 9)}          # column-major
    n1, n2 = np.sqrt((w1 * w1).sum(-1)), np.sqrt((w2 * w2).sum(-1))
    npr = np.sqrt((f64["log"] ** 2).sum(-1))
    one = np.ones(m)
    scale = {"exp": one, "mul": one, "cmul": one, "mulc": one, "so3_exp": one, "rot": np.maximum(1.0, n2),
             "log": np.where(npr < 1e-4, npr, np.maximum(1.0, npr))}
    sub = sorted(set(range(n_edge)) | set(np.random.default_rng(12).integers(n_edge, m, 200).tolist()))

    def qexp(w):
        th = mpm.sqrt(sum(v * v for v in w))
        if th == 0:
            return [mpm.mpf(1), mpm.mpf(0), mpm.mpf(0), mpm.mpf(0)]
        k = mpm.sin(th / 2) / th
        return [mpm.cos(th / 2)] + [k * v for v in w]

    def qmul(p, q):
        return [p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1], p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]]

    def conj(q):
        return [q[0], -q[1], -q[2], -q[3]]
    mp = {k: np.empty((len(sub), hi - lo)) for k, (lo, hi) in QUAT_BLOCKS.items()}
    dev = {k: 0.0 for k in QUAT_BLOCKS}
    with mpm.workdps(L.DPS):
        for r, i in enumerate(sub):
            u1 = [mpm.mpf(float(v)) for v in w1[i]]; u2 = [mpm.mpf(float(v)) for v in w2[i]]
            qa, qb = qexp(u1), qexp(u2)
            R = L._so3_exp(u1)
            th = mpm.sqrt(sum(v * v for v in u1))
            lg = u1 if th <= mpm.pi else [v * (1 - 2 * mpm.pi / th) for v in u1]
            vals = {"exp": qa, "log": lg, "mul": qmul(qa, qb), "cmul": qmul(conj(qa), qb), "mulc": qmul(qa, conj(qb)),
                    "rot": L._mv(R, u2), "so3_exp": [R[i_][j_] for j_ in range(3) for i_ in range(3)]}
            for k, v in vals.items():
                mp[k][r] = [float(x) for x in v]
                err = max(abs(mpm.mpf(float(f64[k][i, j])) - v[j]) for j in range(len(v)))
                if scale[k][i] > 0:
                    dev[k] = max(dev[k], float(err) / scale[k][i])
    eps = 2.0 ** -52
    bound = {k: max(8.0 * d, 64.0 * eps) for k, d in dev.items()}
    zone = 2.0 * a[:, 0] ** 2 <= CR.SQRT_EPS
    return w1, w2, f64, sub, mp, scale, dev, bound, zone, n1


def test_quaternion_functions_against_mp_and_numpy(tmp_path):
    import conv_ref as CR
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "math_check")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed", "-o", exe,
                           os.path.join(ROOT, "tests", "hip", "math_check.hip")])
    w1, w2, f64, sub, mp, scale, dev, bound, zone, n1 = quat_reference()
    m = len(w1)
    eps = 2.0 ** -52
    assert all(b == 64.0 * eps for b in bound.values()), dev                          # the figures of the header comment
    assert zone.sum() == 16 and zone.mean() < 0.05 and (np.abs(np.abs(np.pi - n1) - CR.ZONE_EDGE) >= CR.ZONE_MARGIN).all()
    np.zeros(512).tofile(str(tmp_path / "in.bin"))
    np.concatenate([w1.T.reshape(-1), w2.T.reshape(-1)]).tofile(str(tmp_path / "qin.bin"))
    out = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(tmp_path / "qin.bin"), str(tmp_path / "qout.bin")],
                         capture_output=True, text=True)
    assert out.returncode == 0 and "math_check quat ok %d" % m in out.stdout, out.stdout + out.stderr
    o = np.fromfile(str(tmp_path / "qout.bin")).reshape(34, m).T
    assert np.isfinite(o).all()
    for k, (lo, hi) in QUAT_BLOCKS.items():
        got = o[:, lo:hi]
        keep = ~zone if k == "log" else np.ones(m, bool)
        lim = bound[k] * scale[k][:, None]
        d64 = np.abs(got - f64[k])
        dmp = np.abs(got[sub] - mp[k])
        ok_zero = (scale[k] == 0)[:, None] & (got == f64[k])                          # ω = 0 exactly: Log(Exp(0)) = 0 exactly
        print("QUAT gpu %s dev %.2f eps, kernel vs float64 %.2f vs mp %.2f (in units of the bound)"
              % (k, dev[k] / eps, np.where(keep[:, None] & ~ok_zero, d64 / np.where(lim > 0, lim, 1.0), 0).max(),
                 np.where((keep[:, None] & ~ok_zero)[sub], dmp / np.where(lim > 0, lim, 1.0)[sub], 0).max()))
        assert ((d64 <= lim) | ok_zero | ~keep[:, None]).all(), (k, np.argwhere(~((d64 <= lim) | ok_zero | ~keep[:, None]))[:4].tolist())
        assert ((dmp <= lim[sub]) | ok_zero[sub] | ~keep[sub][:, None]).all(), k
    # snap zone: θ = π exactly, the axis that of ω
    wz = o[zone, 4:7]
    nz = np.sqrt((wz * wz).sum(-1))
    assert (np.abs(nz - np.pi) <= 4 * CR.ULP_PI).all()
    ax = w1[zone] / n1[zone, None]
    da = np.minimum(np.abs(wz / nz[:, None] - ax).max(-1), np.abs(wz / nz[:, None] + ax).max(-1))
    assert (da <= bound["log"]).all()
    # so3_log(so3_exp(ω)), for comparison, away from both ends
    mid = (n1 >= 1e-4) & (n1 <= 3.0)
    lim = 16.0 * eps * n1[mid] / np.sin(n1[mid]) ** 2 + 64.0 * eps
    assert (np.abs(o[mid, 31:34] - w1[mid]).max(-1) <= lim).all()
