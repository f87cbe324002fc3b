"""References for belief evaluation (k_kde_eval<M>: Flat<2>, Flat<3>, Se3M of rome.jl_amd/csrc/rome_product.hip): what rome_kde_eval /
rome_kde_eval_dev must return.

Definition (include/rome_mi355.h), for a belief of N particles y_j, bandwidths h[dim] and a query x:
    q_j     = Σ_k (d_k(x, y_j) / h_k)²
    logp(x) = −½ q_min + log Σ_j exp(−½ (q_j − q_min)) − log N' − Σ_k log h_k − (dim/2) log 2π
d is the tangent difference of the variable type: x − y (Point2), heading difference wrapped (Pose2), (t_x − t_y, Log(R_yᵀ R_x)) (Pose3,
coordinates (t, rotation vector)).  N' = N; with leave-one-out (self-evaluation only) j = i is skipped and N' = N − 1.

Two sides, neither of which is the kernel:
  * mp_diffs / mp_logpdf -- mpmath at DPS digits, written from the definition.  SO(3) through rotation MATRICES (tests/lin_ref.py's
                            _so3_exp and _so3_log: the angle by atan2(‖skew part‖, trace part)), the heading wrap by atan2(sin, cos).  The
                            tangent differences of a table are formed once and serve every bandwidth.  At most 12 queries per case.
  * np_logpdf            -- float64 NumPy, vectorised over (query, particle), rotations through conv_ref's quaternion helpers, the
                            logarithm of the sum by subtracting the maximum.  Serves every query.

Bound for the device, all from the reference side (never from a GPU run), per case:
    |logp_gpu − logp_mp| <= max(8·dev_np, 64 ulp) · max(1, |logp_mp|)          on the mp rows
    |logp_gpu − logp_np| <= (max(8·dev_np, 64 ulp) + dev_np) · max(1, |logp_np|)   on the others
with dev_np = max over the case's mp rows of |logp_np − logp_mp| / max(1, |logp_mp|).  The factor 8 and the floor are those of
tests/lin_ref.py and tests/mmd_ref.py: the kernel sums in another order, multiplies by 1/h and its fast_exp_neg is good to 2 ulp.
dev_np is at most 6.2 eps over every case (tests/test_kde_eval_host.py holds 8·dev_np under the floor), so the floor decides everywhere.

Cases (name -> belief, bandwidths, queries, mp rows; `cases()`): per dim and per (N, Q) of SHAPES four rows, each with h = 0.3 on every
coordinate ("h03") and with an anisotropic h from 1e-3 to 10 ("aniso"):
  ordinary   unit-spread cloud (Pose2 headings over the whole circle); the first queries are particles themselves, the rest random
  edges      Pose2: particle headings within 0.03 below +π, query headings within 0.03 above −π (every difference wraps); Pose3: query
             rotations = particle rotations turned by π − 6e-4 (relative rotations in (π − 1e-3, π − 2.5e-4), clear of the zone within
             1.7e-4 of π where the library's Log snaps to π as Manifolds.jl's does); query 0 EQUALS particle 0
  identical  all particles identical; query 0 equals them
  far        the queries are the ordinary cloud moved 40 along x: at h_x = 1e-3 logp ≈ −8e8, and at 0.3 exp(−½q) is 0 in float64
plus leave-one-out self-evaluations ("loo"), the two-cluster sets of kde_mode ("mode") and the pairs of kld ("kld").
The mp values are stored (tests/golden/kde_eval_reference.json, written by `python tests/kde_eval_ref.py`, 30 digits) with a digest of
the inputs they belong to, so that the GPU tests do not wait for mpmath; tests/test_kde_eval_host.py recomputes every one of them.
Measured figures: profiles/kde_eval_reference_errors.md (printed by tests/test_kde_eval_host.py -s and tests/test_gpu_kde_eval.py -s).
"""
import functools
import hashlib
import json
import math
import os

import mpmath as mpm
import numpy as np

from conv_ref import q_conj, q_exp, q_log, q_mul
from lin_ref import _mm, _mt, _so3_exp, _so3_log

DPS = 40
EPS = 2.0 ** -52
ULP64 = 64.0 * EPS
DIMS = (2, 3, 6)
SEED = 0x4B4445
SHAPES = ((1, 1), (1, 3), (2, 2), (63, 65), (64, 64), (65, 257), (100, 256), (512, 300))
LOO_N = (2, 64, 65, 100)
ROWS = ("ordinary", "edges", "identical", "far")
H03 = {d: (0.3,) * d for d in DIMS}
ANISO = {2: (1e-3, 10.0), 3: (1e-3, 10.0, 0.1), 6: (1e-3, 0.1, 10.0, 0.05, 1.0, 0.01)}
BANDWIDTHS = (("h03", H03), ("aniso", ANISO))
NEAR_PI = math.pi - 6e-4
MP_QUERIES = 12
MP_QUERIES_BIG = 4          # at N = 512
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLD, "kde_eval_reference.json")
DIGITS = 30
LOG_2PI = 1.8378770664093453


# ------------------------------------------------------------------------------------------------------------ float64 side
def _remainder(x):
    k = np.rint(x / (2.0 * math.pi))
    return (x - k * 6.283185307179586) - k * 2.4492935982947064e-16


def np_diffs(dim, bel, pts):
    """bel (dim, N), pts (dim, Q) -> d(x_i, y_j) as (Q, N, dim)"""
    X, Y = np.ascontiguousarray(pts.T, dtype=np.float64), np.ascontiguousarray(bel.T, dtype=np.float64)
    d = X[:, None, :] - Y[None, :, :]
    if dim == 3:
        d[:, :, 2] = _remainder(d[:, :, 2])
    elif dim == 6:
        d[:, :, 3:] = q_log(q_mul(q_conj(q_exp(Y[:, 3:]))[None, :, :], q_exp(X[:, 3:])[:, None, :]))
    return d


def np_logpdf(dim, bel, h, pts=None, leave_one_out=False):
    """float64 restatement -> (Q,); pts None: the belief's own particles"""
    h = np.asarray(h, dtype=np.float64)
    n = bel.shape[1]
    q = np.sum((np_diffs(dim, bel, bel if pts is None else pts) / h[None, None, :]) ** 2, axis=2)
    if leave_one_out:
        assert pts is None and n >= 2
        q[np.arange(n), np.arange(n)] = np.inf
        n -= 1
    m = q.min(axis=1)
    lse = -0.5 * m + np.log(np.sum(np.exp(-0.5 * (q - m[:, None])), axis=1))
    return lse - math.log(n) - float(np.sum(np.log(h))) - 0.5 * dim * LOG_2PI


# ------------------------------------------------------------------------------------------------------------ mpmath side
def _f(v):
    return mpm.mpf(float(v))


def _mp_elem(dim, x):
    x = [_f(v) for v in x]
    return x if dim < 6 else (x[:3], _so3_exp(x[3:]))


def _mp_diff(dim, x, y):
    if dim == 2:
        return (x[0] - y[0], x[1] - y[1])
    if dim == 3:
        e = x[2] - y[2]
        return (x[0] - y[0], x[1] - y[1], mpm.atan2(mpm.sin(e), mpm.cos(e)))
    w = _so3_log(_mm(_mt(y[1]), x[1]))
    return (x[0][0] - y[0][0], x[0][1] - y[0][1], x[0][2] - y[0][2], w[0], w[1], w[2])


def mp_diffs(dim, bel, pts, idx):
    """squared tangent differences d_k(x_i, y_j)² for the queries i in idx -> [len(idx)][N] tuples of mp numbers"""
    with mpm.workdps(DPS):
        ys = [_mp_elem(dim, bel[:, j]) for j in range(bel.shape[1])]
        out = []
        for i in idx:
            x = _mp_elem(dim, pts[:, i])
            out.append([tuple(c * c for c in _mp_diff(dim, x, y)) for y in ys])
        return out


def mp_logpdf(dim, d2, h, idx=None, leave_one_out=False):
    """d2: mp_diffs(...) -> mp log-densities of those queries, straight from the definition (the sum of exponentials about the smallest
    q, so that it is a sum of numbers <= 1 at any distance).  leave_one_out: query idx[r] skips particle idx[r]."""
    with mpm.workdps(DPS):
        ih2 = [1 / (_f(v) * _f(v)) for v in h]
        lnh = sum(mpm.log(_f(v)) for v in h)
        out = []
        for r, row in enumerate(d2):
            q = [sum(a * b for a, b in zip(ih2, t)) for t in row]
            if leave_one_out:
                del q[idx[r]]
            qm = min(q)
            out.append(-qm / 2 + mpm.log(mpm.fsum(mpm.exp(-(v - qm) / 2) for v in q)) - mpm.log(len(q)) - lnh - mpm.mpf(dim) / 2 * mpm.log(2 * mpm.pi))
        return out


# ------------------------------------------------------------------------------------------------------------ tables
def _compose(w, d):
    """rotation vectors of Exp(w)·Exp(d), rows"""
    return q_log(q_mul(q_exp(w), q_exp(d)))


def _cloud(rng, dim, n):
    x = rng.standard_normal((dim, n))
    if dim == 3:
        x[2] = rng.uniform(-math.pi, math.pi, n)
    if dim == 6:
        x[3:] *= 0.5
    return x


def table(dim, row, N, Q):
    """-> bel (dim, N), pts (dim, Q): one row of the module docstring, from a seed"""
    rng = np.random.default_rng([SEED, dim, ROWS.index(row), N, Q])
    bel, pts = _cloud(rng, dim, N), _cloud(rng, dim, Q)
    k = min(N, (Q + 1) // 2)
    if row == "ordinary":
        pts[:, :k] = bel[:, :k]                           # the particles themselves, then random points
    elif row == "edges":
        if dim == 3:
            bel[2], pts[2] = math.pi - rng.uniform(0.0, 0.03, N), -math.pi + rng.uniform(0.0, 0.03, Q)
        if dim == 6:
            w0, axis = np.array([0.4, -0.7, 0.2]), np.array([2.0, -1.0, 2.0]) / 3.0
            bel[3:] = _compose(np.tile(w0, (N, 1)), 3e-5 * rng.standard_normal((N, 3))).T
            pts[3:] = _compose(_compose(np.tile(w0, (Q, 1)), np.tile(NEAR_PI * axis, (Q, 1))), 3e-5 * rng.standard_normal((Q, 3))).T
        pts[:, 0] = bel[:, 0]
    elif row == "identical":
        bel[:] = bel[:, :1]
        pts[:, 0] = bel[:, 0]
    elif row == "far":
        pts = bel[:, rng.integers(0, N, Q)].copy()
        pts[0] += 40.0
    return bel, pts


def mp_rows(N, Q):
    """the queries of a case that get an mp value: spread over the block, first and last included"""
    k = min(Q, MP_QUERIES_BIG if N > 100 else MP_QUERIES)
    return sorted(set(int(v) for v in np.rint(np.linspace(0, Q - 1, k))))


def two_clusters(dim, n_heavy=60, n_light=40):
    """kde_mode's set: a heavy cluster at the origin and a light one 6 away, interleaved in particle order; h = 0.3"""
    rng = np.random.default_rng([SEED, dim, 77])
    n = n_heavy + n_light
    x = 0.5 * rng.standard_normal((dim, n))
    light = np.zeros(n, dtype=bool)
    light[rng.permutation(n)[:n_light]] = True
    x[0, light] += 6.0
    if dim == 3:
        x[2, light] += 2.0
    return x, light


def kld_pair(dim, na=24, nb=30):
    rng = np.random.default_rng([SEED, dim, 99])
    a, b = _cloud(rng, dim, na), _cloud(rng, dim, nb)
    b[0] += 0.5
    return a, b


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(dim, bel, pts (None: self-evaluation), loo, idx, bws: ((tag, h), ...)); arrays read-only"""
    out = {}

    def add(name, dim, bel, pts, loo, idx, bws):
        for a in (bel, pts):
            if a is not None:
                a.setflags(write=False)
        out[name] = dict(dim=dim, bel=bel, pts=pts, loo=loo, idx=list(idx), bws=tuple(bws))
    for dim in DIMS:
        both = tuple((tag, hs[dim]) for tag, hs in BANDWIDTHS)
        for N, Q in SHAPES:
            for row in ROWS:
                bel, pts = table(dim, row, N, Q)
                add("eval/%d/%s/%d/%d" % (dim, row, N, Q), dim, bel, pts, False, mp_rows(N, Q), both)
        for N in LOO_N:
            bel, _ = table(dim, "ordinary", N, N)
            add("loo/%d/%d" % (dim, N), dim, bel.copy(), None, True, mp_rows(N, N), both)
        a, b = kld_pair(dim)
        add("kld_aa/%d" % dim, dim, a, None, False, range(a.shape[1]), both[:1])
        add("kld_ba/%d" % dim, dim, b, a.copy(), False, range(a.shape[1]), both[:1])
    for dim in (2, 3):
        x, _ = two_clusters(dim)
        add("mode/%d" % dim, dim, x, None, False, range(x.shape[1]), ((("h03", H03[dim]),)))
    return out


def digest(case):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(case["bel"]).tobytes())
    if case["pts"] is not None:
        h.update(np.ascontiguousarray(case["pts"]).tobytes())
    h.update(repr((case["loo"], case["idx"], case["bws"])).encode())
    return h.hexdigest()


def compute(name):
    """the mp side of one case, as it is stored: {"digest", tag: [strings]}"""
    c = cases()[name]
    pts = c["bel"] if c["pts"] is None else c["pts"]
    d2 = mp_diffs(c["dim"], c["bel"], pts, c["idx"])
    rec = {"digest": digest(c)}
    with mpm.workdps(DPS):
        for tag, h in c["bws"]:
            rec[tag] = [mpm.nstr(v, DIGITS) for v in mp_logpdf(c["dim"], d2, h, c["idx"], c["loo"])]
    return rec


@functools.lru_cache(maxsize=None)
def _stored():
    with open(FIXTURE) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def reference(name, tag):
    """-> dict(idx, mp: [mp numbers], np: float64 restatement at EVERY query, dev_np, tol): the stored mp side, which must belong to these
    very inputs, next to the restatement; shared by every test and left unchanged"""
    c = cases()[name]
    rec = _stored()[name]
    assert rec["digest"] == digest(c), "tests/golden/kde_eval_reference.json was made for other inputs: run `python tests/kde_eval_ref.py`"
    h = dict(c["bws"])[tag]
    with mpm.workdps(DPS):
        mp = [mpm.mpf(s) for s in rec[tag]]
        npv = np_logpdf(c["dim"], c["bel"], h, c["pts"], c["loo"])
        npv.setflags(write=False)
        dev = max(float(abs(_f(npv[i]) - m) / max(1, abs(m))) for i, m in zip(c["idx"], mp))
    return dict(idx=c["idx"], mp=mp, np=npv, h=np.array(h), dev_np=dev, tol=max(8.0 * dev, ULP64))


def deviation(ref, got):
    """got (Q,) float64 -> (worst |Δ| / bound over the mp rows, over the other rows, whether every value is finite): the bounds of the
    module docstring"""
    got = np.asarray(got, dtype=np.float64)
    with mpm.workdps(DPS):
        wm = max(float(abs(_f(got[i]) - m) / (ref["tol"] * max(1, abs(m)))) for i, m in zip(ref["idx"], ref["mp"]))
    rest = np.setdiff1d(np.arange(got.shape[0]), ref["idx"])
    wn = 0.0
    if rest.size:
        wn = float(np.max(np.abs(got[rest] - ref["np"][rest]) / ((ref["tol"] + ref["dev_np"]) * np.maximum(1.0, np.abs(ref["np"][rest])))))
    return wm, wn, bool(np.isfinite(got).all())


if __name__ == "__main__":
    out = {}
    for name in cases():
        out[name] = compute(name)
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=0)
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")
