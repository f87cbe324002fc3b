"""References for mmd (k_mmd<M>: Flat<2>, Flat<3>, Se3M of rome.jl_amd/csrc/rome_product.hip): what rome_mmd / rome_mmd_dev must return.

Definition (include/rome_mi355.h): k(x, y) = exp(−σ Σ_c (s_c d_c(x, y))²), S_aa = Σ_{i,j} k(a_i, a_j) over ALL ordered pairs (i = j
included), S_ab, S_bb likewise, mmd = S_aa/Na² − 2 S_ab/(Na Nb) + S_bb/Nb².  d is the tangent difference of the variable type:
x − y (Point2), heading difference wrapped (Pose2), (t_x − t_y, Log(R_yᵀ R_x)) (Pose3, coordinates (t, rotation vector)).

Two sides, neither of which is the kernel:
  * mp_pairs / mp_sums -- mpmath at DPS digits.  The per-pair tangent differences are formed once per table row (rotations as mp unit
                          quaternions, the angle by atan2(‖v‖, |w|)) and kept, so every σ and every scale of that row costs one exp per pair.
                          Unordered pairs i < j are doubled and the diagonal is the exact count: k is exactly symmetric in exact arithmetic.
  * np_sums            -- float64 NumPy, written the plain way and NOT in the kernel's order: a Python loop over the points of the first
                          set, every ORDERED pair evaluated (the diagonal too), rotations through conv_ref's quaternion helpers.

Bounds, all from the reference side (never from a GPU run).  For one panel (aa, ab or bb) with mp sum S over T ordered pairs:
    |S_gpu − S| <= max(8·dev_np, 64 ulp)·S + T·2^-1022
  * dev_np = |S_np − S|/S of the restatement on that panel (the policy of tests/test_gpu_linearize.py: 8 x the double side's own
    deviation, floor 64 ulp).  dev_np is at most 3.4 eps on every panel, so the bound is the floor everywhere; the host test holds
    8·dev_np under it, so that a table cannot move a bound without failing there first.
    What the floor has to cover: every term is a <= 2 ulp exponential of a few-ulp argument, a thread adds at most ⌈T/256⌉ <= 79 positive
    terms (<= 40 ulp even if every rounding went one way), then 6 + 3 additions join the lanes and the waves.
  * T·2^-1022: a term below the normal range is flushed or loses its relative accuracy; fast_exp_neg returns 0 below exp(−750), the
    reference 10^-300 and less.  This decides the panels that underflow entirely (S_ab of row 2 at σ = 1): the device sum is 0, the mp
    sum is not.  On every other panel it is 1e-303 and less.
mmd itself: absolute, 4 x 64 ulp = 5.7e-14 (each normalised sum is <= 1, and they cancel).  No row needs more.

Tables: for every dim one FEATURES table of three rows at Na = Nb = 100, evaluated at CASES (σ = 1e-3, σ = 1, and σ = 1 with a
scale that has a zero entry), and the GOLDEN pair: the reference's own sample files (tests/golden/pose3pose3nh_X1ptst.csv, 100 points;
X2ptst.csv, 200 points), projected to (x, y) and (x, y, ω_z) for dim 2 and 3, at σ = 1e-3.
  row 0  ordinary: unit-spread clouds a fraction of a spread apart; Pose2 headings over the whole circle
  row 1  edges: Pose2 headings of A within 0.03 below +π and of B within 0.03 above −π (every ab difference wraps); Pose3 rotations of B
         = rotations of A turned by π − 6e-4 (every ab relative rotation lies in (π − 1e-3, π − 2.5e-4): past the 1e-3 the issue asks for
         and clear of the zone within acos(1 − √eps) = 1.7e-4 of π, where the library's Log snaps to π as Manifolds.jl's does);
         COINCIDENT points: B's first 10 points are A's, A's points 50..54 repeat its points 0..4
  row 2  far apart: B is A's cloud moved 40 along x: σ d² > 750 for every ab pair at σ = 1, so S_ab underflows to 0 on the device
The mp sums are stored (tests/golden/mmd_reference.json, written by `python tests/mmd_ref.py`, 30 digits) with a digest of the inputs
they belong to, so that the GPU tests do not spend a minute in mpmath; tests/test_mmd_ref_host.py recomputes every one of them.
Measured figures: profiles/mmd_reference_errors.md (printed by tests/test_mmd_ref_host.py -s).
"""
import functools
import hashlib
import json
import math
import os

import mpmath as mpm
import numpy as np

from conv_ref import q_conj, q_exp, q_log, q_mul

DPS = 40
EPS = 2.0 ** -52
ULP64 = 64.0 * EPS
TINY = 2.0 ** -1022
DIMS = (2, 3, 6)
SEED = 0x4D4D44
N_FEATURE = 100
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ZERO_SCALE = {2: (0.0, 1.5), 3: (1.0, 0.0, 0.5), 6: (1.0, 1.0, 0.0, 0.5, 1.0, 2.0)}
# (name, σ, scale): what every row of the FEATURES table is evaluated at
CASES = (("s1e-3", 1e-3, None), ("s1", 1.0, None), ("s1_zero_scale", 1.0, "zero"))
GOLDEN_CASES = (("s1e-3", 1e-3, None),)
ROW_NAMES = ("ordinary", "edges", "far")
NEAR_PI = math.pi - 6e-4


def case_scale(dim, scale):
    return None if scale is None else np.array(ZERO_SCALE[dim])


# ------------------------------------------------------------------------------------------------------------ float64 side
def _remainder(x):
    k = np.rint(x / (2.0 * math.pi))
    return (x - k * 6.283185307179586) - k * 2.4492935982947064e-16


def np_diff(dim, x, Y):
    """d(x, y_j) for one point x (dim,) against the points Y (n, dim) -> (n, dim)"""
    d = x[None, :] - Y
    if dim == 3:
        d[:, 2] = _remainder(d[:, 2])
    elif dim == 6:
        d[:, 3:] = q_log(q_mul(q_conj(q_exp(Y[:, 3:])), q_exp(x[None, 3:])))
    return d


def _np_panel(dim, X, Y, sigma, s):
    tot = 0.0
    for i in range(X.shape[0]):                      # every ordered pair, the diagonal included
        q = np.sum((np_diff(dim, X[i], Y) * s[None, :]) ** 2, axis=1)
        tot += float(np.sum(np.exp(-sigma * q)))
    return tot


def np_sums(dim, A, B, sigma=1e-3, scale=None):
    """A (dim, Na), B (dim, Nb) -> (S_aa, S_ab, S_bb, mmd) in float64"""
    s = np.ones(dim) if scale is None else np.asarray(scale, dtype=np.float64)
    X, Y = np.ascontiguousarray(A.T, dtype=np.float64), np.ascontiguousarray(B.T, dtype=np.float64)
    saa, sab, sbb = _np_panel(dim, X, X, sigma, s), _np_panel(dim, X, Y, sigma, s), _np_panel(dim, Y, Y, sigma, s)
    na, nb = X.shape[0], Y.shape[0]
    return saa, sab, sbb, saa / (na * na) - 2.0 * sab / (na * nb) + sbb / (nb * nb)


# ------------------------------------------------------------------------------------------------------------ mpmath side
def _f(v):
    return mpm.mpf(float(v))


def _mp_elem(dim, x):
    x = [_f(v) for v in x]
    if dim < 6:
        return x
    w = x[3:]
    th = mpm.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    k = mpm.sin(th / 2) / th if th != 0 else mpm.mpf(1) / 2
    return x[:3] + [mpm.cos(th / 2), k * w[0], k * w[1], k * w[2]]


def _mp_diff(dim, x, y):
    if dim == 2:
        return (x[0] - y[0], x[1] - y[1])
    if dim == 3:
        e = x[2] - y[2]
        return (x[0] - y[0], x[1] - y[1], e - 2 * mpm.pi * mpm.nint(e / (2 * mpm.pi)))
    a, b = y[3:], x[3:]                               # conj(q_y) ⊗ q_x
    w = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]
    v = (a[0] * b[1] - a[1] * b[0] - a[2] * b[3] + a[3] * b[2],
         a[0] * b[2] + a[1] * b[3] - a[2] * b[0] - a[3] * b[1],
         a[0] * b[3] - a[1] * b[2] + a[2] * b[1] - a[3] * b[0])
    n = mpm.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    k = 2 * mpm.atan2(n, abs(w)) / n if n != 0 else mpm.mpf(0)
    if w < 0:
        k = -k
    return (x[0] - y[0], x[1] - y[1], x[2] - y[2], k * v[0], k * v[1], k * v[2])


def mp_pairs(dim, A, B):
    """A (dim, Na), B (dim, Nb) -> per panel ("aa": pairs i < j, "ab": every (i, j), "bb": i < j) the squared tangent differences as mp
    tuples, and the set sizes "na", "nb" """
    with mpm.workdps(DPS):
        ea = [_mp_elem(dim, A[:, i]) for i in range(A.shape[1])]
        eb = [_mp_elem(dim, B[:, j]) for j in range(B.shape[1])]
        tri = lambda e: [_mp_diff(dim, e[i], e[j]) for i in range(len(e)) for j in range(i + 1, len(e))]
        out = {"na": len(ea), "nb": len(eb)}
        for key, diffs in (("aa", tri(ea)), ("ab", [_mp_diff(dim, x, y) for x in ea for y in eb]), ("bb", tri(eb))):
            out[key] = [tuple(c * c for c in d) for d in diffs]
        return out


def mp_sums(dim, pairs, sigma=1e-3, scale=None):
    """-> {"S": (S_aa, S_ab, S_bb), "mmd", "T": ordered pairs per panel}; S and mmd mp numbers"""
    with mpm.workdps(DPS):
        s2 = [_f(v) ** 2 for v in ([1.0] * dim if scale is None else scale)]
        sg = _f(sigma)
        S = []
        na, nb = pairs["na"], pairs["nb"]
        for key, mult, diag in (("aa", 2, na), ("ab", 1, 0), ("bb", 2, nb)):
            S.append(mult * mpm.fsum(mpm.exp(-sg * sum(a * b for a, b in zip(s2, d2))) for d2 in pairs[key]) + diag)
        val = S[0] / (na * na) - 2 * S[1] / (na * nb) + S[2] / (nb * nb)
        return {"S": tuple(S), "mmd": val, "T": (na * na, na * nb, nb * nb)}


def bounds(ref):
    """ref: mp_sums result -> (absolute bound per panel sum, absolute bound of mmd): the 64 ulp floor (8·dev_np stays under it on every
    row, held by tests/test_mmd_ref_host.py) plus the underflow term; 4 x the floor for mmd"""
    return tuple(ULP64 * float(s) + t * TINY for s, t in zip(ref["S"], ref["T"])), 4.0 * ULP64


def np_within_floor(ref, got):
    """the restatement's deviation per panel in eps, and whether 8 x it stays under the floor (underflowing panels: within T·2^-1022)"""
    with mpm.workdps(DPS):
        dev = [float(abs(_f(g) - s) / s) / EPS for g, s in zip(got[:3], ref["S"])]
        ok = [float(abs(_f(g) - s)) <= ULP64 / 8.0 * float(s) + t * TINY for g, s, t in zip(got[:3], ref["S"], ref["T"])]
    return dev, ok


# ------------------------------------------------------------------------------------------------------------ tables
@functools.lru_cache(maxsize=None)
def golden_files():
    X1 = np.loadtxt(os.path.join(GOLD, "pose3pose3nh_X1ptst.csv"), delimiter=",")
    X2 = np.loadtxt(os.path.join(GOLD, "pose3pose3nh_X2ptst.csv"), delimiter=",")
    assert X1.shape == (6, 100) and X2.shape == (6, 200)
    return X1, X2


def project(dim, X):
    return np.ascontiguousarray(X if dim == 6 else X[[0, 1, 5]] if dim == 3 else X[[0, 1]])


def _compose(w, d):
    """rotation vectors of Exp(w)·Exp(d), rows"""
    return q_log(q_mul(q_exp(w), q_exp(d)))


@functools.lru_cache(maxsize=None)
def features(dim, n=N_FEATURE):
    """-> A, B (3, dim, n): the three rows of the module docstring"""
    rng = np.random.default_rng(SEED + dim)
    A, B = np.empty((3, dim, n)), np.empty((3, dim, n))
    nt = 3 if dim == 6 else 2
    for r in range(3):
        A[r, :nt] = rng.standard_normal((nt, n))
        B[r, :nt] = rng.standard_normal((nt, n)) + 0.5
    if dim == 3:
        A[0, 2], B[0, 2] = rng.uniform(-math.pi, math.pi, n), rng.uniform(-math.pi, math.pi, n)
        A[1, 2], B[1, 2] = math.pi - rng.uniform(0.0, 0.03, n), -math.pi + rng.uniform(0.0, 0.03, n)
        A[2, 2], B[2, 2] = 0.3 * rng.standard_normal(n), 0.3 * rng.standard_normal(n)
    if dim == 6:
        for r in (0, 2):
            A[r, 3:], B[r, 3:] = 0.5 * rng.standard_normal((3, n)), 0.5 * rng.standard_normal((3, n))
        w0 = np.array([0.4, -0.7, 0.2])
        axis = np.array([2.0, -1.0, 2.0]) / 3.0
        A[1, 3:] = _compose(np.tile(w0, (n, 1)), 3e-5 * rng.standard_normal((n, 3))).T
        B[1, 3:] = _compose(_compose(np.tile(w0, (n, 1)), np.tile(NEAR_PI * axis, (n, 1))), 3e-5 * rng.standard_normal((n, 3))).T
    B[1, :, :10] = A[1, :, :10]                       # coincident points across the sets ...
    A[1, :, 50:55] = A[1, :, 0:5]                     # ... and inside one
    B[2] = A[2]
    B[2, 0] += 40.0
    B[2] = B[2][:, rng.permutation(n)]
    A.setflags(write=False); B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def golden(dim):
    X1, X2 = golden_files()
    A, B = project(dim, X1)[None], project(dim, X2)[None]
    A.setflags(write=False); B.setflags(write=False)
    return A, B


FIXTURE = os.path.join(GOLD, "mmd_reference.json")
DIGITS = 30


def tables(kind, dim):
    return features(dim) if kind == "features" else golden(dim)


def cases(kind):
    return CASES if kind == "features" else GOLDEN_CASES


def digest(A, B):
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(A).tobytes()); h.update(np.ascontiguousarray(B).tobytes())
    return h.hexdigest()


def compute(kind, dim):
    """the mp side of one table, as it is stored: {"digest", "rows": [{case: {"S": [3 strings], "mmd": string}}]}.  Slow
    (a minute in all): run by tests/test_mmd_ref_host.py, which holds the stored copy to it, and by `python tests/mmd_ref.py`."""
    A, B = tables(kind, dim)
    rows = []
    with mpm.workdps(DPS):
        for r in range(A.shape[0]):
            pairs = mp_pairs(dim, A[r], B[r])
            row = {}
            for name, sigma, scale in cases(kind):
                ref = mp_sums(dim, pairs, sigma, case_scale(dim, scale))
                row[name] = {"S": [mpm.nstr(x, DIGITS) for x in ref["S"]], "mmd": mpm.nstr(ref["mmd"], DIGITS)}
            rows.append(row)
    return {"digest": digest(A, B), "rows": rows}


@functools.lru_cache(maxsize=None)
def _stored():
    with open(FIXTURE) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def reference(kind, dim):
    """list over the rows of a table of {case name: {"S", "mmd" (mp), "T", "sigma", "scale", "bound": (sums, mmd)}}: the stored mp
    side (tests/golden/mmd_reference.json), which must belong to these very inputs; shared by every test and left unchanged"""
    A, B = tables(kind, dim)
    rec = _stored()["%s/%d" % (kind, dim)]
    assert rec["digest"] == digest(A, B), "tests/golden/mmd_reference.json was made for other inputs: run `python tests/mmd_ref.py`"
    na, nb = A.shape[2], B.shape[2]
    rows = []
    with mpm.workdps(DPS):
        for stored in rec["rows"]:
            row = {}
            for name, sigma, scale in cases(kind):
                c = stored[name]
                ref = {"S": tuple(mpm.mpf(x) for x in c["S"]), "mmd": mpm.mpf(c["mmd"]), "T": (na * na, na * nb, nb * nb)}
                row[name] = dict(ref, sigma=sigma, scale=case_scale(dim, scale), bound=bounds(ref))
            rows.append(row)
    return rows


def golden_halves():
    """mp mmd at σ = 1e-3, unit scale, of the even against the odd points of each sample file -> (X1 halves, X2 halves)"""
    X1, X2 = golden_files()
    return [mp_sums(6, mp_pairs(6, X[:, 0::2], X[:, 1::2]), 1e-3, None) for X in (X1, X2)]


if __name__ == "__main__":
    out = {"%s/%d" % (kind, dim): compute(kind, dim) for kind in ("features", "golden") for dim in DIMS}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", FIXTURE)
