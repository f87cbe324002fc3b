"""rome_linearize (k_lin and the seven lin_row_* bodies) row by row against references that share nothing with the kernel
(tests/lin_ref.py): mpmath at 50 digits on a subset of every table, a float64 NumPy restatement and the oracle's residuals on all rows.

Bounds: per table and output, 8x the deviation of the double-precision side (oracle residual, restated Jacobians) from mpmath, floor
64 ulp, times max(1, largest |reference entry| of the row); computed on the CPU by lin_ref.Reference, never from a GPU run.  The factor
8 covers fast_atan2 (<= 2 ulp), fast_sincos and the summation order of store_whitened.  The figures, the bounds and the largest
deviation seen on the GPU are recorded per kind and edge group in profiles/linearize_reference_errors.md; every check prints its own
(`pytest -s`).  No row is masked or skipped except the single landmark-on-the-pose row (n2 == 0) of its own test."""
import math

import numpy as np
import pytest

import lin_ref as L

pytestmark = pytest.mark.gpu
R = None
PREFIXES = (1, 63, 64, 65, 128, 129)


@pytest.fixture(scope="module", autouse=True)
def _pkg():
    global R
    import rome_jl_amd
    R = rome_jl_amd
    R.default_context()
    yield


def _run(t, F=None, W=None):
    n = len(t["mu"]) if F is None else F
    W = t["W"] if W is None else W
    out = R.linearize(t["kind"], t["mu"][:n], W[:n], t["xa"][:n], None if t["xb"] is None else t["xb"][:n])
    return dict(zip(("r", "Ja", "Jb"), out))


def _assert_within(tag, got, bound):
    print("LINREF gpu %s gpu_dev %.3e bound %.3e" % (tag, got, bound))
    assert got <= bound, (tag, got, bound)


def _check_table(tag, ref, out, upto=None):
    """every row against the double-precision side, the mp rows against mp"""
    n = ref.F if upto is None else upto
    for o in ref.outputs:
        assert np.all(np.isfinite(np.delete(out[o][:n], [f for f in [ref.table.get("excluded")] if f is not None and f < n], axis=0)))
        _assert_within("%s %s vs_double" % (tag, o), *ref.check_np(o, out[o], n))
        if upto is None:
            _assert_within("%s %s vs_mp" % (tag, o), *ref.check_mp(o, out[o]))
        else:
            k = [i for i, f in enumerate(ref.rows) if f < n]
            rows = [ref.rows[i] for i in k]
            d = L.deviation(ref.kind, ref.table["W"][rows], out[o][rows], ref.mp[o][k], wrapped=(o == "r")) / ref.scale[o][k]
            _assert_within("%s %s vs_mp" % (tag, o), float(d.max()), ref.rel_bound[o])


# ------------------------------------------------------------------ a. block geometry
@pytest.mark.parametrize("kind", L.KINDS)
def test_block_geometry_every_prefix_every_row(kind):
    ref = L.geometry_reference(kind)
    outs = {F: _run(ref.table, F) for F in PREFIXES}
    for F in PREFIXES:
        _check_table("%s geometry F=%d" % (L.NAMES[kind], F), ref, outs[F], upto=F)
    full = outs[129]
    for F in PREFIXES[:-1]:                                    # row i does not depend on how many rows follow it
        for o in ref.outputs:
            assert np.array_equal(outs[F][o], full[o][:F]), (kind, F, o)


# ------------------------------------------------------------------ b. position independence
@pytest.mark.parametrize("kind", L.KINDS)
def test_a_row_computes_the_same_at_every_position(kind):
    base = L.geometry_reference(kind).table
    fixed = L.geometry_table(kind, 1, seed=3)
    seen = []
    for pos in (0, 63, 64, 128):
        t = {k: (v if v is None or k == "kind" else np.array(v, copy=True)) for k, v in base.items()}
        for k in ("mu", "W", "xa", "xb"):
            if t[k] is not None:
                t[k][pos] = fixed[k][0]
        out = _run(t)
        seen.append({o: out[o][pos].copy() for o in out if out[o] is not None})
    ref = L.Reference(fixed)
    for o in ref.outputs:
        for s in seen[1:]:
            assert np.array_equal(s[o], seen[0][o]), (kind, o)
        _assert_within("%s moved_row %s vs_mp" % (L.NAMES[kind], o), *ref.check_mp(o, seen[0][o][None]))


# ------------------------------------------------------------------ c. Pose2 edges
@pytest.mark.parametrize("kind", L.POSE2_EDGE_KINDS)
def test_pose2_edges_against_mp(kind):
    """headings of ±π, ±(π − 1e-12), 3π, −7.5, 1e3; residuals on the ±π cut (r modulo 2π, Jacobians unmasked); for the bearing kinds
    distances 1e-6 .. 1e6 near the origin and near (1e6, −1e6), Jacobians relative to the row's largest reference entry"""
    for name, ref in L.edge_references(kind).items():
        _check_table("%s %s" % (L.NAMES[kind], name), ref, _run(ref.table))


@pytest.mark.parametrize("kind", (L.BEARINGRANGE, L.BEARING))
def test_bearing_residual_on_the_cut_stays_within_pi(kind):
    refs = L.edge_references(kind)
    for name in ("cut", "cut_snap"):
        t = refs[name].table
        dr = L.DIMS[kind][1]
        eye = np.tile(np.eye(dr), (len(t["mu"]), 1, 1))
        out = _run(t, W=eye)
        assert np.all(np.abs(out["r"][:, 0]) <= math.pi), out["r"][:, 0]
        ident = L.Reference(dict(t, W=eye))
        for o in ident.outputs:
            _assert_within("%s %s W=I %s vs_mp" % (L.NAMES[kind], name, o), *ident.check_mp(o, out[o]))


@pytest.mark.parametrize("kind", (L.BEARINGRANGE, L.BEARING))
def test_landmark_on_the_pose_disturbs_no_other_row(kind):
    """n2 == 0: the row's own outputs are whatever 0/0 gives (recorded in profiles/linearize_reference_errors.md: printed here);
    all other rows of its block and of the table are bit-identical to the run with an ordinary row in its place"""
    bad, good = L.n2zero_tables(kind)
    ob, og = _run(bad), _run(good)
    print("LINREF gpu %s n2zero row r=%s Ja=%s Jb=%s" % (L.NAMES[kind], ob["r"][70].tolist(), ob["Ja"][70].tolist(), ob["Jb"][70].tolist()))
    others = np.ones(129, bool); others[70] = False
    for o in ("r", "Ja", "Jb"):
        assert np.array_equal(ob[o][others], og[o][others]), o
        assert np.all(np.isfinite(ob[o][others]))
    _check_table("%s n2zero" % L.NAMES[kind], L.Reference(bad, L.subset_rows(129, 9)), ob)


@pytest.mark.parametrize("kind", L.KINDS)
def test_zero_W_gives_exact_zeros(kind):
    t = L.geometry_reference(kind).table
    out = _run(t, W=np.zeros_like(t["W"]))
    for o, v in out.items():
        assert v is None or np.all(v == 0.0), (kind, o)


# ------------------------------------------------------------------ d. Pose3 edges
@pytest.mark.parametrize("kind", L.POSE3_EDGE_KINDS)
def test_pose3_edges_against_mp(kind):
    """prescribed residual rotations 0 .. π − 1e-3 along generic and coordinate axes, pose vectors at so3_exp's zero guard and beyond
    the principal range, measurement rotations of 0 and 3 with translations of 1e3.  The near-π groups carry the error of the shared
    sqrt(1 − c²)/acos(c) logarithm: their bound is the oracle's own deviation there, not a wider table."""
    for name, ref in L.edge_references(kind).items():
        _check_table("%s %s" % (L.NAMES[kind], name), ref, _run(ref.table))


@pytest.mark.parametrize("kind", L.POSE3_EDGE_KINDS)
def test_jacobians_do_not_jump_across_the_series_switch(kind):
    """|φ| = 0.99e-4 and 1.01e-4 share everything else: the kernel's Jacobians may differ by what mp's differ, plus the tolerance"""
    ref = L.edge_references(kind)["phi_switch"]
    out = _run(ref.table)
    n = len(L.PHI_GROUPS["phi_switch"])
    for ax in range(len(L.AXES)):
        lo, hi = ax * n, ax * n + 1
        for o in ref.outputs[1:]:
            jump = np.abs(out[o][hi] - out[o][lo]).max()
            allowed = np.abs(ref.mp[o][hi] - ref.mp[o][lo]).max() + ref.rel_bound[o] * max(ref.scale[o][lo], ref.scale[o][hi])
            print("LINREF gpu %s switch axis %d %s jump %.3e allowed %.3e" % (L.NAMES[kind], ax, o, jump, allowed))
            assert jump <= allowed, (kind, ax, o, jump, allowed)
