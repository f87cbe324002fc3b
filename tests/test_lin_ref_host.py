"""The references of tests/lin_ref.py check one another on the CPU: mpmath against the oracle's double residuals, against the two-line
closed-form Jacobians of the Pose2 kinds, and against the float64 NumPy restatement; every constructed row of the GPU test's tables is
finite in mp and lies where its construction says.  Run with -s, it prints the reference-side error figures from which
tests/test_gpu_linearize.py derives its bounds (recorded in profiles/linearize_reference_errors.md).

Bounds asserted here, all relative to max(1, largest |reference entry| of the row):
  * ordinary rows: 64 ulp.  Every double-precision side is a handful of correctly rounded libm calls and at most a 6-term whitening
    sum, a few ulp of the row scale; 64 ulp is the floor below which the GPU bound is not tightened either.
  * rows whose formula loses digits by construction get the loss worked out in place (see each test)."""
import math

import numpy as np
import pytest

import lin_ref as L

ULP64 = 64.0 * L.EPS


def test_kind_numbers_and_dims_are_the_librarys():
    from rome_jl_amd import _lib, api
    names = ("PRIORPOSE2", "POSE2POSE2", "POSE2POINT2BR", "PRIORPOINT2", "POSE3POSE3", "PRIORPOSE3", "POSE2POINT2BEARING")
    assert [getattr(_lib, "FACTOR_" + n) for n in names] == list(L.KINDS)
    assert api._LIN_DIMS == L.DIMS


def test_the_distributed_stand_in_is_this_restatement():
    import test_distributed_gloo as g
    assert g._cpu_linearize is L.np_linearize


@pytest.mark.parametrize("kind", L.KINDS)
def test_mp_residuals_and_restatement_agree_on_ordinary_rows(kind):
    ref = L.geometry_reference(kind)
    assert len(ref.rows) >= 8 and ref.F == 129
    for o in ref.outputs:
        assert np.all(np.isfinite(ref.mp[o]))
        print("LINREF cpu %s geometry %s ref_err %.3e bound %.3e" % (L.NAMES[kind], o, ref.figure[o], ref.rel_bound[o]))
        assert ref.figure[o] <= ULP64, (kind, o, ref.figure[o])           # oracle residual / restated Jacobians against mp
    assert ref.dev["r_np"].max() <= ULP64                                  # the restatement's own residual


@pytest.mark.parametrize("kind", (L.PRIORPOSE2, L.POSE2POSE2, L.PRIORPOINT2))
def test_mp_jacobians_of_the_pose2_kinds_match_their_closed_forms(kind):
    ref = L.geometry_reference(kind)
    t = ref.table
    for k, f in enumerate(ref.rows):
        W, z = t["W"][f], t["mu"][f]
        if kind == L.POSE2POSE2:
            s, c = math.sin(t["xa"][f, 2]), math.cos(t["xa"][f, 2])
            JA = np.array([[1, 0, -s * z[0] - c * z[1]], [0, 1, c * z[0] - s * z[1]], [0, 0, 1]])
            assert np.abs(ref.mp["Jb"][k] + W).max() <= ULP64 * ref.scale["Jb"][k]
        else:
            JA = -np.eye(len(z))
        assert np.abs(ref.mp["Ja"][k] - W @ JA).max() <= ULP64 * ref.scale["Ja"][k], (kind, f)


def test_bearing_jacobian_of_mp_is_smooth_across_the_cut():
    """the unwrapped difference: a row 1e-9 from +π has the Jacobian of the same geometry with the measured bearing moved off the cut"""
    ref = L.edge_references(L.BEARINGRANGE)["cut_snap"]
    t = {k: (None if v is None or k == "kind" else np.array(v, copy=True)) for k, v in ref.table.items()}
    t["mu"][:, 0] -= 1.0
    r2, Ja2, Jb2 = L.ref_rows(L.BEARINGRANGE, t["mu"], t["W"], t["xa"], t["xb"], ref.rows)
    assert np.abs(Ja2 - ref.mp["Ja"]).max() < 1e-15 and np.abs(Jb2 - ref.mp["Jb"]).max() < 1e-15
    assert np.abs(r2 - ref.mp["r"]).max() > 0.5


@pytest.mark.parametrize("kind", L.POSE2_EDGE_KINDS + L.POSE3_EDGE_KINDS)
def test_edge_tables_are_finite_in_mp_and_their_figures(kind):
    """Every constructed row is served by mp (no exclusion) and is finite there.  Figures above the 64 ulp floor are explained:
      * cut_snap: sym_rem returns −π for |x − π| <= √eps·π, the rows sit 1e-9 from π: 1e-9/π of the row scale (the reference's rule);
      * bearing_1e3: a measured bearing of 1e3 enters a subtraction whose rounding is ulp(1e3)/2 = 5.7e-14, times the whitening row
        (its own group: the other headings, a pose heading of 1e3 included, stay at the floor);
      * range 1e6 against positions of 1e6: ulp(1e6)-sized differences, still relative to a row scale of 1e6 and below 64 ulp;
      * Pose3 rows: sqrt(1 − c²)/acos(c) rounds c² at eps, which is eps/θ² relative near θ = 0 and eps/(π − θ)² near π: the figures
        1e-13 at 1e-4 and 5e-10 at π − 1e-3 are that formula's, shared by the reference project, the oracle and the kernel.  Each
        group's figure must stay under the formula's worked-out loss at the group's worst angle (lin_ref.log_formula_error), so a
        restatement that lost more than the formula explains would fail here and not widen the kernel's bound unseen."""
    refs = L.edge_references(kind)
    for name, ref in refs.items():
        assert ref.rows == list(range(ref.F)), name
        for o in ref.outputs:
            assert np.all(np.isfinite(ref.mp[o])), (name, o)
            print("LINREF cpu %s %s %s ref_err %.3e bound %.3e" % (L.NAMES[kind], name, o, ref.figure[o], ref.rel_bound[o]))
            cap = ULP64
            if name == "cut_snap" and o == "r":
                cap = 2e-9
            elif name == "bearing_1e3" and o == "r":
                cap = 4 * 5.7e-14                                          # ulp(1e3)/2, times a dense whitening row
            elif name in ("phi_switch", "phi_mid", "near_pi_1e-2", "near_pi_1e-3"):
                worst = max(L.PHI_GROUPS[name], key=lambda th: th / math.sin(th) ** 2)
                cap = L.log_formula_error(worst)                           # 9.0e-12, 1.3e-13, 2.8e-11, 2.8e-09
            assert ref.figure[o] <= cap, (kind, name, o, ref.figure[o], cap)


@pytest.mark.parametrize("kind", (L.BEARINGRANGE, L.BEARING))
def test_bearing_cut_rows_lie_where_they_were_put(kind):
    refs = L.edge_references(kind)
    seen = []
    for name in ("cut", "cut_snap"):
        t = refs[name].table
        for f in range(len(t["mu"])):
            d, side = L.bearing_cut_distance(t["mu"], t["xa"], t["xb"], f)
            off = min(L.CUT_OFFSETS, key=lambda o: abs(abs(d) - o))
            assert abs(abs(d) - off) < 1e-3 * off, (name, f, d)
            assert (name == "cut_snap") == (side > 0 and off < 1e-8)
            seen.append((off, side, d > 0))
            assert abs(L.ref_residual(kind, t["mu"], t["xa"], t["xb"], f)[0]) <= math.pi
    assert len(set(seen)) == 8                                             # 1e-9 and 1e-4, of +π and of −π, from inside and from outside
    dist = refs["distance"].table
    n = np.hypot(*(dist["xb"] - dist["xa"][:, :2]).T)
    assert np.allclose(n, np.tile(L.DISTANCES, 2), rtol=2e-4)


@pytest.mark.parametrize("kind", (L.PRIORPOSE2, L.POSE2POSE2))
def test_pose2_cut_rows_lie_within_1e12_of_the_cut(kind):
    t = L.edge_references(kind)["cut"].table
    for f in range(4):
        r2 = L.ref_residual(kind, t["mu"], t["xa"], t["xb"], f)[2]
        assert math.pi - abs(r2) < 2e-12, (f, r2)


@pytest.mark.parametrize("kind", L.POSE3_EDGE_KINDS)
def test_pose3_residual_rotations_have_the_prescribed_norms(kind):
    refs = L.edge_references(kind)
    for name, norms in L.PHI_GROUPS.items():
        t = refs[name].table
        assert len(t["mu"]) == len(norms) * len(L.AXES)
        for f in range(len(t["mu"])):
            got = np.linalg.norm(L.ref_residual(kind, t["mu"], t["xa"], t["xb"], f)[3:])
            want = norms[f % len(norms)]
            assert abs(got - want) <= 1e-15 + 1e-12 * want, (name, f, got, want)
            assert got <= math.pi - 1e-3 + 1e-12
    sw = refs["phi_switch"].table
    for base in range(0, 3 * len(L.AXES), 3):                                                    # the two sides of so3_jinv's th2 < 1e-8
        lo = np.linalg.norm(L.ref_residual(kind, sw["mu"], sw["xa"], sw["xb"], base)[3:])
        hi = np.linalg.norm(L.ref_residual(kind, sw["mu"], sw["xa"], sw["xb"], base + 1)[3:])
        assert lo * lo < 1e-8 < hi * hi
    pc = refs["pose_coords"].table
    which = pc["xa"]                                                       # both kinds carry the extreme vector as xa in the even rows
    assert np.allclose(np.linalg.norm(which[0::2, 3:], axis=1), L.POSE_NORMS, rtol=1e-12, atol=0)
    assert np.all(which[0, 3:] == 0.0)                                     # so3_exp's zero guard, exactly
    other = pc["xb"] if kind == L.POSE3POSE3 else pc["mu"]
    assert np.allclose(np.linalg.norm(other[1::2, 3:], axis=1), L.POSE_NORMS, rtol=1e-12, atol=0)


def test_n2zero_table_excludes_exactly_one_row():
    for kind in (L.BEARINGRANGE, L.BEARING):
        bad, good = L.n2zero_tables(kind)
        assert bad["excluded"] == 70 and np.all(bad["xb"][70] == bad["xa"][70, :2])
        same = np.ones(129, bool); same[70] = False
        for k in ("mu", "W", "xa", "xb"):
            assert np.array_equal(bad[k][same], good[k][same])
