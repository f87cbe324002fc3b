"""The root references of tests/conv_ref.py check one another on the CPU: the float64 restatement against mpmath on the mp rows of every
table, against the C oracle's convolutions under the oracle's own Philox draws, and the case tables against what they are listed for
(launch shapes, snap-zone membership and margin).  Run with -s, it prints the reference-side error figures recorded in conv_ref's
docstring; the GPU tests derive their bounds from the same objects."""
import math
import os
import re

import numpy as np
import pytest

import conv_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_CEILING = 8.0 * CR.EPS      # np_root against mp: a handful of correctly rounded operations per coordinate, relative to the row scale


def _references():
    for kind in CR.KINDS:
        yield "edge", kind, CR.edge_reference(kind)
        for N in CR.PACKED_N + CR.NEIGHBOUR_N:
            yield "N=%d" % N, kind, CR.shape_reference(kind, N)


def test_launch_arithmetic_and_every_shape_hits_its_case():
    src = open(os.path.join(ROOT, "rome.jl_amd", "csrc", "rome_conv.hpp")).read()
    assert int(re.search(r"constexpr int kFlatThreads = (\d+);", src).group(1)) == CR.FLAT_THREADS
    assert int(re.search(r"constexpr int kFlatMaxRows = (\d+);", src).group(1)) == CR.FLAT_MAX_ROWS
    assert "lean && a.N >= %d && (a.N + 1) / 2 <= kFlatThreads" % CR.FLAT_MIN_N in src
    assert re.search(r"#define ROME_FLAT_PP (\d+)", src).group(1) == "1"          # H = ceil(N / 2): one pair per thread in every instantiation
    for N, (what, hits) in CR.SHAPE_CASES.items():
        s = CR.launch_shape(N, 1)
        assert s["packed"] and hits(s), (N, what, s)
        assert 0 < s["live"] <= CR.FLAT_THREADS and (s["CPB"] + 1) * s["H"] > CR.FLAT_THREADS or s["clamped"], (N, s)
        for kind in CR.KINDS:
            ns = CR.n_conv_list(kind, N)
            nbs = [CR.launch_shape(N, n)["nb"] for n in ns]
            assert nbs == list(CR.NB[:len(ns)]) and len(ns) == (3 if kind == CR.P3P3 and N >= 256 else 5), (kind, N, ns)
            if s["CPB"] > 1:
                assert all(n % s["CPB"] != 0 for n in ns), (N, ns)            # the last block is partly filled
    assert {CR.launch_shape(N, 1)["CPB"] for N in CR.PACKED_N} == {16, 15, 5, 3, 2, 1}
    assert any(N % 2 for N in CR.PACKED_N) and not any(CR.launch_shape(N, 1)["packed"] for N in CR.NEIGHBOUR_N)
    assert [nb & 7 for nb in CR.NB] == [1, 7, 0, 1, 3]                          # the block permutation with and without a remainder
    # H < NK: the constants of a Pose3 row (27) are staged in more than one pass
    assert CR.launch_shape(CR.EDGE_N, 1)["H"] < 27 and CR.launch_shape(16, 1)["H"] == 8


def test_shape_table_content():
    for kind in CR.KINDS:
        t = CR.shape_table(kind, 100)
        r = t["rows4"]
        assert t["stream_offset"] > 2 ** 32 and CR.shape_table(kind, 34)["stream_offset"] < 2 ** 32
        assert len(t["mu"]) < t["n_conv"] and (r[:, 0] != np.arange(t["n_conv"])).mean() > 0.8
        assert np.bincount(r[:, 2]).min() >= 2 and (np.diff(r[:, 2]) < 0).any() and (np.diff(r[:, 3]) < 0).any()
        if kind != CR.BR0:
            assert [int(d) for d in r[:6, 1]] == [0, 1, 2, 0, 1, 2]                # one wave spans all three row kinds
        else:
            f = r[:, 0]
            assert (t["mu"][f, 1] >= 8.0 * t["L"][f, 1]).all()


@pytest.mark.parametrize("kind", CR.KINDS)
def test_np_root_against_mp_on_every_table(kind):
    worst = {"t": 0.0, "r": 0.0}
    for name, k, ref in _references():
        if k != kind:
            continue
        t = ref.table
        assert len(ref.rows) >= 1 and set(t["edge_rows"]) <= set(ref.rows)
        for c in ref.rows:                                                      # mp is finite on every row it serves, edge rows included
            for el in ref.mp[c]:
                flat = list(el[0]) + ([el[1]] if kind == CR.P2P2 else [v for row in el[1] for v in row] if kind == CR.P3P3 else [])
                assert all(math.isfinite(float(v)) for v in flat), (name, c)
        for part in ("t", "r"):
            print("CONVREF cpu %s %s %s dev %.2f eps bound %.3e" % (CR.NAMES[kind], name, part, ref.dev[part] / CR.EPS, ref.rel_bound[part]))
            assert ref.dev[part] <= DEV_CEILING, (name, part, ref.dev[part])
            assert ref.rel_bound[part] == CR.ULP64
            worst[part] = max(worst[part], ref.dev[part])
        for v in ref.root.values():
            assert np.isfinite(v).all(), name
        # snap zone: decided by the reference, with the stated margin; under 5 % of a Pose3 table, empty elsewhere
        if kind == CR.P3P3:
            assert ref.zone.mean() < 0.05, name
            assert (np.abs(ref.to_pi - CR.ZONE_EDGE) >= CR.ZONE_MARGIN).all(), name
            assert ((ref.to_pi < CR.ZONE_EDGE) == ref.zone).all(), name
            if name == "edge":
                assert ref.zone.sum() == 4 * t["N"]                               # two prior rows and the two compositions, every particle
        else:
            assert not ref.zone.any()
    print("CONVREF cpu %s worst dev %.2f / %.2f eps" % (CR.NAMES[kind], worst["t"] / CR.EPS, worst["r"] / CR.EPS))


def test_edge_tables_hold_what_they_list():
    ref = CR.edge_reference(CR.P3P3)
    t = ref.table
    fx = t["bel_fixed"][t["rows4"][:, 2]]
    norms = np.sqrt((fx[:, 3:] ** 2).sum(axis=1))                                 # (C, N)
    munorm = np.sqrt((t["mu"][t["rows4"][:, 0], 3:] ** 2).sum(axis=1))
    dirs = t["rows4"][:, 1]
    for m in CR.P3_MAGS:
        tol = 1e-12 * max(m, 1e-300)
        as_fixed = np.abs(norms - m).max(axis=1) <= tol                          # every particle of the fixed block at |ω| = m
        as_mu = np.abs(munorm - m) <= tol
        for dr in (0, 1):                                                        # p_ω (dir 0) and q_ω (dir 1); z_ω in both directions
            assert (as_fixed & (dirs == dr)).any() and (as_mu & (dirs == dr)).any(), (m, dr)
        assert (as_mu & (dirs == CR.DIR_PRIOR)).any(), m
    z = CR.measurements(t, ref.xi)
    zn = np.sqrt((z[..., 3:] ** 2).sum(axis=-1))
    for m, side in ((0.9e-8, -1), (1.1e-8, 1)):                                   # |z_ω| stays on its side of the th2 > 1e-16 switch
        rows = np.abs(munorm - m) <= 1e-12 * m
        assert ((zn[rows] ** 2 > 1e-16) == (side > 0)).all()
    assert (zn[munorm == 0.0] == 0.0).all()
    ang = CR.q_angle(ref.root["q"])
    assert (ref.root["q"][..., 0] < 0).any()                                      # the q_w < 0 branch (2 + 2 on one axis)
    assert (ang < 1e-15).all(axis=1).sum() >= 2                                   # p and z cancel to the identity
    tmax = np.abs(ref.root["t"]).max(axis=(1, 2))
    assert (tmax > 1e5).any() and (tmax < 1e-1).any()
    r2 = CR.edge_reference(CR.P2P2)
    th = r2.root["th"]
    assert ((np.abs(th) > math.pi) & (np.abs(th) < math.pi + 0.3)).any() and ((np.abs(th) < math.pi) & (np.abs(th) > math.pi - 0.3)).any()
    assert (np.abs(r2.table["bel_fixed"][:, 2]) == math.pi).any() and (r2.table["bel_fixed"][:, 2] == 7.0).any()
    rb = CR.edge_reference(CR.BR0)
    zb = CR.measurements(rb.table, rb.xi)
    assert (zb[..., 1] > 0).all() and zb[..., 1].min() < 2e-3 and zb[..., 1].max() > 5e3


@pytest.mark.parametrize("kind", CR.KINDS)
def test_np_root_against_the_oracle_with_its_own_philox(kind):
    """ties the noise rule (stream = stream_offset + row, particle id) and the row conventions (factor / dir / fixed / target columns,
    packed L) of np_root to ro.conv_*: benign tables, closed form, 1e-9"""
    import oracle as ro
    for N in (34, 100, 101):
        ref = CR.shape_reference(kind, N)
        t = ref.table
        r = t["rows4"]
        o = ro.make_opts(N=N, solver=ro.SOLVER_CLOSED_FORM, seed=t["seed"], stream_offset=t["stream_offset"])
        if kind == CR.P2P2:
            out = ro.conv_pose2pose2(o, t["mu"], t["L"], t["bel_fixed"], r[:, 2], r[:, 3], r[:, 1], factor=r[:, 0])
        elif kind == CR.P3P3:
            out = ro.conv_pose3pose3(o, t["mu"], t["L"], t["bel_fixed"], r[:, 2], r[:, 3], r[:, 1], factor=r[:, 0])
        else:
            out = ro.conv_pose2point2br(o, 0, t["mu"], t["L"], t["bel_fixed"], t["bel_target"], r[:, 2], r[:, 3], factor=r[:, 0])
        if kind != CR.BR0:                                                      # the oracle samples prior rows through its own entry
            sample = ro.sample_priorpose2 if kind == CR.P2P2 else ro.sample_priorpose3
            pri = r[:, 1] == CR.DIR_PRIOR
            assert pri.sum() >= len(r) // 3
            out[pri] = sample(o, t["mu"], t["L"], factor=r[:, 0])[pri]
        et, er = CR.distance(kind, out, ref.root)
        assert et.max() <= 1e-9 and er.max() <= 1e-9, (kind, N, et.max(), er.max())


def test_root_coords_round_trip_and_wave_groups():
    ref = CR.shape_reference(CR.P3P3, 34)
    et, er = CR.distance(CR.P3P3, CR.root_coords(CR.P3P3, ref.root), ref.root)
    assert et.max() == 0.0 and er.max() <= 8 * CR.EPS
    # mixed-convergence masks: in "parity" every wave holds both states among the first and among the second particles of its threads
    for kind in CR.KINDS:
        n = CR.mixed_reference(kind).table["n_conv"]
        grp = CR.wave_groups(kind, CR.MIXED_N, n)
        blk = (np.arange(n) // CR.launch_shape(CR.MIXED_N, n)["CPB"])[:, None]
        m = CR.mixed_start_mask(kind, "parity", n)
        w = CR.mixed_start_mask(kind, "waves", n)
        for b in range(blk.max()):                                               # (the last block is partly filled)
            for g_ in range(4):
                for k in (0, 1):
                    sel = (grp == g_) & (blk == b) & ((np.arange(CR.MIXED_N) % 2 == k)[None, :])
                    assert sel.any() and m[sel].any() and not m[sel].all(), (kind, b, g_, k)
                    assert w[sel].all() or not w[sel].any()
        assert (m[:, 0::2] == m[:, 1::2]).all()                                  # both particles of a pair share a state
    g = CR.wave_groups(CR.P2P2, 100, 13)
    assert g.shape == (13, 100) and g.min() == 0 and g.max() == 3 and (g[0, :100] == 0).all() and g[1, 28] == 1 and g[1, 27] == 0
