"""The packed sweep k_conv_flat (and its VERIFY / GAUSS_NEWTON instantiations) against the root references of tests/conv_ref.py, at
every row shape of the launch arithmetic and at the SE(2) / SE(3) angle edges.  The kernel is reached the way bench.py reaches it: a
`_dev` entry with a `rows4` table and in-kernel noise (N = 15 and N = 513, the two neighbours of the packed range, run the wave-per-row
kernels against the same reference).  Every particle of every row is compared with the float64 root, the mp rows with mpmath as well;
bounds and snap-zone rule: conv_ref's docstring.

Every output buffer has a guard row before and after the table, guards and table pre-filled with NaN (status: -7): after a launch the
table must be finite and the guards untouched, so a row the block permutation drops or maps twice, or a store past a row, shows.

Status.  The functor check of NEWTON (VERIFY) compares against an ABSOLUTE tol = 1e-12 and re-evaluates the translation in another
operation order (a few ulp of the coordinates), so it is asserted where the row's translation scale is <= 100 (8 ulp(100) = 1.1e-13);
the shape tables keep every translation within that.  GAUSS_NEWTON on the Pose2 / Pose3 rows ends on an exactly reproduced iterate
(the residual Ts - s of the last step is exact) and is asserted everywhere.  The bearing-range iteration evaluates its functor from the
STORED landmark, ρ - ‖l - p.t‖: with the pose at 1e6 the difference l - p.t is quantised at ulp(1e6) = 1e-10, so no double-precision
landmark has a residual within 1e-12 and status 1 is the true report there (the proposal itself still meets its bound); like VERIFY it
is asserted where the row's translation scale is <= 100.
Prior rows are no root-find (the sample IS the proposal): their status is 0 whatever max_iters is."""
import ctypes as C
import math

import numpy as np
import pytest

import conv_ref as CR

pytestmark = pytest.mark.gpu
ENTRY = {CR.P2P2: "rome_conv_pose2pose2_dev", CR.BR0: "rome_conv_pose2point2br_dev", CR.P3P3: "rome_conv_pose3pose3_dev"}
ST_GUARD = -7
CF, NEWTON, GN = 0, 1, 3


@pytest.fixture(scope="module")
def env():
    import torch
    import rome_jl_amd as R
    from rome_jl_amd import _lib
    return torch, _lib, _lib.load(), R.Context(0)


class DevTable:
    """a conv_ref table on the device; `shift` places bel_fixed one double off its 16-byte alignment"""

    def __init__(self, env, t, shift=False):
        torch = env[0]
        self.t, self.kind, self.N = t, t["kind"], t["N"]

        def up(a, off=0):
            a = np.ascontiguousarray(a)
            buf = torch.zeros(a.size + 2, dtype=torch.from_numpy(a).dtype, device="cuda")
            buf[off:off + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
            return buf, buf[off:]
        self.keep = []
        for name, off in (("mu", 0), ("L", 0), ("bel_fixed", int(shift)), ("rows4", 0)):
            buf, view = up(t[name], off)
            self.keep.append(buf)
            setattr(self, name, view)
        if self.kind == CR.BR0:
            buf, self.bel_target = up(t["bel_target"])
            self.keep.append(buf)
        else:
            self.bel_target = self.bel_fixed
        assert self.bel_fixed.data_ptr() % 16 == (8 if shift else 0) and self.rows4.data_ptr() % 16 == 0


def launch(env, d, n_conv, solver, status=False, row0=0, shift=False, mirror=None, **opts):
    """rows [row0, row0 + n_conv) of the device table with streams stream_offset + row -> (out (n_conv, dt, N), status or None, mirror blocks
    or None).  mirror: ("map", array of n_conv slots) or ("rows", up to four row indices).  Guards are checked here."""
    torch, _lib, lib, ctx = env
    dt, N = CR.DIMS[d.kind][2], d.N
    blk = dt * N
    o = _lib.default_opts(solver, n_particles=N, seed=d.t["seed"], stream_offset=d.t["stream_offset"] + row0, **opts)
    off = int(shift)
    out = torch.full(((n_conv + 2) * blk + 2,), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full(((n_conv + 2) * N,), ST_GUARD, dtype=torch.int32, device="cuda") if status else None
    T = _lib.ConvDev()
    T.n_conv, T.dir_all = n_conv, 0
    T.mu, T.L, T.bel_fixed, T.bel_target = d.mu.data_ptr(), d.L.data_ptr(), d.bel_fixed.data_ptr(), d.bel_target.data_ptr()
    T.rows4 = d.rows4.data_ptr() + 16 * row0
    T.out = out.data_ptr() + 8 * (blk + off)
    if N % 2 == 0:
        assert T.out % 16 == (8 if shift else 0)
    if status:
        T.status = st.data_ptr() + 4 * N
    keep, mout, nslot = None, None, 0
    if mirror is not None:
        how, arg = mirror
        if how == "map":
            keep = torch.from_numpy(np.ascontiguousarray(arg, dtype=np.int32)).cuda()
            T.mirror_map = keep.data_ptr()
            nslot = int(max(arg)) + 1
        else:
            T.n_mirror = len(arg)
            for k, r in enumerate(arg):
                T.mirror_row[k] = r
            nslot = len(arg)
        mout = torch.full(((nslot + 2) * blk,), float("nan"), dtype=torch.float64, device="cuda")
        T.mirror_out = mout.data_ptr() + 8 * blk
    torch.cuda.synchronize()
    _lib.check(getattr(lib, ENTRY[d.kind])(ctx.handle, C.byref(o), C.byref(T)), ctx.handle)
    ctx.synchronize()
    h = out.cpu().numpy()
    lo, hi = blk + off, blk + off + n_conv * blk
    assert np.isnan(h[:lo]).all() and np.isnan(h[hi:]).all(), "a store outside the table"
    res = h[lo:hi].reshape(n_conv, dt, N)
    assert np.isfinite(res).all(), ("rows left unwritten", np.unique(np.argwhere(~np.isfinite(res))[:, 0])[:8].tolist())
    hs = None
    if status:
        hs = st.cpu().numpy()
        assert (hs[:N] == ST_GUARD).all() and (hs[(n_conv + 1) * N:] == ST_GUARD).all(), "a status store outside the table"
        hs = hs[N:(n_conv + 1) * N].reshape(n_conv, N)
        assert np.isin(hs, (0, 1)).all()
    hm = None
    if mirror is not None:
        hm = mout.cpu().numpy()
        assert np.isnan(hm[:blk]).all() and np.isnan(hm[(nslot + 1) * blk:]).all(), "a mirror store outside the buffer"
        hm = hm[blk:(nslot + 1) * blk].reshape(nslot, dt, N)
    return res, hs, hm, o


def _assert_ok(ref, out, what, gn_tol=0.0, mp=False):
    fig, bad = ref.check(out, gn_tol=gn_tol, mp=mp)
    print("CONVREF gpu %s N=%d n=%d %s %s" % (ref.kind, ref.table["N"], len(out), what, {k: round(v, 4) for k, v in fig.items()}))
    assert not bad, (what, bad)
    return fig


def _run_solvers(env, ref, d, n, mp, status_rows=None, gn_status_rows=None):
    """closed form, NEWTON without and with status, GAUSS_NEWTON on rows [0, n) -> (closed form, Gauss-Newton) outputs"""
    cf, _, _, _ = launch(env, d, n, CF)
    _assert_ok(ref, cf, "closed", mp=mp)
    nw, _, _, _ = launch(env, d, n, NEWTON)
    assert np.array_equal(nw, cf), "NEWTON without status is the closed form"
    nv, sv, _, _ = launch(env, d, n, NEWTON, status=True)
    assert np.array_equal(nv, cf), "the functor check must not change the proposal"
    assert not sv[slice(None) if status_rows is None else status_rows[:n]].any(), "NEWTON status at the default tol"
    gn, sg, _, o = launch(env, d, n, GN, status=True)
    assert o.tol == 1e-12 and o.max_iters >= 10
    _assert_ok(ref, gn, "gauss-newton", gn_tol=o.tol, mp=mp)
    if gn_status_rows is not None:
        # the rows left out are not left unpinned: with the pose beyond 1e6 the stored landmark quantises ‖l - p.t‖ at >= 1.2e-10, a
        # residual within 1e-12 is a 1-in-100 accident per particle, so such rows must report 1 for most particles
        far = ref.scale_t[:n] >= 1e6
        assert far.any() and (sg[far].mean(axis=1) >= 0.5).all(), sg[far].mean(axis=1)
        sg = sg[gn_status_rows[:n]]
    assert not sg.any(), ("GAUSS_NEWTON status from random starts", np.argwhere(sg)[:4].tolist())
    return cf, gn


@pytest.mark.parametrize("N", CR.PACKED_N + CR.NEIGHBOUR_N)
@pytest.mark.parametrize("kind", CR.KINDS)
def test_every_row_shape_against_the_root_references(env, kind, N):
    ref = CR.shape_reference(kind, N)
    d = DevTable(env, ref.table)
    ns = sorted(CR.n_conv_list(kind, N), reverse=True)
    assert ns[0] == ref.table["n_conv"] and (ref.scale_t <= 100.0).all()
    full_cf, full_gn = _run_solvers(env, ref, d, ns[0], mp=True)
    for n in ns[1:]:
        cf, gn = _run_solvers(env, ref, d, n, mp=False)
        # the first rows of a longer table: the same streams, so the same bits, whatever block and slot a row lands in
        assert np.array_equal(cf, full_cf[:n]) and np.array_equal(gn, full_gn[:n]), n


@pytest.mark.parametrize("kind", CR.KINDS)
def test_angle_and_scale_edges(env, kind):
    ref = CR.edge_reference(kind)
    d = DevTable(env, ref.table)
    n = ref.table["n_conv"]
    assert CR.launch_shape(ref.table["N"], n)["nb"] >= 3
    small = ref.scale_t <= 100.0
    assert small.sum() >= n // 2
    _run_solvers(env, ref, d, n, mp=True, status_rows=small, gn_status_rows=small if kind == CR.BR0 else None)


@pytest.mark.parametrize("kind", CR.KINDS)
def test_unaligned_views_give_the_same_bits(env, kind):
    """bel_fixed and out one double off a 16-byte boundary: N even without the 16-byte accesses"""
    ref = CR.shape_reference(kind, 100)
    n = ref.table["n_conv"]
    a, b = DevTable(env, ref.table), DevTable(env, ref.table, shift=True)
    for solver in (CF, GN):
        want = launch(env, a, n, solver, status=True)
        got = launch(env, b, n, solver, status=True, shift=True)
        assert np.array_equal(want[0], got[0]) and np.array_equal(want[1], got[1]), solver
    _assert_ok(ref, got[0], "unaligned gauss-newton", gn_tol=1e-12)


@pytest.mark.parametrize("N", (100, 101))
@pytest.mark.parametrize("kind", CR.KINDS)
def test_mirror_out(env, kind, N):
    ref = CR.shape_reference(kind, N)
    d = DevTable(env, ref.table)
    n = ref.table["n_conv"]
    plain, _, _, _ = launch(env, d, n, CF)
    slots = np.full(n, -1, dtype=np.int32)
    rows = [0, 4, 5, 17, n - 6, n - 1]                                           # first and last row, both sides of a block boundary
    for m, r in zip((5, 0, 3, 6, 1, 2), rows):                                   # slot 4 stays unused
        slots[r] = m
    for solver in (CF, GN):
        out, _, mir, _ = launch(env, d, n, solver, mirror=("map", slots))
        if solver == CF:
            assert np.array_equal(out, plain)
        for r in rows:
            assert np.array_equal(mir[slots[r]], out[r]), r
        assert np.isnan(mir[4]).all()
    out, _, mir, _ = launch(env, d, n, CF, mirror=("rows", [n - 1, 7, 0]))
    assert np.array_equal(out, plain)
    for m, r in enumerate([n - 1, 7, 0]):
        assert np.array_equal(mir[m], out[r])


@pytest.mark.parametrize("kind", CR.KINDS)
def test_a_row_alone_equals_the_row_in_the_table(env, kind):
    ref = CR.shape_reference(kind, 34)
    d = DevTable(env, ref.table)
    n = 47                                                                       # three full blocks of 15 rows and two rows
    for solver, status in ((CF, False), (NEWTON, True), (GN, True)):
        full, fs, _, _ = launch(env, d, n, solver, status=status)
        for c in range(n):
            one, os_, _, _ = launch(env, d, 1, solver, status=status, row0=c)
            assert np.array_equal(one[0], full[c]), (solver, c)
            assert not status or np.array_equal(os_[0], fs[c])


@pytest.mark.parametrize("kind", CR.KINDS)
def test_gauss_newton_reports_an_exhausted_iteration(env, kind):
    ref = CR.shape_reference(kind, 100)
    t = ref.table
    n = t["n_conv"]
    start = (t["bel_target"] if kind == CR.BR0 else t["bel_fixed"])[t["rows4"][:, 3]]
    et, er = CR.distance(kind, start, ref.root)
    rel = t["rows4"][:, 1] != CR.DIR_PRIOR
    assert (np.maximum(et, er)[rel] > 1e-3).all()                                  # every start is farther than 1e-3 from its root
    _, st, _, _ = launch(env, DevTable(env, t), n, GN, status=True, max_iters=1)
    assert (st[rel] == 1).all() and (st[~rel] == 0).all()


@pytest.mark.parametrize("mode", ("parity", "waves"))
@pytest.mark.parametrize("kind", CR.KINDS)
def test_gauss_newton_with_part_of_a_wave_already_at_the_root(env, kind, mode):
    """threads of alternating pair index (parity: both particles of a pair AT the float64 root, the next pair far away, so every ballot
    sees both) or whole wavefronts (waves: every ballot uniform) start at the root: the three paths through `undecided`, quat_log_iter's
    ballot and quat_log's small branch; the bearing-range ballots likewise.  conv_ref.mixed_start_mask, checked on the CPU."""
    N = CR.MIXED_N
    ref = CR.mixed_reference(kind)
    base = ref.table
    n = base["n_conv"]
    at_root = CR.mixed_start_mask(kind, mode, n)
    assert 0.3 < at_root.mean() < 0.7
    t = dict(base)
    key = "bel_target" if kind == CR.BR0 else "bel_fixed"
    bel = base[key].copy()
    tv = base["rows4"][:, 3]
    bel[tv] = np.where(at_root[:, None, :], CR.root_coords(kind, ref.root), bel[tv])
    t[key] = bel
    out, st, _, o = launch(env, DevTable(env, t), n, GN, status=True)
    _assert_ok(ref, out, "mixed " + mode, gn_tol=o.tol, mp=True)
    assert not st.any()
