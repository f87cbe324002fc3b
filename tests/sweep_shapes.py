"""Launch helpers and the case list of tests/test_gpu_packed_sweep_shapes.py, shared with scripts/packed_sweep_bits.py (which writes
tests/golden/packed_sweep_bits.json from the same cases).  Not a test module.

A table is one of tests/conv_ref.py's shape tables (shape_reference: mixed dir 0 / dir 1 / prior rows, factor and variable indices out of
row order, every variable -- the last block of the store too -- fixed in several rows); a case runs its first n rows.

Two ways into the library for the same rows, same streams (stream_offset + row), same seed:
  packed  -- `rows4` table, in-kernel noise: launch_ppl's plain sweep, the packed kernel k_conv_flat for 16 <= N <= 512
  wave    -- the four table columns as separate arrays and no `rows4`: not a plain sweep, so one wavefront per row (k_conv), the
             feature-complete instantiation
Every output buffer has a guard block before and after the table, pre-filled with NaN (status: -7), checked after the launch.

Hypothesis tables (tests/hypo_ref.py) carry `alt_var`, `hypo_w` and `nullhypo` columns: Dev uploads them where the table has them and
launch(hypo=...) attaches the named ones; noise=... hands the launch its normals (or, with presampled=1, its measurement samples).

Ring tables (tests/ring_ref.py: "br1", "p2r", "ppr0", "ppr1", "pb0", "pb1") go through the range, bearing and bearing-range entries; their
dimensions and direction come from ring_ref.DIMS / DIR_ALL, and the landmark and pose kinds keep their targets in a store of their own."""
import ctypes as C
import functools
import hashlib

import numpy as np

import conv_ref as CR
import ring_ref as RR

ENTRY = {CR.P2P2: "rome_conv_pose2pose2_dev", CR.BR0: "rome_conv_pose2point2br_dev", CR.P3P3: "rome_conv_pose3pose3_dev",
         "br1": "rome_conv_pose2point2br_dev", "p2r": "rome_conv_point2point2range_dev", "ppr0": "rome_conv_pose2point2range_dev",
         "ppr1": "rome_conv_pose2point2range_dev", "pb0": "rome_conv_pose2point2bearing_dev", "pb1": "rome_conv_pose2point2bearing_dev"}
ST_GUARD = -7
HYPO_COLUMNS = {"alt_var": 4, "hypo_w": 8, "nullhypo": 8}                                # column -> bytes per row
CF, NEWTON, GN = 0, 1, 3
SHAPE_N = (16, 18, 100, 101, 512)            # H = 8 (< NK: two staging passes), H = 9 (= NK of Pose2: one), CPB = 5, the odd N, one row per block


def n_conv_cases(N):
    """1, CPB - 1, CPB, CPB + 1, 8 CPB + 3: one row, a partial / full / just-started last block, fewer than 8 blocks, a block count
    that is no multiple of 8"""
    cpb = CR.launch_shape(N, 1)["CPB"]
    return sorted({n for n in (1, cpb - 1, cpb, cpb + 1, 8 * cpb + 3) if n >= 1})


@functools.lru_cache(maxsize=None)
def reference(kind, N):
    """conv_ref's shape reference of (family, N) -- shared with tests/test_gpu_packed_sweep.py -- or, where that table is shorter than the
    longest case (Pose3 at N >= 256), the same table with enough rows"""
    ref = CR.shape_reference(kind, N)
    need = n_conv_cases(N)[-1]
    return ref if ref.table["n_conv"] >= need else CR.Reference(CR.shape_table(kind, N, n_conv=need))


class Dev:
    """a conv_ref table on the device; shift: bel_fixed (and bel_target) one double off their 16-byte alignment"""

    def __init__(self, torch, t, shift=False):
        self.torch, self.t, self.kind, self.N, self.shift = torch, t, t["kind"], t["N"], bool(shift)
        self.keep = []
        self.mu, self.L = self._up(t["mu"]), self._up(t["L"])
        self.bel_fixed = self._up(t["bel_fixed"], int(shift))
        own = self.kind == CR.BR0 or (self.kind in RR.DIMS and "bel_target" in t)     # (a p2r table has one Point2 store)
        self.bel_target = self._up(t["bel_target"], int(shift)) if own else self.bel_fixed
        rows = np.ascontiguousarray(t["rows4"], dtype=np.int32)
        self.rows4 = self._up(rows)
        self.cols = [self._up(np.ascontiguousarray(rows[:, k])) for k in range(4)]       # factor, dir, fixed_var, target_var
        self.hypo = {k: self._up(t[k]) for k in HYPO_COLUMNS if k in t}                  # per-row hypothesis columns of a hypo_ref table

    def _up(self, a, off=0):
        torch = self.torch
        a = np.ascontiguousarray(a)
        buf = torch.zeros(a.size + 2, dtype=torch.from_numpy(a).dtype, device="cuda")
        buf[off:off + a.size] = torch.from_numpy(a.reshape(-1)).cuda()
        self.keep.append(buf)
        return buf[off:]


def launch(env, d, n_conv, solver, how="packed", status=False, row0=0, shift=False, mirror=None, hypo=(), noise=None, dir_all=0,
           refused=False, **opts):
    """rows [row0, row0 + n_conv) of the device table -> (out (n_conv, dt, N), status (n_conv, N) or None, mirror blocks or None).
    how: "packed" (rows4) or "wave" (column arrays).  shift: `out` and the mirror buffer one double off their 16-byte alignment.
    mirror: ("map", slots per row) or ("rows", up to four row indices).  hypo: names of the hypothesis columns of d to attach.
    noise: (n_conv, dz, N) host array for the `noise` field.  dir_all: the direction of a bearing-range table.
    refused=True: the entry point must return an error and store nothing -> its error code."""
    torch, _lib, lib, ctx = env
    ring = d.kind in RR.DIMS
    if ring:
        dir_all = RR.DIR_ALL[d.kind]
    dz = RR.DIMS[d.kind][0] if ring else CR.DIMS[d.kind][0]
    dt, N = (RR.DIMS[d.kind][2] if ring else 3 if d.kind == CR.BR0 and dir_all == 1 else CR.DIMS[d.kind][2]), d.N     # bearing-range towards the pose: the target is a Pose2
    blk = dt * N
    assert 0 <= row0 and row0 + n_conv <= len(d.t["rows4"]), "rows beyond the table"
    o = _lib.default_opts(solver, n_particles=N, seed=d.t["seed"], stream_offset=d.t["stream_offset"] + row0, **opts)
    off = int(shift)
    out = torch.full(((n_conv + 2) * blk + 2,), float("nan"), dtype=torch.float64, device="cuda")
    st = torch.full(((n_conv + 2) * N,), ST_GUARD, dtype=torch.int32, device="cuda") if status else None
    T = _lib.ConvDev()
    T.n_conv, T.dir_all = n_conv, dir_all
    T.mu, T.L, T.bel_fixed, T.bel_target = d.mu.data_ptr(), d.L.data_ptr(), d.bel_fixed.data_ptr(), d.bel_target.data_ptr()
    if how == "packed":
        T.rows4 = d.rows4.data_ptr() + 16 * row0
    else:
        T.factor, T.dir, T.fixed_var, T.target_var = [c.data_ptr() + 4 * row0 for c in d.cols]
        if d.kind == CR.BR0 or (ring and d.kind != "p2r"):
            T.dir = None                                                              # the direction of a bearing-range table is dir_all
    T.out = out.data_ptr() + 8 * (blk + off)
    for name in hypo:
        setattr(T, name, d.hypo[name].data_ptr() + HYPO_COLUMNS[name] * row0)
    if noise is not None:
        assert noise.shape == (n_conv, dz, N)
        hold = torch.from_numpy(np.ascontiguousarray(noise, dtype=np.float64)).cuda()
        T.noise = hold.data_ptr()
    if status:
        T.status = st.data_ptr() + 4 * N
    keep, mout, nslot = None, None, 0
    if mirror is not None:
        kind_, arg = mirror
        if kind_ == "map":
            keep = torch.from_numpy(np.ascontiguousarray(arg, dtype=np.int32)).cuda()
            T.mirror_map = keep.data_ptr()
            nslot = int(max(arg)) + 1
        else:
            T.n_mirror = len(arg)
            for k, r in enumerate(arg):
                T.mirror_row[k] = r
            nslot = len(arg)
        mout = torch.full(((nslot + 2) * blk + 2,), float("nan"), dtype=torch.float64, device="cuda")
        T.mirror_out = mout.data_ptr() + 8 * (blk + off)
    torch.cuda.synchronize()
    rc = getattr(lib, ENTRY[d.kind])(ctx.handle, C.byref(o), C.byref(T))
    if refused:
        ctx.synchronize()
        assert rc != 0, "the entry point accepted the table"
        assert np.isnan(out.cpu().numpy()).all() and (st is None or (st.cpu().numpy() == ST_GUARD).all()), "a refused launch stored something"
        assert mout is None or np.isnan(mout.cpu().numpy()).all(), "a refused launch stored a mirror block"
        return rc
    _lib.check(rc, ctx.handle)
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
        assert np.isnan(hm[:lo]).all() and np.isnan(hm[lo + nslot * blk:]).all(), "a mirror store outside the buffer"
        hm = hm[lo:lo + nslot * blk].reshape(nslot, dt, N)
    return res, hs, hm


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


# the tables of tests/golden/packed_sweep_bits.json: (kind, N, rows, solver), the proposal bytes of the packed launch
GOLDEN_CASES = [(CR.P2P2, 16, 131, CF), (CR.P2P2, 18, 131, CF), (CR.P2P2, 100, 43, CF), (CR.P2P2, 100, 43, GN), (CR.P2P2, 101, 43, CF),
                (CR.P2P2, 512, 11, CF), (CR.BR0, 16, 131, CF), (CR.BR0, 100, 43, CF), (CR.BR0, 101, 43, GN), (CR.P3P3, 18, 131, CF),
                (CR.P3P3, 100, 43, CF), (CR.P3P3, 101, 43, GN), (CR.P3P3, 512, 11, CF)]


def golden_key(kind, N, n, solver):
    return "%s N=%d rows=%d solver=%d" % (kind, N, n, solver)


def golden_hashes(env):
    out = {}
    for kind, N, n, solver in GOLDEN_CASES:
        d = Dev(env[0], reference(kind, N).table)
        out[golden_key(kind, N, n, solver)] = sha(launch(env, d, n, solver)[0])
    return out
