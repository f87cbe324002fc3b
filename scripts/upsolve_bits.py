#!/usr/bin/env python3
"""Writes tests/golden/upsolve_bits.json: the sha256 of what rome_clique_proposals, rome_clique_upsolve and rome_upsolve_plan_create /
_run leave behind (host outputs, store contents, the mirror buffer) on the smallest tables that exercise what the host code behind
them decides -- the update index, the carve of the three arenas, forked phases, host and store-resident messages, stream ids, mirrors,
layout staging -- from the library that is loaded (ROME_MI355_LIB selects another build).  Run on the GPU with the library of the
commit whose bits are to be kept; tests/test_gpu_upsolve_bits.py asserts that they have not changed.

Case 1 goes through DeviceStore + UpsolvePlan; every other case fills the C structs itself (through ctypes), so that the script gives
the same calls to any build of the library.

    python scripts/upsolve_bits.py [out.json]"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

SHAPES_N = (33, 128)         # an odd size below one wavefront pair, and the largest size of the 128-thread product
GIBBS_ITERS = 2
SOA, AOS = 0, 1
DIM = (3, 2, 6)
NAMES = ("pose2", "point2", "pose3")


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        assert np.isfinite(a).all()
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


class _Table:
    """fills a CliqueHost / CliqueUpsolveHost from arrays and keeps them alive"""

    def __init__(self, struct):
        self.s, self.keep = struct, []

    def set(self, obj=None, **fields):
        obj = self.s if obj is None else obj
        for k, v in fields.items():
            if isinstance(v, np.ndarray):
                self.keep.append(v)
                assert v.flags["C_CONTIGUOUS"] and v.dtype in (np.float64, np.int32)
                v = v.ctypes.data_as(C.c_void_p) if v.size else None
            setattr(obj, k, v)


def _i32(a, shape=(-1,)):
    return np.ascontiguousarray(np.array(a, dtype=np.int32).reshape(shape))


def _beliefs(rng, N):
    """four poses along a line, three landmarks beside it, two Pose3 -- SoA blocks [n][dim][N]"""
    p2 = np.array([[2.0 * i, 0.0, 0.0] for i in range(4)])[:, :, None] + rng.normal(size=(4, 3, N)) * np.array([0.1, 0.1, 0.05])[None, :, None]
    pt = np.array([[2.0 * j + 1.0, 3.0] for j in range(3)])[:, :, None] + rng.normal(size=(3, 2, N)) * 0.1
    p3 = np.array([[2.0 * i, 0.0, 0.5 * i, 0.0, 0.0, 0.1 * i] for i in range(2)])[:, :, None] + \
        rng.normal(size=(2, 6, N)) * np.array([0.1, 0.1, 0.1, 0.01, 0.01, 0.01])[None, :, None]
    return [np.ascontiguousarray(a) for a in (p2, pt, p3)]


def _br(pose, point):
    d = np.array([2.0 * point + 1.0 - 2.0 * pose, 3.0])
    return [np.arctan2(d[1], d[0]), np.hypot(d[0], d[1])]


def _pose_landmark_rows(t):
    """the row tables of case 2 (poses x0..x3, landmarks l0..l2; updated: x1, l0 | x2, l1) into the CliqueHost of `t`"""
    cov3 = np.diag([0.01, 0.01, 0.0025]).reshape(-1)
    t.set(t.s.clique, n_p2p2=3, f_p2p2=3, p2p2_rows4=_i32([[0, 0, 0, 1], [1, 0, 1, 2], [2, 1, 3, 2]], (-1, 4)),
          p2p2_mu=np.ascontiguousarray(np.array([[2.0, 0, 0]] * 3)), p2p2_cov=np.ascontiguousarray(np.tile(cov3, (3, 1))),
          # (bearing, range) factors: pose <- landmark (br1), landmark <- pose (br0), one table
          n_br1=2, n_br0=2, f_br=4, br1_rows4=_i32([[0, 1, 2, 1], [1, 1, 2, 2]], (-1, 4)), br0_rows4=_i32([[2, 0, 0, 0], [3, 0, 3, 1]], (-1, 4)),
          br_mu=np.ascontiguousarray(np.array([_br(1, 2), _br(2, 2), _br(0, 0), _br(3, 1)])),
          br_sigma=np.ascontiguousarray(np.array([[0.03, 0.1]] * 4)),
          n_prpt2=1, f_prpt2=1, prpt2_rows4=_i32([[0, 2, 0, 0]], (-1, 4)), prpt2_mu=np.array([[1.0, 3.0]]),
          prpt2_cov=np.array([[0.04, 0.0, 0.0, 0.04]]))


def _to_layout(a, layout):
    return a if layout == SOA else np.ascontiguousarray(a.transpose(0, 2, 1))


def _pose_landmark_case(N, layout=SOA, mirror=None, smsg=True):
    """case 2: -> (table, {type: (new, bw)}); update list (x1, l0 | x2, l1): two groups, so both phases of a step fork"""
    from rome_jl_amd.clique import CliqueUpsolveHost
    rng = np.random.default_rng([N, 2])
    t = _Table(CliqueUpsolveHost())
    _pose_landmark_rows(t)
    msg2 = _to_layout(np.ascontiguousarray(np.array([[2.0, 0.1, 0.0]])[:, :, None] + rng.normal(size=(1, 3, N)) * 0.2), layout)
    msgp = _to_layout(np.ascontiguousarray(np.array([[3.0, 3.1]])[:, :, None] + rng.normal(size=(1, 2, N)) * 0.2), layout)
    out = {0: (np.zeros((2, 3, N) if layout == SOA else (2, N, 3)), np.zeros((2, 3))),
           1: (np.zeros((2, 2, N) if layout == SOA else (2, N, 2)), np.zeros((2, 2)))}
    t.set(gibbs_iters=GIBBS_ITERS, product_iters=1, schedule=0, n_up=4, up_type=_i32([0, 1, 0, 1]), up_var=_i32([1, 0, 2, 1]),
          up_group=_i32([0, 0, 1, 1]), up_stream=_i32([7, 3, 11, 5]),
          n_msg_pose2=1, msg_pose2=msg2, msg_pose2_up=_i32([0]), n_msg_point2=1, msg_point2=msgp, msg_point2_up=_i32([3]),
          new_pose2=out[0][0], bw_pose2=out[0][1], new_point2=out[1][0], bw_point2=out[1][1])
    if smsg:   # store-resident messages: x3 on x2, l2 on l0
        t.set(n_smsg_pose2=1, smsg_pose2_src=_i32([3]), smsg_pose2_up=_i32([2]), n_smsg_point2=1, smsg_point2_src=_i32([2]), smsg_point2_up=_i32([1]))
    if mirror is not None:
        t.set(up_mirror=_i32(mirror))
    return t, out


class _Env:
    def __init__(self):
        import rome_jl_amd as R
        from rome_jl_amd import _lib
        self.R, self._lib, self.lib, self.ctx = R, _lib, _lib.load(), R.Context(0)

    def check(self, rc):
        self._lib.check(rc, self.ctx.handle)

    def opts(self, N, layout=SOA):
        return self._lib.default_opts(self._lib.SOLVER_NEWTON, n_particles=N, seed=11, stream_offset=5, layout=layout)

    def store(self, N, bel):
        h = C.c_void_p()
        self.check(self.lib.rome_store_create(self.ctx.handle, N, len(bel[0]), len(bel[1]), len(bel[2]), C.byref(h)))
        for ti, b in enumerate(bel):
            self.check(self.lib.rome_store_upload(h, SOA, ti, 0, len(b), b.ctypes.data_as(C.POINTER(C.c_double))))
        return h

    def store_contents(self, h, N, counts):
        out = [np.full((n, DIM[ti], N), -7.0) for ti, n in enumerate(counts)]
        for ti, a in enumerate(out):
            self.check(self.lib.rome_store_download(h, SOA, ti, 0, len(a), a.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def plan_run(self, N, bel, t, mirror_doubles=0, mirror_stride=0):
        """a store over `bel`, the plan of table `t`, one run -> (store contents, mirror buffer or None)"""
        lib, o = self.lib, self.opts(N)
        st, P, dmir, mir = self.store(N, bel), C.c_void_p(), C.c_void_p(), None
        self.check(lib.rome_upsolve_plan_create(self.ctx.handle, st, C.byref(o), C.byref(t.s), C.byref(P)))
        if mirror_doubles:
            mir = np.full(mirror_doubles, -7.0)
            self.check(lib.rome_dev_alloc(self.ctx.handle, mir.nbytes, C.byref(dmir)))
            self.check(lib.rome_dev_upload(self.ctx.handle, dmir, mir.ctypes.data_as(C.c_void_p), mir.nbytes))
        self.check(lib.rome_upsolve_plan_run(P, C.byref(o), dmir, mirror_stride))
        self.check(lib.rome_ctx_synchronize(self.ctx.handle))
        got = self.store_contents(st, N, [len(b) for b in bel])
        if mirror_doubles:
            self.check(lib.rome_dev_download(self.ctx.handle, mir.ctypes.data_as(C.c_void_p), dmir, mir.nbytes))
            self.check(lib.rome_dev_free(self.ctx.handle, dmir))
        lib.rome_upsolve_plan_destroy(P)
        lib.rome_store_destroy(st)
        return got, mir


def case_chain(env, N):
    """1: Pose2 chain, three updates one after the other, through DeviceStore + UpsolvePlan -> the store"""
    from rome_jl_amd.clique import DeviceStore, UpsolvePlan
    R = env.R
    fg = R.generateGraph_Circle(6, N=N, landmark=False)
    R.dead_reckon_init(fg, seed=3)
    store = DeviceStore(fg, ctx=env.ctx)
    plan = UpsolvePlan(store, [["x1", "x2", "x3"]], gibbsIters=GIBBS_ITERS)
    plan.run(R.make_opts(N=N, seed=11, stream_offset=5))
    env.ctx.synchronize()
    h = _sha(*[store.get(l) for l in fg.variables])
    plan.close(); store.close()
    return h


def case_pose_landmark(env, N):
    """2: poses and landmarks, every message form, stream ids, host outputs -> new_*, bw_* and the store"""
    bel = _beliefs(np.random.default_rng([N, 1]), N)
    t, out = _pose_landmark_case(N)
    got, _ = env.plan_run(N, bel, t)
    return _sha(out[0][0], out[0][1], out[1][0], out[1][1], *got)


def case_pose3(env, N):
    """3: a Pose3 pair, both updated: a prior row and a Pose3Pose3 row on y0, a Pose3Pose3 row on y1 -> the store"""
    from rome_jl_amd.clique import CliqueUpsolveHost
    bel = _beliefs(np.random.default_rng([N, 1]), N)
    t = _Table(CliqueUpsolveHost())
    cov6 = np.diag([0.01] * 3 + [0.0001] * 3).reshape(-1)
    t.set(t.s.clique, n_p3p3=3, f_p3p3=2, p3p3_rows4=_i32([[0, 2, 0, 0], [1, 1, 1, 0], [1, 0, 0, 1]], (-1, 4)),
          p3p3_mu=np.ascontiguousarray(np.array([[0.0] * 6, [2.0, 0, 0.5, 0, 0, 0.1]])), p3p3_cov=np.ascontiguousarray(np.tile(cov6, (2, 1))))
    t.set(gibbs_iters=GIBBS_ITERS, product_iters=1, schedule=0, n_up=2, up_type=_i32([2, 2]), up_var=_i32([0, 1]))
    got, _ = env.plan_run(N, bel, t)
    return _sha(*got)


def case_mirror(env, N, stride):
    """4: case 2 with up_mirror -> the mirror buffer; stride 0 = the default 6 N, stride N = slots without padding"""
    bel = _beliefs(np.random.default_rng([N, 1]), N)
    t, _ = _pose_landmark_case(N, mirror=[0, 3, -1, 5])
    _, mir = env.plan_run(N, bel, t, mirror_doubles=(5 * (stride or 6 * N) + 6 * N), mirror_stride=stride)
    return _sha(mir)


def case_one_shot(env, N):
    """5: rome_clique_upsolve on the table of case 2 (without the store-resident messages, which belong to plans), AoS -> its outputs"""
    bel = _beliefs(np.random.default_rng([N, 1]), N)
    t, out = _pose_landmark_case(N, layout=AOS, smsg=False)
    t.set(t.s.clique, n_pose2=4, n_point2=3, n_pose3=0, bel_pose2=_to_layout(bel[0], AOS), bel_point2=_to_layout(bel[1], AOS))
    o = env.opts(N, AOS)
    env.check(env.lib.rome_clique_upsolve(env.ctx.handle, C.byref(o), C.byref(t.s)))
    return _sha(out[0][0], out[0][1], out[1][0], out[1][1])


def case_proposals(env, N):
    """6: rome_clique_proposals, all five families, hypothesis and stream columns on some -> out_*"""
    from rome_jl_amd.clique import CliqueUpsolveHost
    bel = _beliefs(np.random.default_rng([N, 1]), N)
    t = _Table(CliqueUpsolveHost())
    _pose_landmark_rows(t)
    cov6 = np.diag([0.01] * 3 + [0.0001] * 3).reshape(-1)
    out = {k: np.full((n, d, N), -7.0) for k, (n, d) in dict(p2p2=(3, 3), br1=(2, 3), br0=(2, 2), p3p3=(2, 6), prpt2=(1, 2)).items()}
    t.set(t.s.clique, n_pose2=4, n_point2=3, n_pose3=2, bel_pose2=bel[0], bel_point2=bel[1], bel_pose3=bel[2],
          n_p3p3=2, f_p3p3=1, p3p3_rows4=_i32([[0, 0, 0, 1], [0, 1, 1, 0]], (-1, 4)), p3p3_mu=np.array([[2.0, 0, 0.5, 0, 0, 0.1]]),
          p3p3_cov=np.ascontiguousarray(cov6.reshape(1, -1)),
          p2p2_nullhypo=np.array([0.0, 0.25, 0.0]), p2p2_stream=_i32([40, 2, 9]), br0_alt=_i32([-1, 2]), br0_hypo_w=np.array([1.0, 0.6]),
          br1_alt=_i32([0, -1]), br1_hypo_w=np.array([0.7, 1.0]), br1_nullhypo=np.array([0.1, 0.0]), p3p3_nullhypo=np.array([0.0, 0.2]),
          prpt2_stream=_i32([17]), **{"out_" + k: v for k, v in out.items()})
    o = env.opts(N)
    env.check(env.lib.rome_clique_proposals(env.ctx.handle, C.byref(o), C.byref(t.s.clique)))
    return _sha(*[out[k] for k in ("p2p2", "br1", "br0", "p3p3", "prpt2")])


def cases():
    """(key, function of the environment) of every recorded run"""
    for N in SHAPES_N:
        yield "1 chain plan N=%d" % N, lambda env, N=N: case_chain(env, N)
        yield "2 pose-landmark plan N=%d" % N, lambda env, N=N: case_pose_landmark(env, N)
        yield "3 pose3 plan N=%d" % N, lambda env, N=N: case_pose3(env, N)
        yield "4 mirror stride=default N=%d" % N, lambda env, N=N: case_mirror(env, N, 0)
        yield "4 mirror stride=N N=%d" % N, lambda env, N=N: case_mirror(env, N, N)
        yield "5 one-shot AoS N=%d" % N, lambda env, N=N: case_one_shot(env, N)
        yield "6 proposals N=%d" % N, lambda env, N=N: case_proposals(env, N)


def hashes():
    """{key: sha256} of every case above, from the loaded library"""
    env = _Env()
    out = {key: fn(env) for key, fn in cases()}
    env.ctx.close()
    return out


def main():
    from rome_jl_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "upsolve_bits.json")
    doc = {"what": "sha256 of the bytes (float64) that rome_clique_proposals, rome_clique_upsolve and up-solve plans leave in their host "
                   "outputs, the store and the mirror buffer on the cases of scripts/upsolve_bits.py",
           "library_version": int(_lib.load().rome_version()), "sha256": hashes()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d hashes -> %s" % (len(doc["sha256"]), out))


if __name__ == "__main__":
    main()
