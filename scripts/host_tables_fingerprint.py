"""Fingerprint of the host tables that turn a factor graph into what the library consumes, without a device: every column of every
`PackedGraph` table, the family records of a plan-only `DeviceGraph`, every field of the `rome_clique_host` / `rome_clique_upsolve_host`
that `CliqueBatch._fill` and `fill_upsolve_plan` write (scalars by value, arrays by digest, null pointers as None), and the refusals.
Arrays are reduced to a digest of dtype, shape and bytes, so equal digests mean equal tables.

    python scripts/host_tables_fingerprint.py [out.json]      -> the fingerprint of every case
    python scripts/host_tables_fingerprint.py --time          -> medians of nine builds of the three Manhattan-3500 host paths

tests/golden/host_tables.json is this output at the commit BEFORE the table builders of graph.py / device.py / clique.py were folded
(scripts copied into a checkout of that commit); tests/test_host_tables_pinned.py rebuilds every case and compares."""
import ctypes as C
import gc
import hashlib
import importlib.util
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import rome_jl_amd as R   # noqa: E402
from rome_jl_amd import clique as K   # noqa: E402
import test_bearing_host as TB   # noqa: E402
import test_device_graph_plan as TP   # noqa: E402
import test_rotation3_host as TR   # noqa: E402

_spec = importlib.util.spec_from_file_location("level_plan_fingerprint_n16", os.path.join(ROOT, "scripts", "level_plan_fingerprint.py"))
FP = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(FP)

N = TP.N   # 16
TABLES = ("p2p2", "p3p3", "br", "prior2", "prior3", "priorpt2", "p2rng", "pprng", "pbear", "p3xyy", "zrp3", "p3rot")
VTS = (R.Pose2, R.Point2, R.Pose3)


def digest(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256()
    h.update(("%s %r " % (a.dtype, a.shape)).encode()); h.update(a.tobytes())
    return h.hexdigest()[:16]


def _short(x):
    return hashlib.sha256(repr(x).encode()).hexdigest()[:16]


# ------------------------------------------------------------------------------------------------ graphs
def _prior_only():
    fg = R.initfg(N)
    fg.addVariable("x0", R.Pose2)
    fg.addFactor(["x0"], R.PriorPose2(R.MvNormal([1.0, 2.0, 0.5], np.diag([0.1, 0.1, 0.01]) ** 2)))
    return TB._zero_init(fg)


EXTRA = {"bearing_only": lambda: TB._zero_init(TB._bearing_graph(N)),
         "partial3": lambda: TR._zero_init(TR._graph(N, xyy=True, zrp=True)),
         "pose2_tables": lambda: R.synth_pose2_tables(64, N=N)[0],
         "prior_only": _prior_only}
PACKED_GRAPHS = sorted(TP.GRAPHS) + sorted(EXTRA)


def source(name):
    """the factor graph (or, for pose2_tables, the PackedGraph) of one case"""
    return EXTRA[name]() if name in EXTRA else TP.GRAPHS[name][0]()


def packed(name):
    g = source(name)
    return g if isinstance(g, R.PackedGraph) else R.PackedGraph(g)


# ------------------------------------------------------------------------------------------------ (a) PackedGraph
def _column(v):
    if isinstance(v, np.ndarray):
        return digest(v)
    if isinstance(v, dict):
        return {k: _column(x) for k, x in v.items()}
    return v if isinstance(v, list) else int(v)


def packed_tables(pk):
    out = {t: _column(getattr(pk, t)) for t in TABLES}
    out["N"], out["index"] = pk.N, sorted(pk.index.items())
    out["labels"] = {vt.name: list(pk.labels[vt]) for vt in VTS}
    return out


# ------------------------------------------------------------------------------------------------ (b) DeviceGraph
def device_layout(name):
    g = source(name)
    dg = R.DeviceGraph(g, plan_only=True)
    out = TP.describe(dg)
    tname = lambda vt: None if vt is None else vt.name
    out["records"] = {f: dict(entry=r["entry"], stream=r["stream"], partial=None if r["partial"] is None else list(r["partial"]),
                              prop_lo=r["prop_lo"], vt_fixed=tname(r["vt_fixed"]), vt_target=tname(r["vt_target"]))
                      for f, r in dg.fams.items()}
    scalar = lambda v: v if v is None or isinstance(v, (bool, int)) else "tensor"
    out["tab"] = {f: {k: scalar(v) for k, v in tb.items()} for f, tb in dg.tab.items()}
    out["fused"], out["unfused"] = [r["name"] for r in dg._fused], [r["name"] for r in dg._unfused]
    return json.loads(json.dumps(out))


# ------------------------------------------------------------------------------------------------ (c) CliqueBatch
def struct_fields(s, arrays):
    """every field of a ctypes struct: scalars by value, pointers by the digest of the array of `arrays` they address (None = null)"""
    by_addr = {a.ctypes.data: a for a in arrays if a.size}
    out = {}
    for name, ct in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out[name] = struct_fields(v, arrays)
        elif ct is C.c_void_p:
            out[name] = None if not v else digest(by_addr[v])
        else:
            out[name] = int(v)
    return out


def batch_rows(b):
    plain = lambda x: x.item() if isinstance(x, np.generic) else x
    fam = lambda d: {k: [[plain(x) for x in row] if isinstance(row, tuple) else plain(row) for row in v] for k, v in d.items()}
    return dict(rows=sorted([fl, tg, f, r] for (fl, tg), (f, r) in b.rows.items()), fam_rows=fam(b.fam_rows), fam_hyp=fam(b.fam_hyp),
                fam_sid=fam(b.fam_sid), fam_meas=fam(b.fam_meas))


CLIQUE_LOCAL = ("hexagon", "beehive_mh", "bearingrange_nullhypo", "landmark_prior_frozen", "helix3d")


def clique_local(name):
    """all (factor, connected variable) pairs of the graph through CliqueBatch._fill over clique-local arrays"""
    fg = source(name)
    b = R.CliqueBatch(fg, [(fl, l) for fl, labels, _ in fg.factors for l in labels])
    q, keep = K.CliqueHost(), []
    out = b._fill(q, keep)
    return dict(struct=struct_fields(q, keep + list(out.values())), vars={vt.name: b.vars[vt] for vt in VTS}, **batch_rows(b))


UPSOLVE = ("hex_relative", "mitbr_relative_hop", "beehive_relative", "helix_relative")


class KeepingBackend(FP.RecordingBackend):
    """the recording backend, which also keeps the arguments of every Plan"""

    def __init__(self):
        FP.RecordingBackend.__init__(self)
        self.plans = []

    def Plan(self, store, spec, share=None, mirror=None):
        self.plans.append((spec, share, mirror))
        return FP.RecordingBackend.Plan(self, store, spec, share, mirror)


def logged_plans(case, n=N):
    """-> ([(spec, share, mirror) per Plan step], the store numbering of the finished universe)"""
    FP.N = n
    FP.graph.cache_clear()
    backend = FP.build(case, KeepingBackend())[1]
    return backend.plans, FP.RecordingStore(backend.universe).index


def fill_level(spec, share, mirror, index):
    u, keep = K.CliqueUpsolveHost(), []
    batch, _ = K.fill_upsolve_plan(u, keep, spec.fg, index, K.plan_level(spec, share, index), mirror)
    return u, keep, batch


def upsolve_steps(case):
    """per Plan step of the case: digests of the filled rome_clique_upsolve_host and of the batch's row lists; for mitbr_relative_hop
    also the share [0] of its first level with more than one clique, as the last entry"""
    plans, index = logged_plans(case)
    if case == "mitbr_relative_hop":
        spec = next(s for s, _, _ in plans if len(s.cliques) > 1)
        plans = plans + [(spec, [0], None)]
    out = []
    for spec, share, mirror in plans:
        u, keep, batch = fill_level(spec, share, mirror, index)
        out.append(dict(struct=_short(struct_fields(u, keep)), **{k: _short(v) for k, v in batch_rows(batch).items()}))
    return out


def _raised(fn):
    try:
        fn()
    except Exception as e:
        return [type(e).__name__, str(e)]
    return None


def error_paths():
    fg = TP.GRAPHS["hexagon"][0]()
    fg.putFactor("s01", ["x0", "x1"], K.SampledPose2Pose2("x2"))
    fg.putFactor("smh", ["x0", "x1", "x2"], K.SampledPose2Pose2("x3"), multihypo=(0.5, 0.5))
    return dict(sampled_without_store=_raised(lambda: R.CliqueBatch(fg, [("s01", "x1")])._fill(K.CliqueHost(), [])),
                sampled_multihypo=_raised(lambda: R.CliqueBatch(fg, [("smh", "x1")])),
                target_not_on_factor=_raised(lambda: R.CliqueBatch(fg, [("x0x1f1", "x3")])))


# ------------------------------------------------------------------------------------------------ (d) refusals
def _refused_graph(kind):
    fg = R.initfg(N)
    p3 = kind == "partial3"
    fg.addVariable("x0", R.Pose3 if p3 else R.Pose2); fg.addVariable("x1", R.Pose3 if p3 else R.Pose2); fg.addVariable("l0", R.Point2)
    if p3:
        fg.addFactor(["x0"], R.PriorPose3(R.MvNormal(np.zeros(6), np.eye(6) * 0.01)))
        fg.addFactor(["x0", "x1"], R.Pose3Pose3(R.MvNormal(np.zeros(6), np.eye(6) * 0.01)))
        fg.addFactor(["x0", "x1"], R.Pose3Pose3XYYaw(R.MvNormal([1.0, 0.0, 0.0], np.eye(3) * 0.01)))
    else:
        fg.addFactor(["x0"], R.PriorPose2(R.MvNormal(np.zeros(3), np.eye(3) * 0.01)))
        fg.addFactor(["x0", "x1"], R.Pose2Pose2(R.MvNormal([1.0, 0.0, 0.0], np.eye(3) * 0.01)))
        if kind in ("bearing", "bearing_then_range"):
            fg.addFactor(["x0", "l0"], R.Pose2Point2Bearing(R.Normal(0.3, 0.05)))
        if kind in ("range", "bearing_then_range"):
            fg.addFactor(["x1", "l0"], R.Pose2Point2Range(R.Normal(3.0, 0.1)))
    return TB._zero_init(fg)


def refusals():
    out = {}
    for kind in ("range", "bearing", "partial3", "bearing_then_range"):
        fg = _refused_graph(kind)
        out[kind] = {"CliqueBatch": _raised(lambda: R.CliqueBatch(fg, [(fl, ls[-1]) for fl, ls, _ in fg.factors])),
                     "DeviceStore": _raised(lambda: K.DeviceStore(fg)),
                     "TreeSolver": _raised(lambda: R.TreeSolver(fg)),
                     "initAllOrdered": _raised(lambda: R.initAllOrdered(fg)),
                     "solveTree": _raised(lambda: R.solveTree(fg))}
    return out


# ------------------------------------------------------------------------------------------------ all of it, and the timing mode
DEVICE_GRAPHS = sorted(EXTRA)   # (the eight of tests/golden/device_graph_plans.json stay in their own test)


def fingerprint():
    return dict(packed={g: packed_tables(packed(g)) for g in PACKED_GRAPHS},
                device={g: device_layout(g) for g in DEVICE_GRAPHS},
                clique={g: clique_local(g) for g in CLIQUE_LOCAL},
                upsolve={c: upsolve_steps(c) for c in UPSOLVE},
                errors=error_paths(), refusals=refusals())


def _median_ms(fn, reps=9):
    """median of `reps` timed calls after one untimed; the cyclic collector is off inside a timed call, as in `timeit` (when it runs
    depends on what the process allocated before, not on the code under the clock)"""
    fn()
    ts = []
    for _ in range(reps):
        gc.collect(); gc.disable()
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
        gc.enable()
    return 1e3 * statistics.median(ts)


def timing():
    """(the two graph builds are timed before the tree solver exists: its heap makes their allocations erratic)"""
    fg = R.loadG2o(os.path.join(ROOT, "tests", "golden", "manhattan.g2o"), N=100)
    pk = R.PackedGraph(fg)
    out = {"PackedGraph(Manhattan-3500)": _median_ms(lambda: R.PackedGraph(fg)),
           "DeviceGraph(packed, plan_only=True)": _median_ms(lambda: R.DeviceGraph(pk, plan_only=True))}
    plans, index = logged_plans("m3500_relative", n=100)
    out["plan_level + fill_upsolve_plan, %d levels of m3500_relative" % len(plans)] = _median_ms(lambda: [fill_level(s, sh, m, index) for s, sh, m in plans])
    return out


if __name__ == "__main__":
    if "--time" in sys.argv[1:]:
        for k, ms in timing().items():
            print("%-70s median of 9: %9.2f ms" % (k, ms))
    else:
        text = json.dumps(fingerprint(), indent=0, sort_keys=True)
        if len(sys.argv) > 1:
            with open(sys.argv[1], "w") as f:
                f.write(text + "\n")
        print("%d bytes, digest %s" % (len(text), _short(text)))
