"""Fingerprint of everything the multi-rank drivers (rome_jl_amd.distributed) lay out before their first step, without a device or a
process group: over plan-only DeviceGraphs of the fixture graphs of tests/test_device_graph_plan.py (N = 16)

  * SeparatorPipeline: payload, arena size and contents, where every store / receive buffer sits in the arena, and per plans[b][k] the
    entry, the stream offset, every integer keyword, the null-ness of the optional keywords, a digest of every index / weight tensor and,
    per buffer keyword, which buffer it views at what offset and length;
  * TargetShardedSweep: the shard bounds, digests of the sorted tables and what its one launch is handed;
  * FrontierShard.plan with recording plan / scatter classes (as `bench.py --dry-run` uses): width, labels, mirror map, scatter lists and
    the send slice.

    python scripts/rank_plan_fingerprint.py [out.json]

tests/golden/rank_plans.json is this output at the commit BEFORE the rank-driver refactor (one all-gather, one launch-keyword builder,
one plan per TargetShardedSweep); tests/test_rank_plans_pinned.py rebuilds every case and compares key by key."""
import functools
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch   # noqa: E402
import rome_jl_amd as R   # noqa: E402
from rome_jl_amd.distributed import SeparatorPipeline, TargetShardedSweep, FrontierShard   # noqa: E402
import test_device_graph_plan as G   # noqa: E402  (the fixture graphs)

N = G.N
STREAM0 = 1000
OPTIONAL = ("alt_var", "hypo_w", "nullhypo", "mirror_map", "mirror_out")
TENSORS = ("rows4", "alt_var", "hypo_w", "nullhypo", "mirror_map", "mu", "L")
BUFFERS = ("bel_fixed", "bel_target", "out", "mirror_out")


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def digest(x):
    """short digest of an array's dtype, shape and bytes (None -> None)"""
    if x is None:
        return None
    a = np.ascontiguousarray(_np(x))
    return hashlib.sha256(repr((str(a.dtype), a.shape)).encode() + a.tobytes()).hexdigest()[:12]


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> (fg, plan-only DeviceGraph holding the graph's beliefs)"""
    fg, dg = G.build(name, plan_only=True)
    dg.upload_beliefs(fg)
    return fg, dg


def _opts(rank):
    return R.make_opts(N=N, seed=7, stream_offset=STREAM0 + (rank << 32))


# ---------------------------------------------------------------------------------------------------------------- SeparatorPipeline
PIPE_GRAPHS = ("hexagon", "beehive_mh", "bearingrange_nullhypo", "helix3d")


def pipe_layout(dg):
    """publish: the first and the last row of every family; ghosts: one per variable type present, fed by the previous rank's slot 0 --
    the variable that the type's alternative columns name first where there is one (so the alternative column follows the ghost), else
    the type's last variable"""
    fams = dg.families()
    publish, vts, named = [], [], {}
    for f in fams:
        tb = dg.family_table(f)
        publish += [(f, r) for r in sorted({0, tb["n"] - 1})]
        for vt in (tb["vt_fixed"], tb["vt_target"]):
            if vt not in vts:
                vts.append(vt)
        if tb["alt"] is not None:
            alt = _np(tb["alt"])
            vl = tb["vt_fixed"] if f == "br1" else tb["vt_target"]
            if (alt >= 0).any():
                named.setdefault(vl, int(alt[alt >= 0][0]))
    ghosts = lambda rank: [(vt, named.get(vt, dg.bel[vt].shape[0] - 1), rank - 1, 0) for vt in vts]   # noqa: E731
    return publish, ghosts


def _view(t, buffers):
    """which of the named buffers the tensor `t` views: [name, offset in elements, length]"""
    if t is None:
        return None
    for name, buf in buffers:
        o = t.data_ptr() - buf.data_ptr()
        if buf.numel() and 0 <= o and o + t.numel() * t.element_size() <= buf.numel() * buf.element_size():
            return [name, o // t.element_size(), t.numel()]
    return ["?", 0, t.numel()]


def describe_plan(pl, buffers):
    kw = pl.kw
    return dict(entry=pl.fn, stream_offset=int(pl.opts.stream_offset),
                ints={k: v for k, v in sorted(kw.items()) if isinstance(v, int)},
                null=[k for k in OPTIONAL if kw.get(k) is None],
                digests={k: digest(kw.get(k)) for k in TENSORS},
                views={k: _view(kw.get(k), buffers) for k in BUFFERS})


def pipeline_case(name, world, rank, depth):
    fg, dg = graph(name)
    publish, ghosts = pipe_layout(dg)
    p = SeparatorPipeline(dg, _opts(rank), None, world, rank, publish, ghosts(rank), depth=depth)
    off = lambda t: (t.data_ptr() - p.arena.data_ptr()) // 8   # noqa: E731
    plans = []
    for b in range(depth):
        buffers = [("arena", p.arena), ("send%d" % b, p.send[b])] + [("out%d.%s" % (b, f), p.out[b][f]) for f in p.families]
        plans.append([describe_plan(pl, buffers) for pl in p.plans[b]])
    return dict(payload=p.payload, arena=p.arena.numel(), arena_digest=digest(p.arena), families=list(p.families),
                store={vt.name: [off(s), list(s.shape)] for vt, s in p.store.items()},
                recv=[[off(r), r.numel()] for r in p.recv], send=[s.numel() for s in p.send], plans=plans)


# --------------------------------------------------------------------------------------------------------------- TargetShardedSweep
SHARD_GRAPHS = ("manhattan_prefix", "beehive_mh", "bearingrange_nullhypo")


def shard_case(name, world, rank):
    fg, dg = graph(name)
    sh = TargetShardedSweep(dg, _opts(0), None, world, rank)
    out = dict(q=sh.q, row_lo=sh.row_lo, row_hi=sh.row_hi, n_rows=sh.n_rows, order=digest(sh.order), ptr=digest(sh.ptr), rows4=digest(sh.rows4),
               alt=digest(getattr(sh, "alt", None)), w=digest(getattr(sh, "w", None)), nh=digest(getattr(sh, "nh", None)),
               store=list(sh.store.shape), store_digest=digest(sh.store), mine=_view(sh.mine, [("store", sh.store)]), plan=None)
    if sh.n_rows:   # (a rank without rows launches nothing)
        out["plan"] = describe_plan(sh.plan, [("store", sh.store), ("prop", sh.prop)])
    return out


# -------------------------------------------------------------------------------------------------------------------- FrontierShard
FRONTIERS = {"level0": [["x0", "x1"], ["x3"], ["x5"]], "level1": [["x2"], ["x4"], ["x6", "l1"]], "two": [["x2"], ["x6", "l1"]]}


class _Rec:
    def __init__(self, *a, **kw):
        self.a, self.kw = a, kw


def frontier_case(frontier, world, rank, always_collective):
    fg, _ = graph("hexagon")

    class _Store:
        pass
    st = _Store()
    st.N, st.fg = N, fg
    sh = FrontierShard(st, torch, None, world, rank, plan_cls=_Rec, scatter_cls=_Rec, always_collective=always_collective)
    pl = sh.plan(FRONTIERS[frontier], gibbsIters=2)
    up, sc = pl["up"], pl["scatter"]
    return dict(width=pl["width"], U=pl["U"], labels=pl["labels"], recv=pl["recv"].numel(), send=_view(pl["send"], [("recv", pl["recv"])]),
                mirror=None if up is None else sorted(up.kw["mirror"].items()), share=None if up is None else up.kw["share"],
                scatter=None if sc is None else [list(sc.a[1]), list(sc.a[2]), sc.kw["stride"]])


def cases():
    """case name -> thunk"""
    out = {}
    for g in PIPE_GRAPHS:
        for world in (1, 3):
            for rank in range(world):
                for depth in (2, 3):
                    out["pipeline/%s/world%d/rank%d/depth%d" % (g, world, rank, depth)] = functools.partial(pipeline_case, g, world, rank, depth)
    for g in SHARD_GRAPHS:
        for world in (1, 2, 3, 8):
            for rank in range(world):
                out["shard/%s/world%d/rank%d" % (g, world, rank)] = functools.partial(shard_case, g, world, rank)
    for fr in FRONTIERS:
        for world in (1, 2, 3):
            for rank in range(world):
                for ac in (False, True):
                    out["frontier/%s/world%d/rank%d/%s" % (fr, world, rank, "collective" if ac else "plain")] = functools.partial(frontier_case, fr, world, rank, ac)
    return out


if __name__ == "__main__":
    out = {name: fn() for name, fn in cases().items()}
    text = json.dumps(out, indent=0, sort_keys=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    print("%d cases, %d bytes, digest %s" % (len(out), len(text), hashlib.sha256(text.encode()).hexdigest()[:12]))
