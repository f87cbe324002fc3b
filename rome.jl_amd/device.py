"""Device-resident belief store + graph-indexed convolution sweeps (torch = device memory/streams only).

One `sweep_*` call = one kernel launch over a whole table of (factor, direction) convolutions with
the beliefs staying in HBM -- what a clique/whole-graph pass of `solveTree!`
(examples/ManhattanDatasetBatch.jl:43; IIF upGibbsCliqueDensity -> approxConvBelief) issues.
"""
import ctypes as C

import numpy as np

from . import _lib
from .factors import (Pose2, Point2, Pose3, Point2Point2Range, Pose2Point2Range, Pose2Point2Bearing, Pose3Pose3XYYaw, PriorPose3ZRP,
                      Pose3Pose3Rotation, partial_coverage)
from .graph import PackedGraph
from .api import cholesky_lower


def partial_tasks(ptr, rows, row_cover, dim):
    """The tables of the partial-aware product of one variable type, on the host.  ptr [V+1] / rows: the CSR variable ->
    proposal rows; row_cover[r]: the 0-based coordinates row r solves, or None for a full row.  -> dict of int32 arrays:
    full_ptr / full_rows, the CSR of the full rows alone (stage 1), and one task per (variable, covered coordinate) in (v, c) order:
    task_var, task_coord, task_ptr [T+1] / task_rows (the partial rows covering c, in CSR order), task_joint (1: v has full rows, whose
    product enters as the last density)."""
    ptr, rows = np.asarray(ptr, dtype=np.int64), np.asarray(rows, dtype=np.int64)
    if len(rows) and (rows.min() < 0 or rows.max() >= len(row_cover)):
        raise ValueError("partial_tasks: proposal row %d is outside the %d rows of row_cover" % (rows.min() if rows.min() < 0 else rows.max(), len(row_cover)))
    for r, m in enumerate(row_cover):
        if m is not None and (len(m) == 0 or min(m) < 0 or max(m) >= dim):
            raise ValueError("partial_tasks: row %d covers coordinates %s of a %d-dimensional variable" % (r, tuple(m), dim))
    i32 = lambda a: np.asarray(a, dtype=np.int32)
    if all(m is None for m in row_cover):   # (the usual graph: nothing to walk)
        none = i32([])
        return dict(full_ptr=i32(ptr), full_rows=i32(rows), task_var=none, task_coord=none, task_ptr=i32([0]), task_rows=none, task_joint=none)
    full_ptr, full_rows, task_var, task_coord, task_ptr, task_rows, task_joint = [0], [], [], [], [0], [], []
    for v in range(len(ptr) - 1):
        rv = [int(r) for r in rows[ptr[v]:ptr[v + 1]]]
        full = [r for r in rv if row_cover[r] is None]
        full_rows += full
        full_ptr.append(len(full_rows))
        for c in range(dim):
            cov = [r for r in rv if row_cover[r] is not None and c in row_cover[r]]
            if cov:
                task_var.append(v); task_coord.append(c); task_joint.append(1 if full else 0)
                task_rows += cov
                task_ptr.append(len(task_rows))
    return dict(full_ptr=i32(full_ptr), full_rows=i32(full_rows), task_var=i32(task_var), task_coord=i32(task_coord),
                task_ptr=i32(task_ptr), task_rows=i32(task_rows), task_joint=i32(task_joint))


def _require_torch_cuda():
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("rome_jl_amd.device needs a HIP device (torch.cuda.is_available() is False); "
                           "there is no CPU fallback")
    return torch


class _PlanStub:
    """what DeviceGraph._plan returns on a plan-only graph: the launch descriptor's arguments, not a launch"""

    def __init__(self, fn, opts, kw):
        self.fn, self.kw = fn, kw
        self.opts = _lib.Opts.from_buffer_copy(opts)

    def __call__(self):
        raise RuntimeError("plan-only DeviceGraph (bench.py --dry-run): there is no device to launch on")


class DeviceGraph:
    def __init__(self, fg_or_packed, device="cuda:0", ctx=None, plan_only=False):
        """plan_only: build the same tables on CPU tensors WITHOUT a device or a context -- the multi-GPU drivers can then lay out
        every rank's arena / exchange plan on a machine without GPUs (`bench.py --gpus 8 --dry-run`); nothing can be launched."""
        self.plan_only = bool(plan_only)
        if plan_only:
            import torch
            device = "cpu"
        else:
            torch = _require_torch_cuda()
        self.torch = torch
        self.device = torch.device(device)
        pk = fg_or_packed if isinstance(fg_or_packed, PackedGraph) else PackedGraph(fg_or_packed)
        self.packed = pk
        self.N = pk.N
        self.ctx = None if plan_only else (ctx or _lib.Context(self.device.index or 0))
        self._lib = None if plan_only else _lib.load()
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=self.device)
        f64, i32 = torch.float64, torch.int32
        self.bel = {Pose2: torch.zeros((len(pk.labels[Pose2]), 3, self.N), dtype=f64, device=self.device),
                    Point2: torch.zeros((len(pk.labels[Point2]), 2, self.N), dtype=f64, device=self.device),
                    Pose3: torch.zeros((len(pk.labels[Pose3]), 6, self.N), dtype=f64, device=self.device)}
        # ---- the family list: one record per (factor family, direction) that is launched on its own, in LAUNCH order.  The proposal
        # rows (prop_lo: rows of prop[vt_target] in list order per target type), the Philox offsets, the CSR, conv_step, the sweep
        # methods and family_table() are all derived from it; `tab` is a view of its counts and tensors for outside readers.
        self.fams = {}
        self.tab = {}
        self.n_prop = {Pose2: 0, Point2: 0, Pose3: 0}
        dev = lambda a, dt: a if a is None or torch.is_tensor(a) else t(a, dt)

        def add(name, entry, vt_fixed, vt_target, dir_all, stream, targets, mu, L, rows4=None, alt=None, w=None, nh=None, in_step=True, partial=None):
            """alt / w / nh stay None unless the graph has them: the library picks its kernel from which pointers are null.
            partial: the 0-based coordinates of the target that the family's proposals solve (factors.partial_coverage), None = all"""
            rec = dict(name=name, entry=entry, fn=entry if plan_only else getattr(self._lib, entry), vt_fixed=vt_fixed, vt_target=vt_target,
                       dir_all=dir_all, stream=stream, n=len(targets), targets_h=np.asarray(targets, dtype=np.int32), mu=mu, L=L,
                       rows4=dev(rows4, i32), alt=dev(alt, i32), w=dev(w, f64), nh=dev(nh, f64), prop_lo=None, partial=partial)
            if in_step:   # (the PriorPose2 / PriorPose3 samplers are launchable but own no rows: their factors are rows of p2p2 / p3p3)
                rec["prop_lo"] = self.n_prop[vt_target]
                self.n_prop[vt_target] += rec["n"]
            self.fams[name] = rec
            return rec

        # relative factors: both directions interleaved, then one ROME_DIR_PRIOR row per prior factor, so a
        # whole-graph sweep of one variable family is a single launch
        def relative(name, entry, vt, stream, tab, ptab):
            d = vt.dim
            F, P = tab["F"], ptab["F"]
            if F == 0 and P == 0:
                return
            factor, dr, fixed, target = PackedGraph.conv_table(tab)
            mu = np.concatenate([tab["mu"].reshape(F, d), ptab["mu"].reshape(P, d)])
            cov = np.concatenate([tab["cov"].reshape(F, d, d), ptab["cov"].reshape(P, d, d)])
            factor = np.concatenate([factor, F + np.arange(P, dtype=np.int32)])
            dr = np.concatenate([dr, np.full(P, 2, dtype=np.int32)])
            fixed = np.concatenate([fixed, ptab["var"]]); target = np.concatenate([target, ptab["var"]])
            # multihypo factors (Pose2Pose2 over two candidates of the second pose): alternative / probability per row, and one
            # more row per such factor -- the proposal of the second candidate -- BEHIND the prior rows (rows 2f+dir and 2F+p keep
            # their meaning).  A table with hypotheses runs on the general kernel, one without on the lean one.
            hyp = PackedGraph.conv_hypotheses(tab)
            E = 0
            alt = w = None
            if hyp is not None:
                alt2, w2, ex = hyp
                E = len(ex["factor"])
                alt = np.concatenate([alt2, np.full(P, -1, np.int32), ex["alt"]]); w = np.concatenate([w2, np.ones(P), ex["w"]])
                factor = np.concatenate([factor, ex["factor"]]); dr = np.concatenate([dr, ex["dir"]])
                fixed = np.concatenate([fixed, ex["fixed"]]); target = np.concatenate([target, ex["target"]])
            # nullhypo=p factors: one probability per row (both directions and the extra row of the factor; prior rows 0)
            nhf = tab["nh"]
            nh = nh_or_none(np.concatenate([np.repeat(nhf, 2), np.zeros(P)] + ([nhf[ex["factor"]]] if E else [])))
            # rows4: the four table columns interleaved (one 16-byte scalar load per convolution; selects the lean kernel)
            rec = add(name, entry, vt, vt, 0, stream, target, t(mu, f64), t(cholesky_lower(cov), f64),
                      rows4=np.stack([factor, dr, fixed, target], axis=1), alt=alt, w=w, nh=nh)
            self.tab[name] = dict(F=F, P=P, E=E, C_rel=2 * F, C=rec["n"], mh=hyp is not None,
                                  **{k: rec[k] for k in ("rows4", "alt", "w", "nh")})

        def sampler(name, entry, vt, stream, tab, in_step=False):
            if tab["F"]:
                add(name, entry, None, vt, 0, stream, tab["var"], t(tab["mu"], f64), t(cholesky_lower(tab["cov"]), f64), in_step=in_step)

        def two_way(name, entry, vt, stream, tab, cls):
            """a relative family launched on its own: both directions of every factor interleaved in ONE record (conv_table), the same
            coordinates solved towards either variable.  Point2Point2Range: L = the [F][1] sigmas; the others: the packed Cholesky"""
            F, ranges = tab["F"], cls is Point2Point2Range
            if F:
                factor, dr, fixed, target = PackedGraph.range_conv_table(tab) if ranges else PackedGraph.conv_table(tab)
                add(name, entry, vt, vt, 0, stream, target, t(tab["mu"], f64), t(tab["sigma"] if ranges else cholesky_lower(tab["cov"]), f64),
                    rows4=np.stack([factor, dr, fixed, target], axis=1), nh=nh_or_none(np.repeat(tab["nh"], 2)), partial=partial_coverage(cls, 0))
                self.tab[name] = dict(C=2 * F) if ranges else dict(F=F, C=2 * F)

        def pose_point(name1, name0, entry, stream1, stream0, tab, key, cls):
            """a pose-to-point family of one scalar belief per factor (L = the [F][1] sigmas): dir 1 (landmark -> pose, variable 0 of the
            factor) then dir 0, two records over the same mu / sigma / nullhypo"""
            F = tab["F"]
            if F:
                fac = np.arange(F, dtype=np.int32)
                mu, sigma, nh = t(tab["mu"], f64), t(tab["sigma"], f64), dev(nh_or_none(tab["nh"]), f64)
                for name, d, stream, vf, vt, fx, tg in ((name1, 1, stream1, Point2, Pose2, tab["point"], tab["pose"]),
                                                        (name0, 0, stream0, Pose2, Point2, tab["pose"], tab["point"])):
                    add(name, entry, vf, vt, d, stream, tg, mu, sigma, rows4=np.stack([fac, col(d, F), fx, tg], axis=1), nh=nh,
                        partial=partial_coverage(cls, 1 - d))
                self.tab[key] = dict(F=F)

        col = lambda v, n: np.full(n, v, np.int32)
        nh_or_none = lambda nh: nh if np.any(nh > 0) else None
        relative("p2p2", "rome_conv_pose2pose2_dev", Pose2, self.STREAM_P2P2, pk.p2p2, pk.prior2)
        if pk.br["F"]:
            b, r0 = pk.br, pk.br["rows0"]
            F, F0 = b["F"], len(r0["factor"])
            mh = bool((b["alt"] >= 0).any())
            nhb = nh_or_none(b["nh"])
            mu, sigma = t(b["mu"], f64), t(b["sigma"], f64)
            br1 = add("br1", "rome_conv_pose2point2br_dev", Point2, Pose2, 1, self.STREAM_BR1, b["pose"], mu, sigma,
                      rows4=np.stack([np.arange(F, dtype=np.int32), col(1, F), b["point"], b["pose"]], axis=1),
                      alt=b["alt"] if mh else None, w=b["w"] if mh else None, nh=nhb)
            add("br0", "rome_conv_pose2point2br_dev", Pose2, Point2, 0, self.STREAM_BR0, r0["point"], mu, sigma,
                rows4=np.stack([r0["factor"], col(0, F0), r0["pose"], r0["point"]], axis=1),
                alt=r0["alt"] if mh else None, w=r0["w"] if mh else None, nh=None if nhb is None else nhb[r0["factor"]])
            self.tab["br"] = dict(F=F, F0=F0, mh=mh, nh=br1["nh"])
        sampler("priorpt2", "rome_sample_priorpoint2_dev", Point2, self.STREAM_PRIORPT2, pk.priorpt2, in_step=True)   # rows behind the sightings
        if "priorpt2" in self.fams:
            self.tab["priorpt2"] = dict(F=pk.priorpt2["F"])
        relative("p3p3", "rome_conv_pose3pose3_dev", Pose3, self.STREAM_P3P3, pk.p3p3, pk.prior3)
        # range-only factors (Range2D.jl): their own tables, launched after every other family; then the bearing-only factor (Bearing2D.jl)
        two_way("p2rng", "rome_conv_point2point2range_dev", Point2, self.STREAM_P2RNG, pk.p2rng, Point2Point2Range)
        pose_point("pprng1", "pprng0", "rome_conv_pose2point2range_dev", self.STREAM_PPRNG1, self.STREAM_PPRNG0, pk.pprng, "pprng", Pose2Point2Range)
        pose_point("pb1", "pb0", "rome_conv_pose2point2bearing_dev", self.STREAM_PB1, self.STREAM_PB0, pk.pbear, "pbear", Pose2Point2Bearing)
        sampler("prior2", "rome_sample_priorpose2_dev", Pose2, None, pk.prior2)
        sampler("prior3", "rome_sample_priorpose3_dev", Pose3, None, pk.prior3)
        # partial Pose3 factors (PartialPose3.jl): the last families, their proposal rows behind every other Pose3 row.  zrp3: prior rows
        # that READ the target belief (fixed = target, L = [F][4] = (σ_z, packed 2x2 Cholesky of the roll / pitch covariance))
        two_way("p3xyy", "rome_conv_pose3pose3xyyaw_dev", Pose3, self.STREAM_P3XYY, pk.p3xyy, Pose3Pose3XYYaw)
        zr = pk.zrp3
        if zr["F"]:
            F = zr["F"]
            L = np.concatenate([zr["sigma_z"].reshape(F, 1), cholesky_lower(zr["cov_rp"]).reshape(F, 3)], axis=1)
            add("zrp3", "rome_conv_priorpose3zrp_dev", Pose3, Pose3, 0, self.STREAM_ZRP3, zr["var"], t(zr["mu"], f64), t(L, f64),
                rows4=np.stack([np.arange(F, dtype=np.int32), col(0, F), zr["var"], zr["var"]], axis=1), nh=nh_or_none(zr["nh"]),
                partial=partial_coverage(PriorPose3ZRP, 0))
            self.tab["zrp3"] = dict(F=F)
        # p3rot: the last record, so a graph without it keeps its launches, rows and streams
        two_way("p3rot", "rome_conv_pose3pose3rotation_dev", Pose3, self.STREAM_P3ROT, pk.p3rot, Pose3Pose3Rotation)

        # one conv_step: the fused Pose2 / Point2 call for its three records when all three have rows, then every other record that
        # owns proposal rows, in list order
        step = [r for r in self.fams.values() if r["prop_lo"] is not None]
        fused = [self.fams[f] for f in ("p2p2", "br1", "br0") if f in self.fams and self.fams[f]["n"]]
        self._fused = fused if len(fused) == 3 else []
        self._unfused = [r for r in step if not any(r is f for f in self._fused)]

        # ---- proposal buffers + CSR (variable -> proposal rows) for the product / solve loop ----
        self.prop_bw = {}
        self.prop = {vt: torch.zeros((max(self.n_prop[vt], 1), vt.dim, self.N), dtype=f64, device=self.device) for vt in (Pose2, Point2, Pose3)}
        for r in step:   # the record's rows of prop[vt_target]: a view, made once (conv_step writes there)
            r["prop"] = self.prop[r["vt_target"]][r["prop_lo"]:r["prop_lo"] + r["n"]]
        self.bel_next = {vt: torch.zeros_like(self.bel[vt]) for vt in (Pose2, Point2, Pose3)}
        self._prop_targets = {vt: np.concatenate([np.zeros(0, np.int32)] + [r["targets_h"] for r in step if r["vt_target"] is vt])
                              for vt in (Pose2, Point2, Pose3)}
        self._prop_cover = {vt: [r["partial"] for r in step if r["vt_target"] is vt for _ in range(r["n"])] for vt in (Pose2, Point2, Pose3)}
        self.frozen = set()
        self._build_csr()

    def _build_csr(self):
        """variable -> proposal rows; frozen (marginalized) variables get no rows, so the product keeps their belief.  csr_full / tasks:
        the same for the partial-aware product (partial_tasks): the full rows alone, and the per-coordinate tasks of the partial ones."""
        pk = self.packed
        t = lambda a, dt: self.torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device=self.device)
        i32 = self.torch.int32
        self.csr, self.csr_full, self.tasks = {}, {}, {}
        for vt in (Pose2, Point2, Pose3):
            tg = np.asarray(self._prop_targets[vt], dtype=np.int64)
            nv = len(pk.labels[vt])
            live = np.ones(nv + 1, dtype=bool)
            if self.frozen:
                for i, l in enumerate(pk.labels[vt]):
                    if l in self.frozen:
                        live[i] = False
            rows = np.nonzero(live[tg])[0] if len(tg) else np.zeros(0, np.int64)
            order = rows[np.argsort(tg[rows], kind="stable")].astype(np.int32)
            ptr = np.zeros(nv + 1, dtype=np.int32)
            np.add.at(ptr, tg[rows] + 1, 1)
            ptr = np.cumsum(ptr).astype(np.int32)
            self.csr[vt] = dict(ptr=t(ptr, i32), rows=t(order if len(order) else np.zeros(1, np.int32), i32),
                                ptr_h=ptr, rows_h=order)
            pt = partial_tasks(ptr, order, self._prop_cover[vt], vt.dim)
            T = len(pt["task_var"])
            if T == 0:   # no partial rows: stage 1 IS the product of today, on the same tables
                self.csr_full[vt], self.tasks[vt] = self.csr[vt], dict(T=0, any_joint=False, host=pt)
                continue
            one = lambda a: t(a if len(a) else np.zeros(1, np.int32), i32)
            self.csr_full[vt] = dict(ptr=t(pt["full_ptr"], i32), rows=one(pt["full_rows"]), ptr_h=pt["full_ptr"], rows_h=pt["full_rows"])
            self.tasks[vt] = dict(T=T, any_joint=bool(pt["task_joint"].any()), host=pt,
                                  **{k: one(pt["task_" + k]) for k in ("var", "coord", "ptr", "rows", "joint")})

    def set_frozen(self, labels):
        """Fixed-lag operation (IIF `fifoFreeze!` / isMarginalized): the beliefs of `labels` are no longer updated by product_step /
        solve; they still serve as the fixed side of every convolution they take part in (test/testFixedLagFG.jl:86-121)."""
        labels = set(labels)
        known = set(self.packed.labels[Pose2]) | set(self.packed.labels[Point2]) | set(self.packed.labels[Pose3])
        if not labels <= known:
            raise KeyError("set_frozen: unknown variables %s" % sorted(labels - known))
        self.frozen = labels
        self._build_csr()

    # ---- one uniform view of the convolution tables (what the multi-GPU drivers plan launches from) ----
    RANK_FAMILIES = ("p2p2", "p3p3", "br1", "br0")

    def families(self, every=False):
        """Convolution families present in this graph: the ones the multi-rank drivers serve, or (every=True) the whole family
        list in launch order."""
        return list(self.fams) if every else [f for f in self.RANK_FAMILIES if f in self.fams]

    def family_table(self, fam):
        """-> the family's record: n, fn, vt_fixed, vt_target, dir_all, rows4 [n,4] int32 (factor, dir, fixed, target; None for the prior
        samplers), mu, L, alt, w, nh (None unless the graph has them), stream, targets_h, prop_lo, prop (its rows of self.prop)."""
        return self.fams[fam]

    # ---- belief store ----
    def upload_beliefs(self, fg):
        for vt in (Pose2, Point2, Pose3):
            if len(self.packed.labels[vt]):
                self.bel[vt].copy_(self.torch.as_tensor(self.packed.beliefs(fg, vt)))

    def _bind_stream(self):
        self.ctx.set_stream(self.torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _conv_dev(keep, **kw):
        """a rome_conv_dev descriptor from keywords (ints by value, tensors by address and appended to `keep`, None = null)"""
        cd = _lib.ConvDev()
        for k, v in kw.items():
            if k == "mirror_row":
                for m, r in enumerate(v):
                    cd.mirror_row[m] = int(r)
            elif isinstance(v, int):
                setattr(cd, k, v)
            elif v is not None:
                keep.append(v)
                setattr(cd, k, v.data_ptr())
        return cd

    def _plan(self, fn, opts, _ctx=None, **kw):
        """Pre-builds the rome_conv_dev descriptor once; the returned callable only binds the current
        torch stream and issues the launch (what a captured / replayed step calls).  `_ctx`: a Context whose stream the
        caller has fixed (one per pipeline slot) -- the launch then is a single C call with no stream lookup.  The callable's `.opts`
        is the options copy it launches with (a cached launch's stream offset is updated there)."""
        if self.plan_only:
            return _PlanStub(fn, opts, kw)
        keep = []
        cd = self._conv_dev(keep, **kw)
        o = _lib.Opts.from_buffer_copy(opts)
        ctx, check, cur = self.ctx, _lib.check, self.torch.cuda.current_stream
        h = ctx.handle
        po, pc = C.byref(o), C.byref(cd)

        if _ctx is not None:
            hf = _ctx.handle

            def launch_fixed():
                rc = fn(hf, po, pc)
                if rc:
                    check(rc, hf)
            launch_fixed._keep, launch_fixed.opts = (keep, o, cd, _ctx), o
            return launch_fixed

        def launch():
            ctx.set_stream(cur(self.device).cuda_stream)
            rc = fn(h, po, pc)
            if rc:
                check(rc, h)
        launch._keep, launch.opts = (keep, o, cd), o
        return launch

    def _conv_kw(self, rec, out, noise=None, status=None, rows=None):
        """the rome_conv_dev keywords of one family record (rows: a (lo, hi) slice of its table)"""
        cut = (lambda x: x) if rows is None else (lambda x: None if x is None else x[rows[0]:rows[1]])
        sampler = rec["vt_fixed"] is None
        return dict(n_conv=rec["n"] if rows is None else rows[1] - rows[0], dir_all=rec["dir_all"], rows4=cut(rec["rows4"]), mu=rec["mu"], L=rec["L"],
                    bel_fixed=None if sampler else self.bel[rec["vt_fixed"]], bel_target=None if sampler else self.bel[rec["vt_target"]],
                    alt_var=cut(rec["alt"]), hypo_w=cut(rec["w"]), nullhypo=cut(rec["nh"]), noise=noise, out=out, status=status)

    def _sweep(self, rec, opts, out=None, noise=None, status=None, rows=None, fixed_ctx=None, plan=False):
        """One launch of one family record -> its proposals [n, dim, N].  rows=(lo, hi): that slice of the table, row ids (Philox
        streams) kept.  plan=True: the pre-built launch (a callable) instead of launching."""
        if out is None:
            n = rec["n"] if rows is None else rows[1] - rows[0]
            out = self.torch.empty((n, rec["vt_target"].dim, self.N), dtype=self.torch.float64, device=self.device)
        if rows is not None:
            opts = self._opts_at(opts, rows[0])
        launch = self._plan(rec["fn"], opts, _ctx=fixed_ctx, **self._conv_kw(rec, out, noise, status, rows))
        if plan:
            return launch
        launch()
        return out

    def plan_sweep_pose2pose2(self, opts, out, noise=None, status=None, fixed_ctx=None):
        """fixed_ctx: a Context whose stream the caller has set once (Context.set_stream): the launch is then ONE C call, without the
        per-launch lookup of torch's current stream (5.4 -> ~2 us of host time per launch)"""
        return self._sweep(self.fams["p2p2"], opts, out, noise, status, fixed_ctx=fixed_ctx, plan=True)

    def plan_sample_priors(self, opts, out, kind="prior2", noise=None):
        return self._sweep(self.fams[kind], opts, out, noise, plan=True)

    # ---- solve loop pieces ----
    STREAM_P2P2, STREAM_BR1, STREAM_BR0, STREAM_PROD2, STREAM_PRODL, STREAM_P3P3, STREAM_PROD3, STREAM_PRIORPT2 = \
        0, 1 << 28, 2 << 28, 3 << 28, 4 << 28, 5 << 28, 6 << 28, 7 << 28
    STREAM_P2RNG, STREAM_PPRNG1, STREAM_PPRNG0 = 8 << 28, 9 << 28, 10 << 28   # range factors (Point2Point2Range, Pose2Point2Range dir 1 / 0)

    STREAM_PB1, STREAM_PB0 = 11 << 28, 12 << 28   # bearing-only factor (Pose2Point2Bearing dir 1 / 0)

    STREAM_P3XYY, STREAM_ZRP3 = 13 << 28, 14 << 28   # partial Pose3 factors (Pose3Pose3XYYaw both directions, PriorPose3ZRP)
    STREAM_P3ROT = (14 << 28) + (1 << 27)            # Pose3Pose3Rotation both directions: the upper half of zrp3's slot (every slot is taken)

    # stage 2 of the partial-aware product (task (v, c) draws base + v·dim + c): Pose2, Pose3.  15 << 28 is the last 28-bit slot below
    # the sweep field (sweep << 32), so the two bases share it, 2^27 streams each
    STREAM_PARTIAL2, STREAM_PARTIAL3 = 15 << 28, (15 << 28) + (1 << 27)

    def has_partial3(self):
        """does the graph hold partial Pose3 factors (served by conv_step / solve only: not by the multi-rank drivers)"""
        return "p3xyy" in self.tab or "zrp3" in self.tab or "p3rot" in self.tab

    def has_bearing(self):
        """does the graph hold bearing-only factors (served by conv_step / solve only: not by the multi-rank drivers)"""
        return "pbear" in self.tab

    def has_range(self):
        """does the graph hold range-only factors (served by conv_step / solve only: not by the multi-rank drivers)"""
        return "p2rng" in self.tab or "pprng" in self.tab

    def _opts_at(self, opts, offset):
        o = _lib.Opts.from_buffer_copy(opts)
        o.stream_offset = opts.stream_offset + offset
        return o

    def conv_step(self, opts, sweep=0):
        """All factor convolutions of the graph with the current beliefs -> self.prop (one launch per factor
        family/direction, in the order of the family list).  Philox streams: base + sweep·2³² + family offset + row."""
        base = sweep << 32
        if self._fused:   # a Pose2 / Point2 graph: ONE library call for the three families (one fused launch when the tables are plain)
            self.sweep_graph_pose2(self._opts_at(opts, base), *[r["prop"] for r in self._fused])
        for rec in self._unfused:
            self._sweep(rec, self._opts_at(opts, base + rec["stream"]), out=rec["prop"])

    def conv_plan(self, opts, sweep=0):
        """What conv_step(opts, sweep) launches, without launching (works on a plan-only graph): per launch the entry point, n_conv,
        dir_all, the absolute Philox stream_offset, where its rows go in prop[vt_target], which optional columns are non-null, and
        whether it is part of the fused Pose2 / Point2 call."""
        base = opts.stream_offset + (sweep << 32)
        return [dict(name=r["name"], entry=r["entry"], n_conv=r["n"], dir_all=r["dir_all"], stream_offset=base + r["stream"],
                     vt_target=r["vt_target"].name, prop_lo=r["prop_lo"], cols=[k for k in ("alt", "w", "nh") if r[k] is not None],
                     fused=k < len(self._fused))
                for k, r in enumerate(self._fused + self._unfused)]

    def product_step(self, opts, sweep=0, bandwidth="silverman", product="importance", gibbs_iters=1, partial_product="off"):
        """bel <- product of the proposals targeting each variable (Jacobi update: computed into bel_next, copied back in place
        so that launch plans holding the belief pointers stay valid).
        product:   "gibbs" = the reference's algorithm, ⚠AMP manifoldProduct / KDE.jl multiscale Gibbs sampling
                   (rome_product_gibbs_dev; Point2 / Pose2 / Pose3, N <= 256; always on the `manikde!` bandwidths of the proposals);
                   "importance" = the round-1 importance-sampling stand-in (rome_product_bw_dev).
        bandwidth: "silverman" (in-kernel rule on the proposal spread; importance product only) or "lcv" (leave-one-out
                   likelihood bandwidths of every proposal by rome_kde_bandwidth_dev first -- what the reference's `manikde!`
                   attaches to each convolution result).
        partial_product: "off" = every proposal row enters the product above as a full-dimensional density (the pass-through coordinates
                   of a partial factor's proposal then count as evidence for the current belief); "coordinate" = IIF's rule (DESIGN.md
                   §12d): the product above over the FULL rows only, then rome_product_partial_dev -- every coordinate that a partial
                   row covers becomes the 1-D importance product of the marginals covering it (and of the joint result, when the
                   variable has full rows); under "lcv" / "gibbs" on the manikde! bandwidths of those marginals.  A variable type
                   without partial rows launches the same under either setting."""
        if partial_product not in ("off", "coordinate"):
            raise ValueError("partial_product must be 'off' or 'coordinate'")
        if bandwidth not in ("silverman", "lcv"):
            raise ValueError("bandwidth must be 'silverman' or 'lcv'")
        if product not in ("importance", "gibbs"):
            raise ValueError("product must be 'importance' or 'gibbs'")
        self._bind_stream()
        base = sweep << 32
        for vt, dim, off in ((Pose2, 3, self.STREAM_PROD2), (Point2, 2, self.STREAM_PRODL), (Pose3, 6, self.STREAM_PROD3)):
            V = self.bel[vt].shape[0]
            if V == 0:
                continue
            o = self._opts_at(opts, base + off)
            tk = self.tasks[vt] if partial_product == "coordinate" else None
            c = self.csr_full[vt] if tk is not None and tk["T"] else self.csr[vt]
            bw_ptr = None
            rows = self.n_prop[vt]
            gibbs = product == "gibbs"
            circ = 0b100 if vt is Pose2 else (0b111000 if vt is Pose3 else 0)   # bandwidth rule: which coordinates are angles
            if (bandwidth == "lcv" or gibbs) and rows:
                if vt not in self.prop_bw:
                    self.prop_bw[vt] = self.torch.empty((self.prop[vt].shape[0], dim), dtype=self.torch.float64, device=self.device)
                _lib.check(self._lib.rome_kde_bandwidth_dev(self.ctx.handle, dim, rows, self.N, self.prop[vt].data_ptr(), circ, 0.0, 0.0,
                                                            self.prop_bw[vt].data_ptr()),
                           self.ctx.handle)
                bw_ptr = self.prop_bw[vt].data_ptr()
            if gibbs and rows:
                max_k = max(1, int(np.diff(c["ptr_h"]).max())) if len(c["ptr_h"]) > 1 else 1
                _lib.check(self._lib.rome_product_gibbs_dev(self.ctx.handle, C.byref(o), dim, V, c["ptr"].data_ptr(), c["rows"].data_ptr(),
                                                            self.prop[vt].data_ptr(), bw_ptr, rows, self.bel[vt].data_ptr(),
                                                            self.bel_next[vt].data_ptr(), 0b100 if vt is Pose2 else 0, int(gibbs_iters), max_k),
                           self.ctx.handle)   # (Pose3: rotations are handled in the chart of each proposal, no wrapped coordinate)
            else:
                _lib.check(self._lib.rome_product_bw_dev(self.ctx.handle, C.byref(o), dim, V, c["ptr"].data_ptr(), c["rows"].data_ptr(),
                                                         self.prop[vt].data_ptr(), bw_ptr, self.bel[vt].data_ptr(),
                                                         self.bel_next[vt].data_ptr()), self.ctx.handle)
            if tk is not None and tk["T"]:
                jbw_ptr = None
                if bw_ptr is not None and tk["any_joint"]:   # the joint result enters as a density of its own: its manikde! bandwidths
                    jbw = self.torch.empty((V, dim), dtype=self.torch.float64, device=self.device)
                    _lib.check(self._lib.rome_kde_bandwidth_dev(self.ctx.handle, dim, V, self.N, self.bel_next[vt].data_ptr(), circ, 0.0, 0.0,
                                                                jbw.data_ptr()), self.ctx.handle)
                    jbw_ptr = jbw.data_ptr()
                op = self._opts_at(opts, base + (self.STREAM_PARTIAL2 if vt is Pose2 else self.STREAM_PARTIAL3))
                _lib.check(self._lib.rome_product_partial_dev(self.ctx.handle, C.byref(op), dim, V, tk["T"], tk["var"].data_ptr(),
                                                              tk["coord"].data_ptr(), tk["ptr"].data_ptr(), tk["rows"].data_ptr(),
                                                              tk["joint"].data_ptr(), self.prop[vt].data_ptr(), bw_ptr, jbw_ptr, circ,
                                                              self.bel_next[vt].data_ptr()), self.ctx.handle)
            self.bel[vt].copy_(self.bel_next[vt])

    def solve(self, opts, n_sweeps=10, bandwidth="silverman", product="importance", gibbs_iters=1, partial_product="off"):
        """n_sweeps x (convolution sweep, product): whole-graph nonparametric inference, a Jacobi schedule in place of the
        clique-by-clique Gibbs of `solveTree!` (no Bayes tree)."""
        self.check_particle_limits(bandwidth, product)
        for s in range(n_sweeps):
            self.conv_step(opts, s)
            self.product_step(opts, s, bandwidth, product, gibbs_iters, partial_product)

    # ---- row-range forms of the two `next` stages, as the sharded drivers call them (rome_jl_amd.distributed) ----
    def kde_bandwidth_rows(self, dim, n_rows, prop, circ, bw_out):
        """manikde! bandwidths of `n_rows` proposal blocks (a contiguous device slice) -> bw_out [n_rows][dim]"""
        self._bind_stream()
        _lib.check(self._lib.rome_kde_bandwidth_dev(self.ctx.handle, dim, n_rows, self.N, prop.data_ptr(), circ, 0.0, 0.0, bw_out.data_ptr()),
                   self.ctx.handle)

    def product_gibbs_rows(self, opts, dim, V, ptr, rows, prop, bw, n_rows, bel_in, bel_out, circ, iters, max_k):
        """multiscale Gibbs product of V variables whose proposals are `rows` (CSR `ptr`) of the slice `prop` / `bw`"""
        self._bind_stream()
        _lib.check(self._lib.rome_product_gibbs_dev(self.ctx.handle, C.byref(opts), dim, V, ptr.data_ptr(), rows.data_ptr(), prop.data_ptr(),
                                                    bw.data_ptr(), n_rows, bel_in.data_ptr(), bel_out.data_ptr(), circ, iters, max_k),
                   self.ctx.handle)

    def check_particle_limits(self, bandwidth="silverman", product="importance"):
        """The stages of one solve iteration have different particle limits (include/rome_mi355.h): fail BEFORE the first launch,
        naming the stage, instead of part-way through an iteration."""
        N = self.N
        if product == "gibbs" and N > _lib.MAX_PARTICLES_GIBBS:
            raise ValueError("product='gibbs' (multiscale Gibbs product, the reference's manifoldProduct) takes N <= %d particles; this graph has "
                             "N = %d.  Use product='importance' (N <= %d) or fewer particles." % (_lib.MAX_PARTICLES_GIBBS, N, _lib.MAX_PARTICLES_PRODUCT))
        if (bandwidth == "lcv" or product == "gibbs") and N > _lib.MAX_PARTICLES_KDE:
            raise ValueError("manikde! bandwidths (bandwidth='lcv') take N <= %d particles; N = %d" % (_lib.MAX_PARTICLES_KDE, N))
        lim = _lib.MAX_PARTICLES_PRODUCT_POSE3 if self.bel[Pose3].shape[0] else _lib.MAX_PARTICLES_PRODUCT
        if product == "importance" and N > lim:
            raise ValueError("the importance product takes N <= %d particles here; N = %d (convolution sweeps alone go to %d)" % (lim, N, _lib.MAX_PARTICLES))

    def init_from_means(self, means, sigma=None, seed=3):
        """Beliefs = per-variable mean ⊕ N(0, diag σ²) jitter: e.g. means from solveGraphParametric (IIF can
        initialise the nonparametric solve from the parametric one: initParametricFrom!/autoinit)."""
        rng = np.random.default_rng(seed)
        for vt in (Pose2, Point2):
            ls = self.packed.labels[vt]
            if not ls:
                continue
            sg = np.asarray(sigma[vt] if sigma is not None else ([0.05, 0.05, 0.01] if vt is Pose2 else [0.1, 0.1]))
            m = np.stack([np.asarray(means[l], dtype=float) for l in ls])
            b = m[:, :, None] + sg[None, :, None] * rng.standard_normal((len(ls), vt.dim, self.N))
            self.bel[vt][:len(ls)].copy_(self.torch.as_tensor(b))
        ls = self.packed.labels[Pose3]
        if ls:   # Pose3: translation jitter added, rotation jitter composed on the right (R ← R Exp(e))
            from scipy.spatial.transform import Rotation as Rot
            sg = np.asarray(sigma[Pose3] if sigma is not None and Pose3 in sigma else [0.05, 0.05, 0.05, 0.01, 0.01, 0.01])
            m = np.stack([np.asarray(means[l], dtype=float) for l in ls])
            e = sg[None, :, None] * rng.standard_normal((len(ls), 6, self.N))
            b = np.empty_like(e)
            b[:, :3] = m[:, :3, None] + e[:, :3]
            for k in range(len(ls)):
                b[k, 3:] = (Rot.from_rotvec(m[k, 3:]) * Rot.from_rotvec(e[k, 3:].T)).as_rotvec().T
            self.bel[Pose3][:len(ls)].copy_(self.torch.as_tensor(b))

    def belief_stats(self, vartype):
        """(mean [V,dim], std [V,dim]) of every belief of one variable type, on device."""
        self._bind_stream()
        b = self.bel[vartype]
        V, d, N = b.shape
        mean = self.torch.empty((V, d), dtype=self.torch.float64, device=self.device)
        sd = self.torch.empty((V, d), dtype=self.torch.float64, device=self.device)
        _lib.check(self._lib.rome_belief_stats_dev(self.ctx.handle, d, V, N, b.data_ptr(), mean.data_ptr(), sd.data_ptr()), self.ctx.handle)
        return mean, sd

    def mmd(self, vartype, other, bw=0.001, scale=None, out=None):
        """[V] maximum mean discrepancies (AMP `mmd`, rome_mmd_dev) between every belief of one variable type and the same block of
        `other`, a device tensor shaped like self.bel[vartype] -- e.g. a clone taken before a sweep: how far the sweep moved each belief
        as a distribution.  scale: per-coordinate weights (host values) or None = ones.  One launch, no host synchronisation, capturable
        (pass `out` to keep the result outside the graph's memory pool)."""
        torch = self.torch
        b = self.bel[vartype]
        V, d, N = b.shape
        if tuple(other.shape) != (V, d, N) or other.dtype != torch.float64 or other.device != b.device or not other.is_contiguous():
            raise ValueError("DeviceGraph.mmd: `other` must be a contiguous float64 tensor of shape %s on %s" % ((V, d, N), b.device))
        if out is None:
            out = torch.empty((V,), dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != (V,) or out.dtype != torch.float64 or out.device != b.device or not out.is_contiguous():
            raise ValueError("DeviceGraph.mmd: `out` must be a contiguous float64 tensor of shape (%d,) on %s" % (V, b.device))
        sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
        if sc is not None and sc.shape != (d,):
            raise ValueError("DeviceGraph.mmd: scale must have %d entries" % d)
        self._bind_stream()
        _lib.check(self._lib.rome_mmd_dev(self.ctx.handle, d, V, N, b.data_ptr(), None, N, other.data_ptr(), None,
                                          None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_double)), float(bw), out.data_ptr(), None),
                   self.ctx.handle)
        return out

    # ---- deconvolution (rome_deconv_dev): each factor of a family ONCE, whichever of its `to` / `from` records is named ----
    # record name -> (packed table, record holding its mu / L, columns of the first / second variable, their types, ROME_DECONV_*, dz,
    # whether rome_mmd_dev serves the measurement manifold: dim 3 = SE(2) coordinates, dim 6 = SE(3) coordinates)
    _DECONV = {
        "p2p2": ("p2p2", "p2p2", "var_from", "var_to", Pose2, Pose2, _lib.DECONV_POSE2POSE2, 3, True),
        "br1": ("br", "br1", "pose", "point", Pose2, Point2, _lib.DECONV_POSE2POINT2BR, 2, False),
        "pb1": ("pbear", "pb1", "pose", "point", Pose2, Point2, _lib.DECONV_POSE2POINT2BEARING, 1, False),
        "p2rng": ("p2rng", "p2rng", "from", "to", Point2, Point2, _lib.DECONV_POINT2POINT2RANGE, 1, False),
        "pprng1": ("pprng", "pprng1", "pose", "point", Pose2, Point2, _lib.DECONV_POSE2POINT2RANGE, 1, False),
        "p3p3": ("p3p3", "p3p3", "var_from", "var_to", Pose3, Pose3, _lib.DECONV_POSE3POSE3, 6, True),
        "p3xyy": ("p3xyy", "p3xyy", "var_from", "var_to", Pose3, Pose3, _lib.DECONV_POSE3POSE3XYYAW, 3, True),
        "p3rot": ("p3rot", "p3rot", "var_from", "var_to", Pose3, Pose3, _lib.DECONV_POSE3POSE3ROTATION, 3, False),
    }
    _DECONV.update(br0=_DECONV["br1"], pb0=_DECONV["pb1"], pprng0=_DECONV["pprng1"])

    def _deconv_family(self, kind, who):
        if kind not in self.fams:
            raise KeyError("%s: the graph has no family record %r (it has %s)" % (who, kind, ", ".join(self.fams) or "none"))
        if kind not in self._DECONV:
            raise TypeError("%s: family %r holds prior rows; the deconvolution of a prior is the belief itself" % (who, kind))
        spec = self._DECONV[kind]
        tab = getattr(self.packed, spec[0])
        if "alt" in tab and (tab["alt"] >= 0).any():   # (the scalar-belief tables p2rng / pprng / pbear have no hypothesis columns)
            raise ValueError("%s: family %r has multihypo rows; a deconvolution pairs one first with one second variable" % (who, kind))
        return spec, tab

    def deconv_labels(self, kind):
        """the factor labels of DeviceGraph.deconv(opts, kind)'s rows, in row order"""
        return list(self._deconv_family(kind, "DeviceGraph.deconv_labels")[1]["labels"])

    def deconv(self, opts, kind, pred=None, meas=None):
        """rome_deconv_dev over the factors of the family record `kind` of self.fams, each factor once (row f = factor f of the family's
        table; the `to` and `from` records of a family name the same factors): -> (pred, meas), each [F, dz, N] on the device.
        pred[f] = the measurement that particle pair i of the factor's two beliefs predicts, meas[f] = the sample the convolution of
        stream opts.stream_offset + f draws (include/rome_mi355.h).  pred / meas: a tensor to write into, None to allocate one, False
        to skip that output.  One launch, no synchronisation, capturable (with both tensors passed).  Raises on a family of prior
        rows (TypeError) and on one with multihypo rows (ValueError)."""
        torch = self.torch
        (_, rname, ca, cb, vta, vtb, fam, dz, _), tab = self._deconv_family(kind, "DeviceGraph.deconv")
        if pred is False and meas is False:
            raise ValueError("DeviceGraph.deconv: one of pred / meas must be asked for")
        F = tab["F"]
        cache = self.__dict__.setdefault("_deconv_rows", {})
        if rname not in cache:
            rows = np.stack([np.arange(F, dtype=np.int32), np.zeros(F, np.int32), np.asarray(tab[ca], np.int32), np.asarray(tab[cb], np.int32)], axis=1)
            cache[rname] = torch.as_tensor(np.ascontiguousarray(rows), dtype=torch.int32, device=self.device)
        rows4, rec = cache[rname], self.fams[rname]
        outs = []
        for name, x in (("pred", pred), ("meas", meas)):
            if x is None:
                x = torch.empty((F, dz, self.N), dtype=torch.float64, device=self.device)
            elif x is not False and (tuple(x.shape) != (F, dz, self.N) or x.dtype != torch.float64 or x.device != self.device or not x.is_contiguous()):
                raise ValueError("DeviceGraph.deconv: `%s` must be a contiguous float64 tensor of shape %s on %s" % (name, (F, dz, self.N), self.device))
            outs.append(x)
        ptr = lambda x: None if x is None or x is False else x.data_ptr()
        t = _lib.DeconvTable(n_rows=F, rows4=rows4.data_ptr(), mu=rec["mu"].data_ptr(), L=rec["L"].data_ptr(), bel_a=self.bel[vta].data_ptr(),
                             bel_b=self.bel[vtb].data_ptr(), pred=ptr(outs[0]), meas=ptr(outs[1]))
        self._bind_stream()
        _lib.check(self._lib.rome_deconv_dev(self.ctx.handle, C.byref(opts), fam, C.byref(t)), self.ctx.handle)
        return tuple(None if x is False else x for x in outs)

    def factor_mmd(self, opts, kind, bw=0.001, out=None):
        """[F] consistency scores of the factors of family record `kind`: rome_mmd_dev between what each factor's two beliefs predict
        for its measurement and N samples of the measurement it carries (deconv, then mmd on the measurement manifold; the reference's
        test/testBasicPose2Conv.jl:51-56 accepts a factor at < 0.001).  A factor at odds with the solved beliefs -- a wrong loop
        closure -- stands out.  Two launches, no host round trip, capturable (pass `out`; the two [F, dz, N] work tensors are kept with
        the graph).  Families whose measurement manifold rome_mmd_dev does not serve (R, the circle, circle x R, SO(3): the range,
        bearing, bearing-range and rotation factors) raise TypeError."""
        torch = self.torch
        spec, tab = self._deconv_family(kind, "DeviceGraph.factor_mmd")
        rname, dz, ok = spec[1], spec[7], spec[8]
        if not ok:
            raise TypeError("DeviceGraph.factor_mmd: the measurement manifold of family %r (dz = %d) is not one rome_mmd_dev serves" % (kind, dz))
        F = tab["F"]
        buf = self.__dict__.setdefault("_deconv_buf", {})
        if rname not in buf:
            buf[rname] = tuple(torch.empty((F, dz, self.N), dtype=torch.float64, device=self.device) for _ in range(2))
        pred, meas = self.deconv(opts, kind, *buf[rname])
        if out is None:
            out = torch.empty((F,), dtype=torch.float64, device=self.device)
        elif tuple(out.shape) != (F,) or out.dtype != torch.float64 or out.device != self.device or not out.is_contiguous():
            raise ValueError("DeviceGraph.factor_mmd: `out` must be a contiguous float64 tensor of shape (%d,) on %s" % (F, self.device))
        _lib.check(self._lib.rome_mmd_dev(self.ctx.handle, dz, F, self.N, pred.data_ptr(), None, self.N, meas.data_ptr(), None, None, float(bw),
                                          out.data_ptr(), None), self.ctx.handle)
        return out

    def kde_bandwidths(self, vartype, tol_euclid=0.0, tol_circular=0.0):
        """[V, dim] leave-one-out likelihood bandwidths of every belief of one variable type (`manikde!` rule), on device."""
        self._bind_stream()
        b = self.bel[vartype]
        V, d, N = b.shape
        bw = self.torch.empty((V, d), dtype=self.torch.float64, device=self.device)
        _lib.check(self._lib.rome_kde_bandwidth_dev(self.ctx.handle, d, V, N, b.data_ptr(), 0b100 if vartype is Pose2 else 0,
                                                    float(tol_euclid), float(tol_circular), bw.data_ptr()), self.ctx.handle)
        return bw

    def logpdf(self, vartype, queries=None, bw=None, leave_one_out=False, out=None):
        """[V, Q] log-densities (rome_kde_eval_dev; api.kde_logpdf on store-resident beliefs) of every belief of one variable type at
        the Q points of the same block of `queries`, a device tensor [V][dim][Q]; None evaluates each belief at its own N particles, and
        leave_one_out then leaves each particle out of its own density.  bw: [V][dim] device tensor of kernel bandwidths, default
        self.kde_bandwidths(vartype).  No host round trip, capturable (pass `out` to keep the result outside the graph's memory pool)."""
        torch = self.torch
        b = self.bel[vartype]
        V, d, N = b.shape

        def ok(t, shape):
            return tuple(t.shape) == shape and t.dtype == torch.float64 and t.device == b.device and t.is_contiguous()
        if queries is not None and not (queries.dim() == 3 and ok(queries, (V, d, queries.shape[2]))):
            raise ValueError("DeviceGraph.logpdf: `queries` must be a contiguous float64 tensor of shape (%d, %d, Q) on %s" % (V, d, b.device))
        if leave_one_out and (queries is not None or N < 2):
            raise ValueError("DeviceGraph.logpdf: leave_one_out applies to self-evaluation (queries=None) of at least 2 particles")
        Q = N if queries is None else queries.shape[2]
        if bw is None:
            bw = self.kde_bandwidths(vartype)
        elif not ok(bw, (V, d)):
            raise ValueError("DeviceGraph.logpdf: `bw` must be a contiguous float64 tensor of shape %s on %s" % ((V, d), b.device))
        if out is None:
            out = torch.empty((V, Q), dtype=torch.float64, device=self.device)
        elif not ok(out, (V, Q)):
            raise ValueError("DeviceGraph.logpdf: `out` must be a contiguous float64 tensor of shape %s on %s" % ((V, Q), b.device))
        self._bind_stream()
        _lib.check(self._lib.rome_kde_eval_dev(self.ctx.handle, d, V, N, b.data_ptr(), None, bw.data_ptr(), Q,
                                               None if queries is None else queries.data_ptr(), None, 1 if leave_one_out else 0,
                                               out.data_ptr()), self.ctx.handle)
        return out

    def download_beliefs(self, fg):
        for vt in (Pose2, Point2, Pose3):
            h = self.bel[vt].cpu().numpy()
            for k, l in enumerate(self.packed.labels[vt]):
                fg.vals[l] = h[k].copy()

    def capture(self, fn, warmup=2):
        """Capture `fn` (a sequence of launches on the current stream) into a hipGraph; returns the
        torch.cuda.CUDAGraph (call .replay()).  Launch-bound inner loops (one sweep is ~10-20 µs of GPU
        time) are replayed without per-launch host cost."""
        torch = self.torch
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            for _ in range(warmup):
                fn()
        torch.cuda.current_stream(self.device).wait_stream(s)
        torch.cuda.synchronize(self.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fn()
        return g

    # ---- sweeps: one launch over one family's whole table ----
    def sweep_pose2pose2(self, opts, out=None, noise=None, status=None, conv_slice=None):
        """All (factor, direction) Pose2Pose2 convolutions (row 2f+dir) followed by the PriorPose2 rows (and one row per multihypo
        factor for its second candidate) -> proposals [2F+P+E, 3, N], one launch."""
        return self._sweep(self.fams["p2p2"], opts, out, noise, status, rows=conv_slice)

    def sweep_pose3pose3(self, opts, out=None, noise=None, status=None):
        return self._sweep(self.fams["p3p3"], opts, out, noise, status)

    def sweep_bearingrange(self, opts, direction, out=None, noise=None, status=None):
        """direction 0: poses -> landmark proposals [F0,2,N] (one row per (factor, candidate landmark));
        1: landmarks -> pose proposals [F,3,N].  Multihypo factors draw the landmark per particle."""
        return self._sweep(self.fams["br0" if direction == 0 else "br1"], opts, out, noise, status)

    def sweep_point2point2range(self, opts, out=None, noise=None, status=None):
        """Every Point2Point2Range factor in both directions (row 2f + dir: 0 solves lm from xi, 1 xi from lm) -> [2F, 2, N], one launch."""
        return self._sweep(self.fams["p2rng"], opts, out, noise, status)

    def sweep_pose2point2range(self, opts, direction, out=None, noise=None, status=None):
        """direction 0: poses -> landmark proposals [F, 2, N]; 1: landmarks -> pose proposals [F, 3, N] ((x, y) only, headings kept)."""
        return self._sweep(self.fams["pprng0" if direction == 0 else "pprng1"], opts, out, noise, status)

    def sweep_pose2point2bearing(self, opts, direction, out=None, noise=None, status=None):
        """direction 0: poses -> landmark proposals [F, 2, N] (on the sighting rays); 1: landmarks -> pose proposals [F, 3, N]
        (translations kept, headings turned to the bearing)."""
        return self._sweep(self.fams["pb0" if direction == 0 else "pb1"], opts, out, noise, status)

    def sweep_pose3pose3rotation(self, opts, out=None, noise=None, status=None):
        """Pose3Pose3Rotation rows, both directions interleaved -> proposals [2F, 6, N] ((ω_x, ω_y, ω_z) solved, the translation kept)."""
        return self._sweep(self.fams["p3rot"], opts, out, noise, status)

    def sweep_pose3pose3xyyaw(self, opts, out=None, noise=None, status=None):
        """Pose3Pose3XYYaw rows, both directions interleaved -> proposals [2F, 6, N] ((x, y, ω_z) solved, z, ω_x, ω_y kept)."""
        return self._sweep(self.fams["p3xyy"], opts, out, noise, status)

    def sweep_priorpose3zrp(self, opts, out=None, noise=None):
        """PriorPose3ZRP rows -> proposals [F, 6, N]: the variables' own particles with z, ω_x, ω_y replaced by the samples."""
        return self._sweep(self.fams["zrp3"], opts, out, noise)

    def sample_priors(self, opts, kind="prior2", out=None, noise=None):
        return self._sweep(self.fams[kind], opts, out, noise)

    def sweep_graph_pose2(self, opts, out_p2p2, out_br1, out_br0, family_offsets=None):
        """The whole convolution sweep of a Pose2 / Point2 graph in ONE library call (rome_sweep_pose2_dev): Pose2Pose2 + PriorPose2
        rows, bearing-range -> pose rows, bearing-range -> landmark rows.  Plain tables run as one fused launch; tables with multihypo
        columns take the per-family launches inside the library -- the proposals are the same bit for bit either way.
        family_offsets: Philox stream offsets of the three families (default: the records' own, STREAM_P2P2 / STREAM_BR1 / STREAM_BR0)."""
        keep = []
        recs = [self.fams[f] for f in ("p2p2", "br1", "br0")]
        cds = [self._conv_dev(keep, **self._conv_kw(r, out)) for r, out in zip(recs, (out_p2p2, out_br1, out_br0))]
        offs = (C.c_uint64 * 3)(*(family_offsets if family_offsets is not None else [r["stream"] for r in recs]))
        self._bind_stream()
        _lib.check(self._lib.rome_sweep_pose2_dev(self.ctx.handle, C.byref(opts), *[C.byref(cd) for cd in cds], offs), self.ctx.handle)
