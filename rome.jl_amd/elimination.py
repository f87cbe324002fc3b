"""`solveTree!` for pose graphs as VARIABLE ELIMINATION IN RELATIVE-FACTOR ALGEBRA (`R.solveTree(fg, messages="elimination")`).

Why (round 6; docs/EXPERIMENTS.md, scripts/relative_elimination_surrogate.py, scripts/tree_gaussian_backend.py): the clique solves of
tree.TreeSolver are one-shot outward solves and their down pass multiplies proposals whose spread is the neighbours' ABSOLUTE spread --
the weights of a product then follow the (common, gauge-dominated) uncertainty of where the neighbours are instead of how tight each
factor is, and the solve stays at the quality of the init pass (measured on Manhattan-3500 against the converged MAP: init pass 0.8 /
tree solves 0.9 - 2.1 m after rigid alignment in the Gaussian restatement of the schedule; the exact elimination 0.18 m in ONE pass).
What an elimination needs is (a) the marginal over the neighbours of the eliminated variable and (b) the conditional of the variable
given its neighbours' VALUES.  For a pose graph both exist in sample form without any belief about where the poses are:

  edges     every factor between a and b is N samples of the relative pose a^-1 b (Pose2Pose2: mu + L xi; any SamplableBelief would do)
  merge     parallel edges between one pair multiply: the reference's `manifoldProduct` (manikde! bandwidths + multiscale Gibbs
            product) on the relative-pose samples
  eliminate v with neighbours u_1..u_m (edges z_k = v^-1 u_k): the pair marginal of (u_j, u_k) is EXACTLY the composition
            z_j^-1 (+) z_k, particle by particle (ROME_BLOCKOP_COMPOSE).  The dense marginal over the m neighbours is kept as a TREE
            (Chow-Liu node removal, as in pose-graph sparsification): the star about v's TIGHTEST neighbour c -- the minimum spanning
            tree when a pair costs spread(z_j) + spread(z_k).  m <= 2 is exact; the edge count never grows.
  order     rounds of independent (mutually non-adjacent) lowest-degree variables of the CURRENT graph, variables with priors last:
            every round is one product launch chain + one compose launch whatever the number of variables in it
  back      rounds in reverse: v = product over its neighbours of (mean of u_k) (+) z_k^-1 -- sampled-measurement convolutions from
            ANCHOR blocks (N copies of the neighbour's posterior mean: conditioning on the neighbours' values), multiplied by the
            reference's product.  A belief is therefore the conditional of a pose given its neighbours at their posterior means.

No init pass, no linearisation point, no iteration: a pass is a function of the seed.  `passes > 1` pool the particles of
independent passes (a belief is then a mixture over passes; its mean the running average).  Scope: Pose2 variables with Pose2Pose2 and
PriorPose2 factors (BASELINE configs[0-1]), or Pose3 variables with Pose3Pose3 and PriorPose3 factors (configs[4], SE3:QUAT g2o files);
no hypotheses, at least one prior, no mixed graphs; anything else -> tree.TreeSolver.  Structural decisions (which neighbour is tightest,
the order) are taken on the host from first-order covariances of the edges ("shadow"), once per graph.

The algorithm does not know the variable type: what depends on it is one small description per type (`_Pose2Kind`, `_Pose3Kind`) -- the
variable type of the ZERO / anchor / pool blocks, the sampled factor class, the anchor operation ("anchor" for Pose2; "anchor_mean" for
Pose3, whose "anchor" keeps the rotation of ONE particle) and the shadow arithmetic.  Pose3 products are not staged (`max_product` splits
Pose2 products only) and take N <= 256 (ROME_MAX_PARTICLES_PRODUCT_POSE3).  `solveTree(messages="auto")` chooses this form for Pose2
graphs only, as before (`covers(fg)`; `covers(fg, pose3=True)` is the constructor's predicate).

Reference: examples/ManhattanDatasetBatch.jl:43 (`tree = solveTree!(fg)`); the operations are the hot path's own
(sampled-measurement rows of `approxConvBelief`, `manikde!`, `manifoldProduct`)."""
import math

import numpy as np

from .levels import ZERO, LevelSpec, LevelGraph, LevelSolver, split_products
from .tree import DeviceBackend


def _inv(z):
    c, s = math.cos(z[2]), math.sin(z[2])
    return (-(c * z[0] + s * z[1]), -(-s * z[0] + c * z[1]), -z[2])


def _comp(a, b):
    c, s = math.cos(a[2]), math.sin(a[2])
    t = a[2] + b[2]
    return (a[0] + c * b[0] - s * b[1], a[1] + s * b[0] + c * b[1], math.atan2(math.sin(t), math.cos(t)))


class _Pose2Kind:
    """what the elimination needs to know about Pose2: block type, factor classes, anchor op, shadow arithmetic on (x, y, theta)"""
    name, dim, anchor_op, max_n = "Pose2", 3, "anchor", None
    inv, comp = staticmethod(_inv), staticmethod(_comp)

    def __init__(self):
        from .clique import SampledPose2Pose2
        from .factors import Pose2, Pose2Pose2, PriorPose2
        self.vt, self.between, self.prior, self.sampled = Pose2, Pose2Pose2, PriorPose2, SampledPose2Pose2

    @staticmethod
    def shadow(Z):
        """(mean, vt, vth) of a factor's measurement distribution"""
        C = Z.cov
        return ((float(Z.mu[0]), float(Z.mu[1]), float(Z.mu[2])), math.sqrt(max(float(C[0, 0] * C[1, 1] - C[0, 1] * C[1, 0]), 1e-300)), float(C[2, 2]))

    @staticmethod
    def t2(m):
        return m[0] * m[0] + m[1] * m[1]

    @staticmethod
    def spread(vt, vth):
        return (vt * vt * vth) ** (1.0 / 3.0)

    @staticmethod
    def merge(seen):
        """information-weighted mean of parallel edges [(mean, vt, vth)] -> (mean, vt, vth)"""
        m0 = seen[0][0]
        it = ith = hx = hy = hth = 0.0
        for m_, vt_, vth_ in seen:
            dth = m_[2] - m0[2]
            dth = math.atan2(math.sin(dth), math.cos(dth))
            it += 1.0 / vt_; ith += 1.0 / vth_
            hx += (m_[0] - m0[0]) / vt_; hy += (m_[1] - m0[1]) / vt_; hth += dth / vth_
        return (m0[0] + hx / it, m0[1] + hy / it, m0[2] + hth / ith), 1.0 / it, 1.0 / ith


def _rot(w):
    from scipy.spatial.transform import Rotation as Rot
    return Rot.from_rotvec(w).as_matrix()


def _rotlog(R):
    from scipy.spatial.transform import Rotation as Rot
    return Rot.from_matrix(R).as_rotvec()


class _Pose3Kind:
    """Pose3: the mean relative pose is a (t, R) pair; vt = det(S_tt)^(1/3), vth = det(S_ww)^(1/3) (isotropic variances with the determinant of
    the block); the lever arm |t|^2 vth enters an inverse / a composition as in 2-D; s = (vt^3 vth^3)^(1/6).  Plain float arithmetic."""
    name, dim, anchor_op = "Pose3", 6, "anchor_mean"

    def __init__(self):
        from . import _lib
        from .clique import SampledPose3Pose3
        from .factors import Pose3, Pose3Pose3, PriorPose3
        self.vt, self.between, self.prior, self.sampled = Pose3, Pose3Pose3, PriorPose3, SampledPose3Pose3
        self.max_n = _lib.MAX_PARTICLES_PRODUCT_POSE3

    @staticmethod
    def inv(m):
        return (-(m[1].T @ m[0]), m[1].T)

    @staticmethod
    def comp(a, b):
        return (a[0] + a[1] @ b[0], a[1] @ b[1])

    @staticmethod
    def shadow(Z):
        mu, C = np.asarray(Z.mu, dtype=float), np.asarray(Z.cov, dtype=float)
        return ((mu[:3].copy(), _rot(mu[3:])), max(float(np.linalg.det(C[:3, :3])), 1e-300) ** (1.0 / 3.0),
                max(float(np.linalg.det(C[3:, 3:])), 1e-300) ** (1.0 / 3.0))

    @staticmethod
    def t2(m):
        return float(m[0] @ m[0])

    @staticmethod
    def spread(vt, vth):
        return (vt ** 3 * vth ** 3) ** (1.0 / 6.0)

    @staticmethod
    def merge(seen):
        t0, R0 = seen[0][0]
        it = ith = 0.0
        ht, hw = np.zeros(3), np.zeros(3)
        for (t_, R_), vt_, vth_ in seen:
            it += 1.0 / vt_; ith += 1.0 / vth_
            ht += (t_ - t0) / vt_; hw += _rotlog(R0.T @ R_) / vth_
        return (t0 + ht / it, R0 @ _rot(hw / ith)), 1.0 / it, 1.0 / ith


class _Edge:
    """N samples of a^-1 b in store block `block`.  (m, vt, vth) = the SHADOW used for structural decisions only (which neighbour is
    tightest, what an elimination loses): mean relative pose, an isotropic translation variance and the heading variance, propagated to
    first order in plain float arithmetic (the lever arm |t|^2 * vth enters the translation variance of an inverse / a composition);
    s = (vt^2 vth)^(1/3), the geometric mean of the eigenvalues of diag(vt, vt, vth) (Pose3: of diag(vt x3, vth x3)).  K = the type's kind."""
    __slots__ = ("a", "b", "block", "m", "vt", "vth", "s", "_rev", "K")

    def __init__(self, a, b, block, m, vt, vth, K):
        self.a, self.b, self.block, self.m, self.vt, self.vth, self.K = a, b, block, m, vt, vth, K
        self.s = K.spread(vt, vth)
        self._rev = None

    def seen_from(self, v):
        """(mean, vt, vth) of v^-1 other"""
        if v == self.a:
            return self.m, self.vt, self.vth
        if self._rev is None:
            m = self.m
            self._rev = (self.K.inv(m), self.vt + self.K.t2(m) * self.vth, self.vth)
        return self._rev


class RelativeEliminationSolver(LevelSolver):
    """interface of tree.TreeSolver (upload / solve / download / stats / store); backend as there (device by default)"""

    def __init__(self, fg, backend=None, ctx=None, max_product=8, shard=None, loss_slack=1e9, loss_factor=1.0, priors_last=1, order_seed=0, structures=1, centre="tight", near_weight=0.0, mesh_max=0):
        from .factors import Pose3
        why = self.covers(fg, why=True, pose3=True)
        if why is not True:
            raise TypeError("messages='elimination' covers Pose2 graphs of Pose2Pose2 / PriorPose2 factors and Pose3 graphs of Pose3Pose3 / PriorPose3 "
                            "factors, without hypotheses (%s): use messages='relative' / 'marginal'" % why)
        K = self.kind = _Pose3Kind() if next(iter(fg.variables.values()), None) is Pose3 else _Pose2Kind()
        if K.max_n is not None and fg.N > K.max_n:
            raise ValueError("the %s product takes N <= %d particles (ROME_MAX_PARTICLES_PRODUCT_POSE3); fg.N = %d" % (K.name, K.max_n, fg.N))
        VT = K.vt            # (the one variable type of the graph, of the ZERO / anchor / pool blocks)
        self.messages = "elimination"
        self.max_product = int(max_product or 0)
        self.loss_slack, self.loss_factor, self.priors_last = float(loss_slack), float(loss_factor), bool(priors_last)
        self.order_seed = int(order_seed)
        self.centre = centre
        self.near_weight = float(near_weight)
        self.mesh_max = int(mesh_max)
        self._open_universe(fg, backend or DeviceBackend(ctx))
        U = self.universe
        U.addVariable(ZERO, VT)
        self.VT = VT
        for l in list(fg.variables):
            U.addVariable(l + "^", VT)          # anchor block: N copies of the posterior mean
            U.addVariable(l + "&", VT)          # pool block: the mixture over the passes so far (solve(passes > 1))
        from .graph import gc_paused
        self.structures = max(1, int(structures))
        with gc_paused():     # (~1e6 live small objects, nothing to free: the generation scans cost a third of the build)
            self._build(fg, shard)
        self._to_pool = self.backend.BlockOp(self.store, "copy", [(l, l + "&") for l in fg.variables])
        self._mix = {}
        self.passes_pooled = 0

    def _build(self, fg, shard):
        import time
        t0 = time.perf_counter()
        schedules = [self._structure(k) for k in range(self.structures)]
        self.schedules = schedules
        t1 = time.perf_counter()
        B = self._open_store(shard)
        self.steps = []
        for sched in schedules:
            st = []
            for kind, x in sched:
                st.append(("plan", B.Plan(self.store, x)) if kind == "plan" else ("op", B.BlockOp(self.store, kind, x)))
            self.steps.append(st)
        self.build_s = dict(structure=t1 - t0, store_and_plans=time.perf_counter() - t1)

    @staticmethod
    def covers(fg, why=False, pose3=False):
        """True when the graph is in this solver's scope (else False, or the reason with why=True).  pose3=False (what solveTree's
        messages="auto" asks): the Pose2 scope only; pose3=True (what the constructor asks): an all-Pose3 graph of Pose3Pose3 / PriorPose3
        factors is in scope too."""
        from .factors import Pose2, Pose2Pose2, PriorPose2, Pose3, Pose3Pose3, PriorPose3
        if pose3 and fg.variables and next(iter(fg.variables.values())) is Pose3:
            Pose2, Pose2Pose2, PriorPose2 = Pose3, Pose3Pose3, PriorPose3
        bad = None
        for l, vt in fg.variables.items():
            if vt is not Pose2:
                bad = "variable %s is %s" % (l, getattr(vt, "__name__", type(vt).__name__.lstrip("_"))); break
        if bad is None:
            for fl, ls, f in fg.factors:
                if not isinstance(f, (Pose2Pose2, PriorPose2)) or fl in fg.multihypo or fl in getattr(fg, "nullhypo", {}):
                    bad = "factor %s" % fl; break
        if bad is None and not any(isinstance(f, PriorPose2) for _, _, f in fg.factors):
            bad = "no prior"
        return (True if bad is None else bad) if why else bad is None

    # ------------------------------------------------------------------------------------------------ structure (host, once per graph)
    def _spec(self, L, entries, smsgs=()):
        """entries: [(destination label, [factor labels])] -> a one-group LevelSpec (every destination its own 'clique': a level is dealt
        to the ranks by variable), two-stage products where a destination has more than max_product proposals"""
        cliques = [([l], [0]) for l, _ in entries]
        pairs_of = {l: list(rows) for l, rows in entries}
        return LevelSpec(L, *split_products(L, cliques, pairs_of, list(smsgs), self.max_product), 1)

    def _loss(self, v, adj):
        """what eliminating v NOW costs, and the centre of its star: the star about neighbour c replaces the pair (j, k) of spread
        s_j + s_k by the path j - c - k of spread s_j + s_k + 2 s_c; summed relative loss of information over the dropped pairs,
        discounted where the pair already has a direct edge (scalar spreads of the shadow covariances).  c = the neighbour with the
        smallest loss (centre="loss") or the tightest one (centre="tight").  Degree <= 2: exact, loss 0.  -> (loss, c)"""
        nb = adj[v]
        s = {u: (es[0].s if len(es) == 1 else 1.0 / sum(1.0 / e.s for e in es)) for u, es in nb.items()}
        if not s:
            return 0.0, None
        tight = min(s, key=lambda u: (s[u], self._pos[u]))
        if len(nb) <= max(2, self.mesh_max):
            return 1e-9 * (len(nb) > 2), tight
        us = list(s)
        ex = {}
        for a in range(len(us)):
            for b in range(a + 1, len(us)):
                es = adj[us[a]].get(us[b])
                ex[(a, b)] = sum(1.0 / e.s for e in es) if es else 0.0
        best = None
        for ci in (range(len(us)) if self.centre == "loss" else [us.index(tight)]):
            sc, tot = s[us[ci]], 0.0
            for a in range(len(us)):
                if a == ci:
                    continue
                for b in range(a + 1, len(us)):
                    if b == ci:
                        continue
                    sj = s[us[a]] + s[us[b]]
                    it = 1.0 / sj
                    tot += (it - 1.0 / (sj + 2 * sc)) / (it + ex[(a, b)])
            if best is None or (tot, self._pos[us[ci]]) < (best[0], self._pos[best[1]]):
                best = (tot, us[ci])
        return best

    def _structure(self, k_struct=0):
        fg, VT = self.fg, self.VT
        K = self.kind
        Prior, Sampled, _inv, _comp = K.prior, K.sampled, K.inv, K.comp
        U = self.universe
        n_edge = [0]

        def new_block(prefix):
            l = "%s%d.%d~" % (prefix, k_struct, n_edge[0]); n_edge[0] += 1
            U.addVariable(l, VT)
            return l

        adj = {v: {} for v in fg.variables}            # v -> {u: [edges]}
        unary = {v: [] for v in fg.variables}          # v -> [blocks of ABSOLUTE samples of v]: priors, and priors transported along edges
        sched = []
        # ---- step 0: the samples of every factor's measurement (a row from the ZERO block: 0 (+) z = z; a prior: its own row), ONE launch chain
        L = LevelGraph(U); L.need(ZERO, VT)
        ent = []
        for fl, ls, f in fg.factors:
            if isinstance(f, Prior):
                blk = new_block("p")
                L.need(blk, VT)
                ent.append((blk, [L.lift(fl, 0, "p", [blk], f, fg)]))
                unary[ls[0]].append(blk)
                continue
            a, b = ls
            blk = new_block("e")
            L.need(blk, VT)
            ent.append((blk, [L.putFactor("s:" + fl, [ZERO, blk], f)]))
            e = _Edge(a, b, blk, *K.shadow(f.Z), K)
            adj[a].setdefault(b, []).append(e); adj[b].setdefault(a, []).append(e)
        pri = {v for v in fg.variables if unary[v]}
        if not pri:
            raise ValueError("the graph holds no prior: it has no gauge")
        sched.append(("plan", self._spec(L, ent)))
        self.n_factor_edges = len(ent) - sum(len(u) for u in unary.values())
        # ---- rounds
        alive = set(fg.variables)
        hold = set(pri) if self.priors_last else set()
        pos = {v: k for k, v in enumerate(fg.variables)}
        if self.order_seed or k_struct:   # another tie-break among equal losses / degrees: another structure, another set of approximations
            perm = np.random.default_rng(self.order_seed + 7919 * k_struct).permutation(len(pos))
            pos = {v: int(perm[k]) for v, k in pos.items()}
        self._pos = pos
        dist = {v: 0.0 for v in fg.variables}
        if self.near_weight:      # hops to the nearest prior variable, scaled to [0, 1]
            from collections import deque
            dq = deque(pri); seen = {v: 0 for v in pri}
            while dq:
                v = dq.popleft()
                for u in adj[v]:
                    if u not in seen:
                        seen[u] = seen[v] + 1; dq.append(u)
            mx = max(seen.values()) or 1
            dist = {v: seen.get(v, mx) / mx for v in fg.variables}
        rounds, down = [], []
        n_merge = n_comp = n_approx = n_transport = 0

        def identity_rows(Lx, dst, blocks, flip=()):
            """rows that re-emit the samples of `blocks` as proposals of `dst` (0 (+) z = z; flipped: 0 (-) z = z^-1)"""
            rows = []
            for k, blk in enumerate(blocks):
                Lx.need(blk, VT)
                rows.append(Lx.putFactor("g:%s:%d" % (dst, k), [dst, ZERO] if k in flip else [ZERO, dst], Sampled(blk)))
            return rows

        while alive:
            pool = (alive - hold) or alive
            lc = {v: self._loss(v, adj) for v in pool}
            loss = {v: x[0] for v, x in lc.items()}
            cand = sorted(pool, key=lambda v: (loss[v] + self.near_weight * dist[v], len(adj[v]), pos[v]))
            sel, blocked = [], set()
            cap = loss[cand[0]] * self.loss_factor + self.loss_slack
            for v in cand:
                if loss[v] > cap:
                    break
                if v in blocked:
                    continue
                if not adj[v] and not unary[v]:
                    raise ValueError("variable %s is not connected to a prior" % v)
                sel.append(v); blocked.add(v); blocked.update(adj[v])
            Lm = LevelGraph(U); Lm.need(ZERO, VT)
            Lt = LevelGraph(U)
            merges, transports, comps, dn = [], [], [], []
            for v in sel:
                nb = {}
                for u, es in adj[v].items():
                    if len(es) > 1:     # parallel edges -> one: product of their samples, all seen from v
                        blk = new_block("m")
                        Lm.need(blk, VT)
                        mm, mvt, mvth = K.merge([e.seen_from(v) for e in es])
                        merges.append((blk, identity_rows(Lm, blk, [e.block for e in es], flip={k for k, e in enumerate(es) if e.a != v})))
                        n_merge += 1
                        nb[u] = _Edge(v, u, blk, mm, mvt, mvth, K)
                    else:
                        nb[u] = es[0]
                if len(unary[v]) > 1:   # several absolute beliefs of v -> one
                    blk = new_block("q")
                    Lm.need(blk, VT)
                    merges.append((blk, identity_rows(Lm, blk, unary[v]))); n_merge += 1
                    unary[v] = [blk]
                for u in nb:
                    del adj[u][v]
                if nb and 2 < len(nb) <= self.mesh_max:
                    # STAR-MESH transform (Kron reduction): the marginal of a star with leg variances v_k is EXACTLY (commuting case) the
                    # full mesh whose edge (j, k) has the composed mean and the variance v_j + v_k + v_j v_k sum_{i != j,k} 1 / v_i --
                    # the composition's own spread, inflated by what the pair shares with the other legs
                    us = list(nb)
                    seen = {u: nb[u].seen_from(v) for u in us}
                    it_all = sum(1.0 / seen[u][1] for u in us); ith_all = sum(1.0 / seen[u][2] for u in us)
                    for ai in range(len(us)):
                        for bi in range(ai + 1, len(us)):
                            j, k = us[ai], us[bi]
                            zj, vtj, vthj = seen[j]; zk, vtk, vthk = seen[k]
                            zi = _inv(zj); vti = vtj + K.t2(zj) * vthj
                            vt0 = vti + vtk + K.t2(zk) * vthj
                            vth0 = vthj + vthk
                            gt = 1.0 + vtj * vtk * (it_all - 1.0 / vtj - 1.0 / vtk) / (vtj + vtk)
                            gth = 1.0 + vthj * vthk * (ith_all - 1.0 / vthj - 1.0 / vthk) / (vthj + vthk)
                            blk = new_block("c")
                            e = _Edge(j, k, blk, _comp(zi, zk), vt0 * gt, vth0 * gth, K)
                            comps.append((nb[j].block, nb[k].block, blk, nb[j].a == v, nb[k].a != v, math.sqrt(gt), math.sqrt(gth)))
                            adj[j].setdefault(k, []).append(e); adj[k].setdefault(j, []).append(e)
                            n_comp += 1
                elif nb:
                    # tightest neighbour: smallest log det of the covariance of v^-1 u
                    c = lc[v][1]
                    zi, vti, vthi = nb[c].seen_from(c)             # c^-1 v
                    for k, ek in nb.items():
                        if k == c:
                            continue
                        zk, vtk, vthk = ek.seen_from(v)
                        blk = new_block("c")
                        e = _Edge(c, k, blk, _comp(zi, zk), vti + vtk + K.t2(zk) * vthi, vthi + vthk, K)
                        # c^-1 k = (v^-1 c)^-1 (+) (v^-1 k): invert the block of c when it holds v^-1 c, the block of k when it holds k^-1 v
                        comps.append((nb[c].block, ek.block, blk, nb[c].a == v, ek.a != v))
                        adj[c].setdefault(k, []).append(e); adj[k].setdefault(c, []).append(e)
                        n_comp += 1
                    if unary[v]:        # the absolute belief of v travels to c: p(c) = p(v) (+) z_c -- a convolution of BELIEF samples
                        blk, pv, ec = new_block("a"), unary[v][0], nb[c]
                        for l in (blk, pv, ec.block):
                            Lt.need(l, VT)
                        transports.append((blk, [Lt.putFactor("t:%s" % blk, [pv, blk] if ec.a == v else [blk, pv], Sampled(ec.block))]))
                        unary[c].append(blk); n_transport += 1
                    n_approx += len(nb) > 2
                dn.append((v, list(nb.items()), list(unary[v])))
                del adj[v]
            if merges:
                sched.append(("plan", self._spec(Lm, merges)))
            if transports:
                sched.append(("plan", self._spec(Lt, transports)))
            if comps:
                sched.append(("compose", comps))
            rounds.append(len(sel)); down.append(dn)
            alive -= set(sel)
        # ---- back substitution: rounds in reverse; a variable = product of its own absolute beliefs (store-resident messages) and the
        #      sampled-measurement convolutions from its neighbours' ANCHOR blocks
        anchor = lambda v: v + "^"     # noqa: E731
        anchored = set()
        for dn in reversed(down):
            Ld = LevelGraph(U)
            need, ent, sm = [], [], []
            for v, nbs, un in dn:
                Ld.need(v, VT)
                rows = []
                for u, e in nbs:
                    if u not in anchored:
                        anchored.add(u); need.append((u, anchor(u)))
                    for l in (anchor(u), e.block):
                        Ld.need(l, VT)
                    rows.append(Ld.putFactor("d:%s:%s:%s" % (v, u, e.block), [v, anchor(u)] if e.a == v else [anchor(u), v], Sampled(e.block)))
                for blk in un:
                    Ld.need(blk, VT)
                    sm.append((blk, v))
                ent.append((v, rows))
            if need:
                sched.append((K.anchor_op, need))
            sched.append(("plan", self._spec(Ld, ent, sm)))
        self.rounds = rounds
        self._stats = dict(rounds=len(rounds), round_sizes=rounds[:16], merges=n_merge, compositions=n_comp, transports=n_transport,
                           approximated_eliminations=n_approx, factor_edges=self.n_factor_edges, prior_variables=len(pri), blocks=len(U.variables),
                           launch_steps=len(sched), plan_steps=sum(1 for k, _ in sched if k == "plan"), structures=self.structures)
        return sched

    # ------------------------------------------------------------------------------------------------ the solve
    def upload(self, fg=None):
        """(nothing to upload: the solve starts from the factors alone; present so that solveTree treats every solver alike)"""

    def solve(self, opts, passes=1):
        """passes > 1 (and repeated calls): independent passes -- other Philox streams, the next of the `structures` -- POOLED: after pass p
        a belief holds ~N / p particles of every pass so far (ROME_BLOCKOP_MIX), its mean is the running average.  reset() starts over."""
        for _ in range(passes):
            if self.shard is not None:
                self.shard.bind_stream()
            p = self.passes_pooled + 1
            if p > 1:
                self._to_pool.run()
            for kind, x in self.steps[(p - 1) % self.structures]:
                if kind == "plan":
                    self._run(x, opts)
                else:
                    x.run()
            if p > 1:
                if p not in self._mix:
                    self._mix[p] = self.backend.BlockOp(self.store, "mix", [(l + "&", l, p) for l in self.fg.variables])
                self._mix[p].run()
            self.passes_pooled = p

    def reset(self):
        self.passes_pooled = 0

    def stats(self):
        return dict(self._stats, messages=self.messages, build_s=self.build_s)
