"""What the two `solveTree` drivers (tree.TreeSolver, elimination.RelativeEliminationSolver) build their schedules from, host side only:
a LEVEL is one up-solve description (`LevelSpec`) over a level graph (`LevelGraph`: lifted labels and relabelled factors, every label
also a block of the solver's lifted universe), products with many proposals are staged (`split_products`), and `LevelSolver` owns what
both drivers do around their specs -- the universe, the store, the sharded backend view and the Philox offset of a plan run.
The module itself imports neither ctypes nor torch; `split_products` takes the sampled-measurement factor class of its identity rows
from `clique` when it is called (as it did in tree.py), and `clique` loads the library's ctypes layer."""
import numpy as np

from .factors import Pose2
from .graph import FactorGraph

ZERO = "0~"          # a block that stays zero: the samples of an identity row (split_products; the elimination's measurement rows)


class LevelSpec:
    """One tree level as ONE up-solve description over lifted labels:
      fg        FactorGraph holding the level's variables and (relabelled) factors -- what CliqueBatch / the oracle restatement consume
      cliques   per clique of the level: (update labels, their group numbers)
      order / groups / owner   the level's update list: group g of every clique together, groups in order; owner[k] = clique (position
                in the level) of entry k
      pairs     (factor, destination) rows in update order
      smsgs     (source label, destination label): store-resident messages, in destination order
      copies / anchors   block operations BEFORE the run: (source, destination) copies; (belief, destination) anchors (N copies of the mean)
      relatives          AFTER the run: (anchor block, separator block, destination): samples of anchor^-1 * separator"""

    def __init__(self, fg, cliques, pairs_of, smsgs, gibbs_iters, copies=(), anchors=(), relatives=()):
        self.fg, self.cliques, self.gibbs_iters = fg, cliques, gibbs_iters
        self.copies, self.anchors, self.relatives = list(copies), list(anchors), list(relatives)
        self.order, self.groups, self.owner = [], [], []
        for g in sorted({g for _, gs in cliques for g in gs}):
            for k, (upd, gs) in enumerate(cliques):
                for l, gl in zip(upd, gs):
                    if gl == g:
                        self.order.append(l); self.groups.append(g); self.owner.append(k)
        self.pairs = [(fl, l) for l in self.order for fl in pairs_of.get(l, ())]
        by_dest = {}
        for src, dst in smsgs:
            by_dest.setdefault(dst, []).append(src)
        self.smsgs = [(src, l) for l in self.order for src in by_dest.get(l, ())]


class LevelGraph(FactorGraph):
    """The graph of one level, bound to the solver's lifted universe: block indices in the store follow the universe's insertion order,
    so a label enters the universe the first time ANY level needs it."""

    def __init__(self, universe):
        FactorGraph.__init__(self, universe.N)
        self.universe = universe

    def need(self, label, vt):
        if label not in self.universe.variables:
            self.universe.addVariable(label, vt)
        if label not in self.variables:
            self.addVariable(label, vt)

    def lift(self, fl, cid, tag, labels, factor, src):
        """the factor `fl` of clique `cid` over lifted labels, with the hypotheses it carries in the graph `src`"""
        mh, nh = src.multihypo, getattr(src, "nullhypo", None)
        return self.putFactor("%s%s%d" % (fl, tag, cid), labels, factor, mh[fl] if fl in mh else None, nh[fl] if nh and fl in nh else None)


def split_products(L, cliques, pairs_of, smsgs, max_product):
    """staged products for Pose2 variables with more than max_product proposals (tree.TreeSolver docstring): a variable with K proposals
    is the root of a tree of partial products with fan-in <= max_product; a variable of update group g is solved in step
    g * (D + 1) + D, its partial products of depth d below it in step g * (D + 1) + D - d (D = the deepest tree of the level)"""
    from .clique import SampledPose2Pose2
    G = max_product
    by_dest = {}
    for src, dst in smsgs:
        by_dest.setdefault(dst, []).append(src)
    count = lambda l: len(pairs_of.get(l, ())) + len(by_dest.get(l, ()))     # noqa: E731

    def depth(k):
        d = 0
        while k > G:
            k = -(-k // G); d += 1
        return d
    D = max((depth(count(l)) for upd, _ in cliques for l in upd if L.variables[l] is Pose2), default=0) if G > 1 else 0
    if D == 0:
        return cliques, pairs_of, smsgs
    out_cliques, out_smsgs = [], []
    for upd, grp in cliques:
        nu, ng = [], []

        def build(l, items, g, lvl):
            """make `l` the product of `items` ((kind, id): a factor row, a store message, or a partial-product label) in step
            g * (D + 1) + D - lvl"""
            if len(items) > G and L.variables[l] is Pose2:
                nch = -(-len(items) // G)
                parts = []
                for k in range(nch):
                    pl = "%s^%d" % (l, k)
                    L.need(pl, Pose2)
                    build(pl, [(kind, x, l) for kind, x, _ in items[k::nch]], g, lvl + 1)
                    parts.append(("p", pl, l))
                items = parts
            rows = []
            for kind, x, owner in items:
                if kind == "f":          # a factor row of the ORIGINAL variable `owner`, retargeted to l
                    if owner == l:
                        rows.append(x)
                    else:
                        _, labels, f = L.getFactor(x)
                        rows.append(L.putFactor("%s>%s" % (x, l), [l if o == owner else o for o in labels], f,
                                                L.multihypo.get(x), L.nullhypo.get(x)))
                elif kind == "m":
                    out_smsgs.append((x, l))
                else:                    # a partial product enters through an identity row (sampled row whose samples are zero)
                    L.need(ZERO, Pose2)
                    rows.append(L.putFactor("=%s" % x, [x, l], SampledPose2Pose2(ZERO)))
            pairs_of[l] = rows
            nu.append(l); ng.append(g * (D + 1) + D - lvl)
        for l, g in zip(upd, grp):
            build(l, [("f", fl, l) for fl in pairs_of.get(l, ())] + [("m", src, l) for src in by_dest.get(l, ())], g, 0)
        out_cliques.append((nu, ng))
    return out_cliques, pairs_of, out_smsgs


class _ShardedPlans:
    """backend view whose Plan() returns a FrontierShard level plan (share up-solve + exchange + scatter); block operations unchanged"""

    def __init__(self, backend, make):
        self.backend, self.make = backend, make

    def Plan(self, store, spec):
        return self.make(spec)

    def BlockOp(self, store, op, entries):
        return self.backend.BlockOp(store, op, entries)


class LevelSolver:
    """What the tree solvers share around their level specs.  backend: object with Store(universe_fg) -> store (`.index`, `.put`,
    `.upload(fg)`, `.download(fg, labels)`), Plan(store, spec, share=None, mirror=None) -> `.run(opts)`, BlockOp(store, op, entries) ->
    `.run()`."""

    def _open_universe(self, fg, backend):
        """home blocks of every variable of fg, in graph order: the start of the lifted universe"""
        self.fg, self.N, self.backend = fg, fg.N, backend
        self.findex = {fl: (fl, ls, f) for fl, ls, f in fg.factors}
        self.universe = FactorGraph(fg.N)
        for l, vt in fg.variables.items():
            self.universe.addVariable(l, vt)
        self.runs = 0

    def _open_store(self, shard):
        """the store over the FINISHED universe (its ZERO block filled) -> the backend to build the plans through: itself, or (shard: a
        factory `store -> distributed.FrontierShard`) the view whose level plans are dealt to the ranks by clique"""
        U = self.universe
        self.store = self.backend.Store(U)
        if ZERO in U.variables:
            self.store.put(ZERO, np.zeros((U.variables[ZERO].dim, self.N)))
        self.shard = shard(self.store) if shard is not None else None
        if self.shard is None:
            return self.backend
        return _ShardedPlans(self.backend, lambda s: self.shard.plan_level(s, self.backend.Plan))

    def _run(self, plan, opts):
        o = type(opts).from_buffer_copy(opts)
        o.stream_offset = opts.stream_offset + (self.runs << 36)     # (it << 32) + family / product offsets stay below 2^36: run k draws from k << 36
        if self.shard is not None:
            self.shard.step(plan, o)
        else:
            plan.run(o)
        self.runs += 1

    def download(self, fg=None):
        """home blocks -> fg.vals (the posterior of every variable)"""
        self.store.download(fg or self.fg, labels=list(self.fg.variables))
