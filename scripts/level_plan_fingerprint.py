"""Fingerprint of everything the host layer of `solveTree` hands to a backend, without a device: the solvers are built over a RECORDING
backend (its store only numbers the blocks per type, as `DeviceStore.index` does; `Plan` and `BlockOp` append to a log) and every step of
the log is reduced to a short digest -- per plan step the level graph (variables in insertion order, factors, hypotheses) and the whole
LevelSpec, per block-operation step the operation and its entries -- plus one digest of the lifted universe.  Lifted labels, row order
(hence Philox stream ids) and block indices (universe insertion order) all enter, so equal digests mean equal plan tables.

    python scripts/level_plan_fingerprint.py [out.json]      -> {case: [digest per step ..., digest of the universe]}

tests/golden/level_plans.json is this output at the commit BEFORE the level-plan refactor (levels.py); tests/test_level_plans_pinned.py
rebuilds every case and names the first step that differs."""
import functools
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import rome_jl_amd as R   # noqa: E402
from rome_jl_amd.elimination import RelativeEliminationSolver   # noqa: E402
from rome_jl_amd.tree import TreeSolver   # noqa: E402

N = 100


def _tname(vt):
    return getattr(vt, "__name__", type(vt).__name__)


def _digest(x):
    return hashlib.sha256(repr(x).encode()).hexdigest()[:12]


def _variables(fg):
    return [(l, _tname(vt)) for l, vt in fg.variables.items()]


class RecordingStore:
    def __init__(self, universe):
        self.fg, self.N, self.index = universe, universe.N, {}
        cnt = {}
        for l, vt in universe.variables.items():
            self.index[l] = cnt.get(vt, 0); cnt[vt] = cnt.get(vt, 0) + 1

    def put(self, label, pts):
        pass


class RecordingBackend:
    def __init__(self):
        self.log, self.universe = [], None

    def Store(self, universe):
        self.universe = universe
        return RecordingStore(universe)

    def Plan(self, store, spec, share=None, mirror=None):
        L = spec.fg
        self.log.append(("plan", _variables(L), [(fl, list(ls), type(f).__name__, getattr(f, "meas", None)) for fl, ls, f in L.factors],
                         sorted(L.multihypo.items()), sorted(L.nullhypo.items()), spec.cliques, spec.order, spec.groups, spec.owner, spec.pairs,
                         spec.smsgs, spec.gibbs_iters, spec.copies, spec.anchors, spec.relatives))
        return len(self.log)

    def BlockOp(self, store, op, entries):
        self.log.append(("op", op, [tuple(e) for e in entries]))
        return len(self.log)

    def digests(self):
        return [_digest(step) for step in self.log] + [_digest(_variables(self.universe))]


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "m3500":
        return R.loadG2o(os.path.join(ROOT, "tests", "golden", "manhattan.g2o"), N=N)
    if name == "hex":
        return R.generateGraph_Hexagonal(N=N)
    if name == "mitbr":
        return R.synth_mit_br(P=200, n_landmarks=30, N=N)
    if name == "beehive":
        return R.synth_beehive_mh(poseCountTarget=36, N=N)
    if name == "helix":
        return R.synth_helix3d(P=200, N=N)
    raise KeyError(name)


HOP_SWEEPS = dict(messages="relative", message_tree="hop", rootIters=1, refineIters=1, relIters=1, max_product=4)
CASES = {   # case -> (graph, solver class, keywords)
    "m3500_marginal": ("m3500", TreeSolver, dict(messages="marginal")),
    "m3500_relative": ("m3500", TreeSolver, dict(messages="relative")),
    "m3500_relative_hop_sweeps": ("m3500", TreeSolver, HOP_SWEEPS),
    "m3500_elimination_structures2": ("m3500", RelativeEliminationSolver, dict(structures=2)),
    "m3500_elimination_mesh4": ("m3500", RelativeEliminationSolver, dict(mesh_max=4)),
    "hex_marginal": ("hex", TreeSolver, dict(messages="marginal")),
    "hex_relative": ("hex", TreeSolver, dict(messages="relative")),
    "mitbr_marginal": ("mitbr", TreeSolver, dict(messages="marginal")),
    "mitbr_relative": ("mitbr", TreeSolver, dict(messages="relative")),
    "mitbr_relative_hop": ("mitbr", TreeSolver, dict(messages="relative", message_tree="hop", relIters=1)),
    "beehive_marginal": ("beehive", TreeSolver, dict(messages="marginal")),
    "beehive_relative": ("beehive", TreeSolver, dict(messages="relative")),
    "helix_marginal": ("helix", TreeSolver, dict(messages="marginal")),
    "helix_relative": ("helix", TreeSolver, dict(messages="relative")),
    "helix_elimination_structures2": ("helix", RelativeEliminationSolver, dict(structures=2)),
}


def build(case, backend=None):
    """the solver of `case` over a recording backend -> (solver, backend)"""
    g, cls, kw = CASES[case]
    backend = backend or RecordingBackend()
    return cls(graph(g), backend=backend, **kw), backend


def fingerprint(case):
    return build(case)[1].digests()


if __name__ == "__main__":
    out = {case: fingerprint(case) for case in CASES}
    text = json.dumps(out, indent=0, sort_keys=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    print("\n".join("%-32s %5d steps  %s" % (c, len(d) - 1, _digest(d)) for c, d in out.items()))
