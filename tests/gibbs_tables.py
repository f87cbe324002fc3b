"""Input tables of the multiscale Gibbs product (rome_product_gibbs_dev) whose output bytes are recorded in
tests/golden/gibbs_bits.json (scripts/gibbs_bits.py writes it, tests/test_gpu_gibbs.py compares).  numpy only, fixed seeds, bandwidths
drawn uniformly in [0.05, 0.4]: the tables depend on no library build.  The shapes are the smallest at which the kernels can still go
wrong, not the workload's:

  shapes D=.. circ=..   one family per instantiation (D, circular mask) of k_product_gibbs, every N of SHAPE_N: N = 1 has no tree
                        level (L = 0), 2 has one, 3 an odd leaf pair, 128 is the last N of the 128-slot build, 129 the first of the
                        256-slot build (two-slot merges); eight variables with KS proposals (0: belief kept, 1: proposal copied),
                        so every level image is resident
  sweeps                two Gibbs sweeps per level (iters = 2)
  wide                  513 variables: the launch is wide enough to protect occupancy, four images are resident and the variables
                        with 5 and 7 proposals stream theirs through slot 0
  lds                   D = 6, N = 130: 64 kB hold six 10 240-byte images, so K = 7 streams while K = 6 stays resident in one launch

Proposals are scattered over the row table; a circular coordinate straddles ±π; SE(3) rotation vectors reach about 3 rad, so the
chart at point 0 is exercised."""
import functools

import numpy as np

SHAPE_N = (1, 2, 3, 9, 37, 64, 100, 128, 129, 200, 256)
INSTANTIATIONS = ((2, 0), (2, 0b10), (3, 0b100), (3, 0), (3, 0b011), (6, 0), (6, 0b001))   # (D, circ); masks 0b10, 0b011, 0b001 are read at run time
OWN_MASK = {2: 0, 3: 0b100, 6: 0}                                                          # the mask of the variable type of each D
KS = (2, 3, 0, 1, 5, 11, 2, 4)
KS_WIDE = (5, 7) + (2, 1, 0) * 170 + (2,)                                                  # 513 variables
KS_LDS = (7, 6, 2)
SEED, STREAM_OFFSET = 11, 5                                                                # of the draws (rome_opts)


def _quat(w):
    """unit quaternions (w, x, y, z) of rotation vectors w (..., 3)"""
    th = np.linalg.norm(w, axis=-1, keepdims=True)
    k = np.where(th > 1e-12, np.sin(0.5 * th) / np.where(th > 1e-12, th, 1.0), 0.5)
    return np.concatenate([np.cos(0.5 * th), k * w], axis=-1)


def _qmul(a, b):
    aw, av, bw, bv = a[..., :1], a[..., 1:], b[..., :1], b[..., 1:]
    return np.concatenate([aw * bw - (av * bv).sum(-1, keepdims=True), aw * bv + bw * av + np.cross(av, bv)], axis=-1)


def _rotvec(q):
    """rotation vectors of unit quaternions, angle in [0, π]"""
    q = np.where(q[..., :1] < 0, -q, q)
    n = np.linalg.norm(q[..., 1:], axis=-1, keepdims=True)
    th = 2.0 * np.arctan2(n, q[..., :1])
    return np.where(n > 1e-12, th / np.where(n > 1e-12, n, 1.0), 2.0) * q[..., 1:]


def rotation_angle(wa, wb):
    """angle between the rotations of rotation vectors wa, wb (..., 3)"""
    qa = _quat(wa)
    qa[..., 1:] *= -1.0
    r = _qmul(qa, _quat(wb))
    return 2.0 * np.arctan2(np.linalg.norm(r[..., 1:], axis=-1), np.abs(r[..., 0]))


def _proposals(D, N, Ks, circ, rng):
    props = []
    for K in Ks:
        centre = rng.normal(0, 3, D)
        if D == 6:
            u = rng.standard_normal(3)
            centre[3:] = u / np.linalg.norm(u) * rng.uniform(2.6, 3.1)
        for _ in range(K):
            mu = centre + rng.normal(0, 0.3, D)
            sd = rng.uniform(0.05, 0.8, D)
            P = mu[:, None] + sd[:, None] * rng.standard_normal((D, N))
            if rng.random() < 0.3:   # a bimodal proposal
                P[0, rng.random(N) < 0.4] += 2.5
            if D == 6:               # rotations: the variable's rotation ∘ a small one ∘ noise
                q = _qmul(_qmul(_quat(centre[3:]), _quat(rng.normal(0, 0.1, 3))), _quat(rng.uniform(0.02, 0.2, 3) * rng.standard_normal((N, 3))))
                P[3:] = _rotvec(q).T
            for d in range(D):
                if (circ >> d) & 1:
                    P[d] = np.arctan2(np.sin(P[d] + 3.0), np.cos(P[d] + 3.0))   # straddling ±π
            props.append(P)
    return np.stack(props)


def _table(D, circ, N, Ks, iters, seed):
    rng = np.random.default_rng(seed)
    prop = _proposals(D, N, Ks, circ, rng)
    rows = rng.permutation(len(prop)).astype(np.int32)   # proposals scattered over the table:
    prop = np.ascontiguousarray(prop[np.argsort(rows)])  # row rows[k] holds the k-th proposal of the CSR order
    return {"D": D, "circ": circ, "N": N, "iters": iters, "ptr": np.concatenate([[0], np.cumsum(Ks)]).astype(np.int32), "rows": rows,
            "prop": prop, "bw": rng.uniform(0.05, 0.4, (len(prop), D)), "bel": rng.standard_normal((len(Ks), D, N)),
            "seed": SEED, "stream_offset": STREAM_OFFSET}


def _families():
    fam = {}
    for i, (D, circ) in enumerate(INSTANTIATIONS):
        fam["shapes D=%d circ=%d" % (D, circ)] = [("D=%d circ=%d N=%d" % (D, circ, N), (D, circ, N, KS, 1, 10000 * i + N)) for N in SHAPE_N]
    fam["sweeps"] = [("sweeps D=%d N=%d" % (D, N), (D, OWN_MASK[D], N, KS, 2, 100000 + 1000 * D + N)) for D in (2, 3, 6) for N in (37, 200)]
    fam["wide"] = [("wide D=%d N=%d" % (D, N), (D, OWN_MASK[D], N, KS_WIDE, 1, 200000 + 1000 * D + N)) for D in (2, 3, 6) for N in (9, 130)]
    fam["lds"] = [("lds D=6 N=130", (6, 0, 130, KS_LDS, 1, 300000))]
    return fam


FAMILIES = _families()
_SPEC = {name: spec for tables in FAMILIES.values() for name, spec in tables}


@functools.lru_cache(maxsize=None)
def table(name):
    """the table of that name: built once, shared, not to be written to"""
    t = _table(*_SPEC[name])
    for a in t.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


def names(family=None):
    return [n for f, tables in FAMILIES.items() if family in (None, f) for n, _ in tables]
