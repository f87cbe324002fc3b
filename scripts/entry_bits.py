#!/usr/bin/env python3
"""Writes tests/golden/entry_bits.json: the sha256 of the output bytes (and of the status array where the entry has one) of every
host-pointer convolution entry, sampler entry and residual entry of include/rome_mi355.h, on the smallest tables that exercise what
the host code behind them decides -- dimensions per direction, packing of the noise parameters, layout staging, the direction
column, multihypo blocks, nullhypo -- from the library that is loaded (ROME_MI355_LIB selects another build).  Run on the GPU with
the library of the commit whose bits are to be kept; tests/test_gpu_dev_entries.py asserts that they have not changed.

Only the C entry points are called (through ctypes), never the wrappers of rome_jl_amd/api.py: the script gives the same calls to
any build of the library.

    python scripts/entry_bits.py [out.json]"""
import ctypes as C
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

C_ROWS = 3
SHAPES_N = (10, 34)          # one shape on the wave-per-row path, one on the packed path
SOA, AOS, AOS_POINTS = 0, 1, 2
POINT_LEN = {2: 2, 3: 6, 6: 12}

# entry -> (dz, d1, d2, noise parameters, direction argument, status array); d1 == 0: a sampler (no fixed side)
CONV = {
    "rome_conv_pose2pose2":         (3, 3, 3, "cov", "rows", True),
    "rome_conv_pose2point2br":      (2, 3, 2, "sigma", "scalar", True),
    "rome_conv_pose3pose3":         (6, 6, 6, "cov", "rows", True),
    "rome_conv_point2point2range":  (1, 2, 2, "sigma", "rows", True),
    "rome_conv_pose2point2range":   (1, 3, 2, "sigma", "scalar", True),
    "rome_conv_pose2point2bearing": (1, 3, 2, "sigma", "scalar", True),
    "rome_conv_pose3pose3xyyaw":    (3, 6, 6, "cov", "rows", True),
    "rome_conv_pose3pose3rotation": (3, 6, 6, "cov", "rows", True),
    "rome_conv_priorpose3zrp":      (3, 6, 6, "zrp", None, False),
    "rome_sample_priorpose2":       (3, 0, 3, "cov", None, False),
    "rome_sample_priorpose3":       (6, 0, 6, "cov", None, False),
    "rome_sample_priorpoint2":      (2, 0, 2, "cov", None, False),
}
MULTIHYPO = {"rome_conv_pose2pose2_mh": "rome_conv_pose2pose2", "rome_conv_pose2point2br_mh": "rome_conv_pose2point2br"}
# entry -> widths of the rows of (z, a, b or None, r)
RESIDUAL = {
    "rome_residual_pose2pose2": (3, 3, 3, 3), "rome_residual_priorpose2": (3, 3, None, 3),
    "rome_residual_pose2point2br": (2, 3, 2, 2), "rome_residual_pose2point2br_pt": (2, 6, 2, 2),
    "rome_residual_pose3pose3": (6, 6, 6, 6), "rome_residual_pose3pose3_pt": (6, 12, 12, 6),
    "rome_residual_priorpose3": (6, 6, None, 6),
    "rome_residual_point2point2range": (1, 2, 2, 1), "rome_residual_pose2point2range": (1, 3, 2, 1),
    "rome_residual_pose2point2bearing": (1, 3, 2, 1), "rome_residual_pose2point2bearing_pt": (1, 6, 2, 1),
    "rome_residual_pose3pose3xyyaw": (3, 6, 6, 3), "rome_residual_pose3pose3xyyaw_pt": (3, 12, 12, 3),
    "rome_residual_pose3pose3rotation": (3, 6, 6, 3), "rome_residual_pose3pose3rotation_pt": (3, 12, 12, 3),
}
RESIDUAL_N = (5, 0, 1)

_PD = C.POINTER(C.c_double)
_PI = C.POINTER(C.c_int32)


def _p(a):
    return None if a is None else a.ctypes.data_as(_PD)


def _pi(a):
    return None if a is None else a.ctypes.data_as(_PI)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _coords(rng, d, shape):
    """coordinates of a variable of dimension d, (..., d): Point2 (x, y), Pose2 (x, y, θ), Pose3 (t, ω) with |ω| well inside π"""
    scale = {2: [3.0, 3.0], 3: [3.0, 3.0, 0.8], 6: [3.0, 3.0, 3.0, 0.4, 0.4, 0.4]}[d]
    return rng.normal(size=tuple(shape) + (d,)) * np.array(scale)


def _measurement(rng, entry, dz):
    mu = rng.normal(size=(C_ROWS, dz)) * 0.5
    if "range" in entry:
        mu = np.abs(mu) + 2.0                     # a range
    if entry.startswith("rome_conv_pose2point2br"):
        mu[:, 1] = np.abs(mu[:, 1]) + 2.0         # (bearing, range)
    return np.ascontiguousarray(mu)


def _noise_parameters(rng, form, dz):
    """what the entry takes between mu and the blocks: [cov], [sigma] (one negative: a Uniform belief) or [sigma_z, cov_rp]"""
    def cov(d):
        a = rng.normal(size=(C_ROWS, d, d)) * 0.1
        return np.ascontiguousarray(a @ a.transpose(0, 2, 1) + 0.01 * np.eye(d))
    if form == "cov":
        return [cov(dz)]
    if form == "sigma":
        s = 0.02 + 0.1 * rng.random(size=(C_ROWS, dz))
        s[C_ROWS - 1, 0] *= -1.0
        return [np.ascontiguousarray(s)]
    return [np.ascontiguousarray(0.05 + 0.1 * rng.random(size=C_ROWS)), cov(2)]


def _blocks(lib, ctx, coords, layout):
    """coords (C, N, d) -> the caller's array in `layout`: [C][d][N], [C][N][d] or [C][N][point_len] native points"""
    from rome_jl_amd import _lib
    n, N, d = coords.shape
    if layout == SOA:
        return np.ascontiguousarray(coords.transpose(0, 2, 1))
    if layout == AOS or d == 2:
        return np.ascontiguousarray(coords)
    pts = np.empty((n, N, POINT_LEN[d]))
    _lib.check(lib.rome_coords_to_points(ctx.handle, d, n * N, _p(np.ascontiguousarray(coords)), _p(pts)), ctx.handle)
    return pts


def _layouts(dims):
    return (SOA, AOS, AOS_POINTS) if max(dims) > 2 else (SOA, AOS)   # (a Point2 point IS its coordinates)


def conv_case(lib, ctx, entry, N, direction, layout, with_noise, solver=1, presampled=0, nullhypo=0.0, mh_of=None):
    """one call of a convolution / sampler entry -> sha256 of (output, status).  direction: None (all rows 0 through a NULL column, or
    an entry without one), "rows" (a per-row column 1, 0, 1), or the scalar 0 / 1."""
    from rome_jl_amd import _lib
    dz, d1, d2, form, dirform, has_status = CONV[mh_of or entry]
    rng = np.random.default_rng([N, layout, sum(map(ord, entry))])        # (the inputs depend on the family and the shape only)
    mu, prm = _measurement(rng, mh_of or entry, dz), _noise_parameters(rng, form, dz)
    df, dt = (d2, d1) if direction == 1 else (d1, d2)
    fixed = _blocks(lib, ctx, _coords(rng, df, (C_ROWS, N)), layout) if d1 and form != "zrp" else None
    out = _blocks(lib, ctx, _coords(rng, dt, (C_ROWS, N)), layout)
    alt = hypo_w = None
    if mh_of:
        alt = _blocks(lib, ctx, _coords(rng, df if direction == 1 else dt, (C_ROWS, N)), layout)
        hypo_w = np.array([0.5, 0.8, 1.0])
    noise = None
    if with_noise:
        xi = rng.normal(size=(C_ROWS, N, dz))
        if presampled:
            xi = mu[:, None, :] + 0.05 * xi                                 # the measurement samples themselves
        noise = np.ascontiguousarray(xi.transpose(0, 2, 1) if layout == SOA else xi)
    o = _lib.default_opts(solver, n_particles=N, seed=11, stream_offset=5, layout=layout, presampled=presampled, nullhypo=nullhypo)
    st = np.full((C_ROWS, N), -7, dtype=np.int32) if has_status else None
    args = [ctx.handle, C.byref(o), C_ROWS]
    if dirform == "rows" and not mh_of:
        args.append(_pi(np.array([1, 0, 1], dtype=np.int32)) if direction == "rows" else None)
    elif dirform is not None:
        args.append(int(direction))
    args += [_p(mu)] + [_p(a) for a in prm]
    if fixed is not None:
        args.append(_p(fixed))
    if mh_of:
        args += [_p(alt), _p(hypo_w)]
    args += [_p(noise), _p(out)]
    if has_status:
        args.append(_pi(st))
    _lib.check(getattr(lib, entry)(*args), ctx.handle)
    return _sha(out, st) if has_status else _sha(out)


def conv_cases():
    """(key, keyword arguments of conv_case) of every recorded convolution / sampler call"""
    for entry, (dz, d1, d2, form, dirform, has_status) in CONV.items():
        directions = {"rows": (None, "rows"), "scalar": (0, 1), None: (None,)}[dirform]
        for N in SHAPES_N:
            for direction in directions:
                for layout in _layouts((d1, d2)):
                    for with_noise in (False, True):
                        yield ("%s N=%d dir=%s layout=%d noise=%d" % (entry, N, direction, layout, with_noise),
                               dict(entry=entry, N=N, direction=direction, layout=layout, with_noise=with_noise))
        yield entry + " presampled", dict(entry=entry, N=SHAPES_N[0], direction=directions[-1], layout=SOA, with_noise=True, presampled=1)
        if d1:
            yield entry + " nullhypo=0.3", dict(entry=entry, N=SHAPES_N[1], direction=directions[-1], layout=AOS, with_noise=False, nullhypo=0.3)
    for entry, of in MULTIHYPO.items():
        for N in SHAPES_N:
            for direction in (0, 1):
                yield ("%s N=%d dir=%d" % (entry, N, direction),
                       dict(entry=entry, N=N, direction=direction, layout=AOS, with_noise=False, mh_of=of))
    for solver in (0, 1, 2, 3):
        yield ("rome_conv_pose2pose2 solver=%d" % solver,
               dict(entry="rome_conv_pose2pose2", N=SHAPES_N[0], direction="rows", layout=SOA, with_noise=False, solver=solver))


def residual_case(lib, ctx, entry, n):
    """-> sha256 of the residual rows; the buffer holds one row more than the entry may write, so n = 0 shows that nothing was"""
    from rome_jl_amd import _lib
    zw, aw, bw, rw = RESIDUAL[entry]
    rng = np.random.default_rng([n, sum(map(ord, entry))])
    z = rng.normal(size=(n, zw)) * 0.5
    if "range" in entry:
        z = np.abs(z) + 2.0

    def rows(w):
        d = {6: 3, 12: 6}.get(w, w) if entry.endswith("_pt") else w     # (_pt: the pose rows are native points)
        c = np.ascontiguousarray(_coords(rng, d, (n,)))
        pts = np.empty((n, w))
        if d == w or n == 0:
            return c if d == w else pts
        _lib.check(lib.rome_coords_to_points(ctx.handle, d, n, _p(c), _p(pts)), ctx.handle)
        return pts
    ins = [np.ascontiguousarray(z), rows(aw)] + ([rows(bw)] if bw else [])
    r = np.full((n + 1, rw), -7.0)
    _lib.check(getattr(lib, entry)(ctx.handle, n, *[_p(a) for a in ins], _p(r)), ctx.handle)
    return _sha(r)


def hashes():
    """{key: sha256} of every case above, from the loaded library"""
    import rome_jl_amd as R
    from rome_jl_amd import _lib
    lib, ctx = _lib.load(), R.Context(0)
    out = {key: conv_case(lib, ctx, **kw) for key, kw in conv_cases()}
    for entry in RESIDUAL:
        for n in RESIDUAL_N:
            out["%s n=%d" % (entry, n)] = residual_case(lib, ctx, entry, n)
    ctx.close()
    return out


def main():
    from rome_jl_amd import _lib
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "entry_bits.json")
    doc = {"what": "sha256 of the output bytes (float64 blocks, then the int32 status array where the entry has one) of every host-pointer "
                   "convolution, sampler and residual entry on the cases of scripts/entry_bits.py",
           "library_version": int(_lib.load().rome_version()), "sha256": hashes()}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d hashes -> %s" % (len(doc["sha256"]), out))


if __name__ == "__main__":
    main()
