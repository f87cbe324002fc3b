"""The entry points of include/rome_mi355.h that no other test calls by name: the device-pointer twins of the parametric linearisation and of
getKDEMax, the thin device-memory helpers a caller without a HIP binding uses (the Julia shim), the device count and the HIP error
accessors.  A `_dev` entry must return what its host-pointer twin returns, bit for bit -- the twin IS the same kernel behind a
staging copy.

The convolution, sampler and residual entries, which other tests call for what they compute, are held here to the bytes they returned
before they shared one body (tests/golden/entry_bits.json), and to the return code of every input that is invalid in exactly one way."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    import rome_jl_amd as R
    from rome_jl_amd import _lib, api
    return torch, R, _lib, api, _lib.load(), R.Context(0)


def test_device_count_and_error_accessors(env):
    torch, R, _lib, api, lib, ctx = env
    assert lib.rome_device_count() == torch.cuda.device_count() >= 1
    assert lib.rome_last_hip_error(ctx.handle) == 0                       # nothing failed on this context
    assert isinstance(lib.rome_last_hip_error_string(ctx.handle).decode(), str)
    assert lib.rome_last_hip_error(None) == 0                             # a NULL context: no error to report, no crash
    h = C.c_void_p()
    assert lib.rome_ctx_create(C.byref(h), 10 ** 6) == _lib.ERR_INVALID_ARG  # no such device: refused, no context made
    assert not h.value
    assert lib.rome_ctx_create(C.byref(h), -1) == _lib.ERR_INVALID_ARG      # the survey's "device = -1: CPU oracle" is deliberately refused
    assert lib.rome_ctx_create(None, 0) == _lib.ERR_INVALID_ARG


def test_dev_alloc_upload_download_roundtrip(env):
    torch, R, _lib, api, lib, ctx = env
    rng = np.random.default_rng(3)
    src = rng.normal(size=4097)
    back = np.zeros_like(src)
    p = C.c_void_p()
    _lib.check(lib.rome_dev_alloc(ctx.handle, src.nbytes, C.byref(p)), ctx.handle)
    assert p.value
    _lib.check(lib.rome_dev_upload(ctx.handle, p, src.ctypes.data, src.nbytes), ctx.handle)
    _lib.check(lib.rome_dev_download(ctx.handle, back.ctypes.data, p, src.nbytes), ctx.handle)
    assert np.array_equal(src, back)
    # a partial, offset copy: the helpers take plain byte counts and pointers
    back[:] = 0
    _lib.check(lib.rome_dev_download(ctx.handle, back.ctypes.data, C.c_void_p(p.value + 8 * 100), 8 * 50), ctx.handle)
    assert np.array_equal(back[:50], src[100:150]) and not back[50:].any()
    # zero bytes is a no-op, NULL pointers with bytes > 0 are refused
    assert lib.rome_dev_upload(ctx.handle, p, src.ctypes.data, 0) == _lib.OK
    assert lib.rome_dev_upload(ctx.handle, None, src.ctypes.data, 8) == _lib.ERR_INVALID_ARG
    assert lib.rome_dev_download(ctx.handle, back.ctypes.data, None, 8) == _lib.ERR_INVALID_ARG
    assert lib.rome_dev_alloc(ctx.handle, 8, None) == _lib.ERR_INVALID_ARG
    _lib.check(lib.rome_dev_free(ctx.handle, p), ctx.handle)
    assert lib.rome_dev_free(ctx.handle, None) == _lib.OK                 # like free(NULL)


def test_kde_max_dev_equals_the_host_entry(env):
    torch, R, _lib, api, lib, ctx = env
    rng = np.random.default_rng(5)
    V, N = 37, 100
    bel = rng.normal(size=(V, 3, N)) * np.array([2.0, 0.5, 0.3])[None, :, None] + rng.normal(size=(V, 3, 1)) * 5
    bel[:, 2] = (bel[:, 2] + np.pi) % (2 * np.pi) - np.pi
    bw = api.kde_bandwidth(bel, ctx=ctx)
    want = api.kde_max(bel, bw, ctx=ctx)
    d_bel = torch.from_numpy(bel).cuda(); d_bw = torch.from_numpy(bw).cuda(); d_out = torch.zeros((V, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for grid in (0, 200, 64):
        _lib.check(lib.rome_kde_max_dev(ctx.handle, 3, V, N, d_bel.data_ptr(), d_bw.data_ptr(), grid, d_out.data_ptr()), ctx.handle)
        ctx.synchronize()
        ref = want if grid in (0, 200) else api.kde_max(bel, bw, grid_points=grid, ctx=ctx)
        assert np.array_equal(d_out.cpu().numpy(), ref), grid              # 0 = the reference's 200 grid points
    assert lib.rome_kde_max_dev(ctx.handle, 3, V, N, d_bel.data_ptr(), d_bw.data_ptr(), 257, d_out.data_ptr()) == _lib.ERR_INVALID_ARG
    assert lib.rome_kde_max_dev(ctx.handle, 3, V, N, None, d_bw.data_ptr(), 0, d_out.data_ptr()) == _lib.ERR_INVALID_ARG


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5])
def test_linearize_dev_equals_the_host_entry(env, kind):
    torch, R, _lib, api, lib, ctx = env
    dz, dr, da, db = api._LIN_DIMS[kind]
    rng = np.random.default_rng(100 + kind)
    F = 513
    mu = rng.normal(size=(F, dz)); xa = rng.normal(size=(F, da)) * 2; xb = rng.normal(size=(F, db)) * 2 if db else None
    if kind == _lib.FACTOR_POSE2POINT2BR:
        mu[:, 1] = np.abs(mu[:, 1]) + 1.0
    A = rng.normal(size=(F, dr, dr)); W = np.triu(A) + 2 * np.eye(dr)
    r, Ja, Jb = api.linearize(kind, mu, W, xa, xb, ctx=ctx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    d_mu, d_W, d_xa = t(mu), t(W), t(xa)
    d_xb = t(xb) if db else None
    d_r = torch.zeros((F, dr), dtype=torch.float64, device="cuda"); d_Ja = torch.zeros((F, dr, da), dtype=torch.float64, device="cuda")
    d_Jb = torch.zeros((F, dr, db), dtype=torch.float64, device="cuda") if db else None
    torch.cuda.synchronize()
    ptr = lambda x: x.data_ptr() if x is not None else None          # noqa: E731
    _lib.check(lib.rome_linearize_dev(ctx.handle, kind, F, ptr(d_mu), ptr(d_W), ptr(d_xa), ptr(d_xb), ptr(d_r), ptr(d_Ja), ptr(d_Jb)), ctx.handle)
    ctx.synchronize()
    assert np.array_equal(d_r.cpu().numpy(), r) and np.array_equal(d_Ja.cpu().numpy(), Ja)
    if db:
        assert np.array_equal(d_Jb.cpu().numpy(), Jb)
        assert lib.rome_linearize_dev(ctx.handle, kind, F, ptr(d_mu), ptr(d_W), ptr(d_xa), None, ptr(d_r), ptr(d_Ja), ptr(d_Jb)) == _lib.ERR_INVALID_ARG
    assert lib.rome_linearize_dev(ctx.handle, 6, F, ptr(d_mu), ptr(d_W), ptr(d_xa), ptr(d_xb), ptr(d_r), ptr(d_Ja), ptr(d_Jb)) == _lib.ERR_INVALID_ARG
    assert lib.rome_linearize_dev(ctx.handle, kind, 0, ptr(d_mu), ptr(d_W), ptr(d_xa), ptr(d_xb), ptr(d_r), ptr(d_Ja), ptr(d_Jb)) == _lib.OK   # nothing to do


# ---- the convolution, sampler and residual entries: recorded bits, and one table of refusals
@pytest.fixture(scope="module")
def EB():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("entry_bits", os.path.join(root, "scripts", "entry_bits.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.ROOT = root
    return m


def test_entry_output_bits_are_the_recorded_ones(env, EB):
    """tests/golden/entry_bits.json was written by scripts/entry_bits.py on an MI355X from the library of commit 74c2229, the last one
    in which every host-pointer entry had a body of its own (profiles/entries_one_body.md); two recordings were equal."""
    with open(os.path.join(EB.ROOT, "tests", "golden", "entry_bits.json")) as f:
        want = json.load(f)["sha256"]
    got = EB.hashes()
    assert sorted(got) == sorted(want) and len(got) == len(list(EB.conv_cases())) + len(EB.RESIDUAL) * len(EB.RESIDUAL_N)
    diff = [k for k in got if got[k] != want[k]]
    assert not diff, diff


def _host_call(EB, _lib, lib, ctx, entry, change):
    """A valid call of a host-pointer convolution / sampler entry (C = 1, N = 10, SoA) with `change` = {argument: value} applied.
    Arguments by name: ctx, opts, C, dir, mu, prm0, prm1, fixed, alt, hypo_w, noise, out, status; n_particles changes the options.
    -> (return code, whether the output and status arrays are untouched)"""
    of = EB.MULTIHYPO.get(entry)
    dz, d1, d2, form, dirform, has_status = EB.CONV[of or entry]
    N, rng = 10, np.random.default_rng(1)
    o = _lib.default_opts(_lib.SOLVER_NEWTON, n_particles=change.get("n_particles", N))
    prm = {"cov": [0.01 * np.eye(dz)[None]], "sigma": [np.full((1, dz), 0.1)], "zrp": [np.full(1, 0.1), 0.01 * np.eye(2)[None]]}[form]
    arrays = {"mu": np.full((1, dz), 2.0), "prm0": prm[0], "out": rng.normal(size=(1, d2, N)), "hypo_w": np.array([0.5]),
              "fixed": rng.normal(size=(1, max(d1, 1), N)), "alt": rng.normal(size=(1, d2, N)), "status": np.full((1, N), -7, np.int32)}
    if len(prm) > 1:
        arrays["prm1"] = prm[1]
    arrays.update({k: v for k, v in change.items() if isinstance(v, np.ndarray)})
    arrays = {k: np.ascontiguousarray(v) for k, v in arrays.items()}
    before = arrays["out"].copy()
    names = ["ctx", "opts", "C"] + (["dir"] if dirform or of else []) + ["mu", "prm0"] + (["prm1"] if len(prm) > 1 else []) + \
        (["fixed"] if d1 and form != "zrp" else []) + (["alt", "hypo_w"] if of else []) + ["noise", "out"] + (["status"] if has_status else [])
    value = {"ctx": ctx.handle, "opts": C.byref(o), "C": 1, "noise": None, "dir": None if dirform == "rows" and not of else 0}
    for k, a in arrays.items():
        value[k] = a.ctypes.data_as(C.POINTER(C.c_int32 if a.dtype == np.int32 else C.c_double))
    value.update({k: v for k, v in change.items() if not isinstance(v, np.ndarray) and k != "n_particles"})
    assert set(change) <= set(names) | {"n_particles"}, (entry, change)
    rc = getattr(lib, entry)(*[value[k] for k in names])
    return rc, np.array_equal(arrays["out"], before) and (arrays["status"] == -7).all()


def test_host_entries_refuse_each_invalid_input_with_the_documented_code(env, EB):
    """One thing wrong per call; every refusal returns before anything is staged or launched (the output arrays stay untouched)."""
    torch, R, _lib, api, lib, ctx = env
    INV, POSDEF, TOO_MANY = _lib.ERR_INVALID_ARG, _lib.ERR_NOT_POSDEF, _lib.ERR_UNSUPPORTED_N
    nan, two = np.array([[np.nan]]), np.array([2], np.int32)
    for entry in list(EB.CONV) + list(EB.MULTIHYPO):
        of = EB.MULTIHYPO.get(entry)
        dz, d1, d2, form, dirform, has_status = EB.CONV[of or entry]
        cases = [({"opts": None}, INV), ({"ctx": None}, INV), ({"C": -1}, INV), ({"C": 0}, _lib.OK), ({"n_particles": _lib.MAX_PARTICLES + 1}, TOO_MANY),
                 ({"mu": None}, INV), ({"prm0": None}, INV), ({"out": None}, INV)]
        if d1 and form != "zrp":
            cases.append(({"fixed": None}, INV))
        if of:
            cases += [({"alt": None}, INV), ({"hypo_w": None}, INV), ({"hypo_w": np.array([1.5])}, INV), ({"hypo_w": np.array([-0.1])}, INV),
                      ({"hypo_w": np.array([np.nan])}, INV)]
        if dirform == "scalar" or of:
            cases += [({"dir": 2}, INV), ({"dir": -1}, INV)]
        elif dirform == "rows" and entry not in ("rome_conv_pose2pose2", "rome_conv_pose3pose3"):
            cases.append(({"dir": two}, INV))
        if form == "cov":
            cases += [({"prm0": -np.eye(dz)[None]}, POSDEF), ({"prm0": np.full((1, dz, dz), np.nan)}, POSDEF)]
        elif form == "sigma":
            cases.append(({"prm0": np.full((1, dz), np.nan)}, POSDEF))
        else:
            cases += [({"prm1": None}, INV), ({"prm0": np.array([np.nan])}, POSDEF), ({"prm1": -np.eye(2)[None]}, POSDEF)]
        for change, want in cases:
            rc, untouched = _host_call(EB, _lib, lib, ctx, entry, change)
            assert rc == want and untouched, (entry, change, rc)
    for entry in ("rome_conv_pose2pose2", "rome_conv_pose3pose3"):     # their rows may be ROME_DIR_PRIOR (2): the column is not range-checked
        rc, untouched = _host_call(EB, _lib, lib, ctx, entry, {"dir": two})
        assert rc == _lib.OK and not untouched, entry


def test_residual_entries_refuse_each_invalid_input(env, EB):
    torch, R, _lib, api, lib, ctx = env
    PD = C.POINTER(C.c_double)
    for entry, (zw, aw, bw, rw) in EB.RESIDUAL.items():
        ins = [np.ones((1, w)) for w in (zw, aw, bw) if w]
        r = np.full((1, rw), -7.0)
        ptrs = [a.ctypes.data_as(PD) for a in ins + [r]]
        fn = getattr(lib, entry)
        assert fn(None, 1, *ptrs) == _lib.ERR_INVALID_ARG, entry
        assert fn(ctx.handle, -1, *ptrs) == _lib.ERR_INVALID_ARG, entry
        for k in range(len(ptrs)):
            assert fn(ctx.handle, 1, *[None if j == k else p for j, p in enumerate(ptrs)]) == _lib.ERR_INVALID_ARG, (entry, k)
        assert fn(ctx.handle, 0, *ptrs) == _lib.OK and (r == -7.0).all(), entry      # nothing to do, nothing touched


# _dev entry -> (alt_var / hypo_w are passed on, the direction rule, the beliefs that are required)
DEV_ENTRIES = {
    "rome_conv_pose2pose2_dev": (True, None, "both"), "rome_conv_pose2point2br_dev": (True, "scalar", "both"),
    "rome_conv_pose3pose3_dev": (True, None, "both"), "rome_conv_point2point2range_dev": (False, "rows", "both"),
    "rome_conv_pose2point2range_dev": (False, "scalar", "both"), "rome_conv_pose2point2bearing_dev": (False, "scalar", "both"),
    "rome_conv_pose3pose3xyyaw_dev": (False, "rows", "both"), "rome_conv_pose3pose3rotation_dev": (False, "rows", "both"),
    "rome_conv_priorpose3zrp_dev": (False, None, "target"), "rome_sample_priorpose2_dev": (True, None, None),
    "rome_sample_priorpose3_dev": (True, None, None), "rome_sample_priorpoint2_dev": (True, None, None),
}


def test_dev_entries_refuse_each_invalid_table_before_any_launch(env):
    """One thing wrong per call.  Every pointer of the table is the same zeroed device buffer, large enough for one row of any family, and
    it is still all zeros afterwards: nothing was launched."""
    torch, R, _lib, api, lib, ctx = env
    INV = _lib.ERR_INVALID_ARG
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = buf.data_ptr()
    o = _lib.default_opts(_lib.SOLVER_NEWTON, n_particles=10)
    big = _lib.default_opts(_lib.SOLVER_NEWTON, n_particles=_lib.MAX_PARTICLES + 1)

    def table(**change):
        t = _lib.ConvDev(n_conv=1, dir_all=0, mu=p, L=p, bel_fixed=p, bel_target=p, out=p)
        for k, v in change.items():
            setattr(t, k, v)
        return t

    for entry, (mh, dir_rule, beliefs) in DEV_ENTRIES.items():
        fn = getattr(lib, entry)
        assert fn(ctx.handle, None, C.byref(table())) == INV, entry
        assert fn(None, C.byref(o), C.byref(table())) == INV, entry
        assert fn(ctx.handle, C.byref(o), None) == INV, entry
        assert fn(ctx.handle, C.byref(big), C.byref(table())) == _lib.ERR_UNSUPPORTED_N, entry
        cases = [dict(n_conv=-1), dict(mu=None), dict(L=None), dict(out=None), dict(mirror_out=p, n_mirror=5)]
        cases += {"both": [dict(bel_fixed=None), dict(bel_target=None)], "target": [dict(bel_target=None)], None: []}[beliefs]
        if not mh:
            cases += [dict(alt_var=p), dict(hypo_w=p)]
        if dir_rule == "scalar":
            cases += [dict(dir=p), dict(dir_all=2), dict(dir_all=-1)]
        if dir_rule == "rows":
            cases += [dict(dir_all=2)]
        for change in cases:
            assert fn(ctx.handle, C.byref(o), C.byref(table(**change))) == INV, (entry, change)
        assert fn(ctx.handle, C.byref(o), C.byref(table(n_conv=0))) == _lib.OK, entry   # no rows: nothing to launch
    ctx.synchronize()
    assert not buf.any()
