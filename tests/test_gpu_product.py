"""The importance product (rome_product_dev / rome_product_bw_dev: k_product<M,S> over the manifolds Flat<2>, Flat<3>, Se3M) and the
belief statistics (rome_belief_stats*: k_belief_stats<D>) against the references of tests/product_ref.py: EVERY particle of every table is
decided -- the pick recovered from the output equals the reference's, the output lies within 64 ulp of Pb[pick] ⊕ h_p⊙ξ at the variable's
scale, K = 0 / 1 blocks are bit copies.  The rule, the bounds and the CPU conditions that make it total are stated in product_ref's
docstring and checked in tests/test_product_ref_host.py; nothing in those tests comes from a GPU run.

tests/golden/product_bits.json holds the sha256 of the output bytes of every one of these tables and of the statistics at every (D, N),
written by scripts/product_bits.py from the two-kernel source (k_product<D,S> and k_product_se3<S>) that the one-body kernel replaced:
the outputs are bit-for-bit what they were then."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

import product_ref as PR

pytestmark = pytest.mark.gpu
R = torch = DG = None
GUARD = 64                                     # doubles of NaN before and after every output
TABLES = dict(PR.all_tables())
ROME_OK, ROME_ERR_INVALID_ARG, ROME_ERR_UNSUPPORTED_N = 0, -1, -5


@pytest.fixture(scope="module", autouse=True)
def _pkg():
    global R, torch, DG
    import torch as _torch
    import rome_jl_amd
    R, torch = rome_jl_amd, _torch
    R.default_context()
    fg = R.initfg(8); fg.addVariable("x0", R.Pose2); fg.addFactor(["x0"], R.PriorPose2())
    DG = R.DeviceGraph(fg)                     # the library handle and its context
    yield


def _dev(a, dt):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda")


def _guarded(n, shift=0):
    """n doubles between two NaN guard blocks; shift = 1 puts the block one double off 16-byte alignment"""
    buf = torch.full((2 * GUARD + n + shift,), float("nan"), dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + shift:GUARD + shift + n]


def _guards_intact(buf, n, shift=0):
    return bool(torch.isnan(buf[:GUARD + shift]).all()) and bool(torch.isnan(buf[GUARD + shift + n:]).all())


def run_product(t, shift=0):
    """launch one table -> host output (V, D, N); asserts the guards and that every input is bit-unchanged"""
    D, N = t["D"], t["N"]
    V = len(t["ptr"]) - 1
    ptr, rows, prop, bel = _dev(t["ptr"], torch.int32), _dev(t["rows"], torch.int32), _dev(t["prop"], torch.float64), _dev(t["bel"], torch.float64)
    bw = None if t["bw"] is None else _dev(t["bw"], torch.float64)
    keep = [x.clone() for x in (ptr, rows, prop, bel)] + ([bw.clone()] if bw is not None else [])
    buf, out = _guarded(V * D * N, shift)
    assert out.data_ptr() % 16 == 8 * shift
    o = R.make_opts(N=N, seed=t["seed"], stream_offset=t["stream_offset"])
    torch.cuda.synchronize()
    if bw is None:
        rc = DG._lib.rome_product_dev(DG.ctx.handle, C.byref(o), D, V, ptr.data_ptr(), rows.data_ptr(), prop.data_ptr(), bel.data_ptr(), out.data_ptr())
    else:
        rc = DG._lib.rome_product_bw_dev(DG.ctx.handle, C.byref(o), D, V, ptr.data_ptr(), rows.data_ptr(), prop.data_ptr(), bw.data_ptr(),
                                         bel.data_ptr(), out.data_ptr())
    R._lib.check(rc, DG.ctx.handle)
    DG.ctx.synchronize()
    assert _guards_intact(buf, V * D * N, shift), "a guard block was written"
    for a, b in zip(keep, [ptr, rows, prop, bel] + ([bw] if bw is not None else [])):
        assert torch.equal(a, b), "an input was modified"
    got = out.cpu().numpy().reshape(V, D, N)
    assert np.isfinite(got).all()
    return got


@pytest.mark.parametrize("name", list(TABLES))
def test_product_every_particle_decided(name):
    ref = PR.reference(name)
    fig, bad = ref.check(run_product(ref.table))
    print("PRODUCT gpu %-32s out %.3f / %.3f of the bound, pick distance %.3f, snap zone %d" % (name, fig["t"], fig["r"], fig["pick"], fig["zone"]))
    assert not bad, (name, bad)


@pytest.mark.parametrize("name", ["shape D=3 N=129 bw", "shape D=6 N=65 silverman", "large D=2 N=65 silverman"])
def test_product_output_one_double_off_alignment(name):
    ref = PR.reference(name)
    fig, bad = ref.check(run_product(ref.table, shift=1))
    assert not bad, (name, bad)


def test_product_error_paths():
    lib, h = DG._lib, DG.ctx.handle
    t = PR.shape_table(6, 2, PR.SILVERMAN)
    V = len(t["ptr"]) - 1
    ptr, rows = _dev(t["ptr"], torch.int32), _dev(t["rows"], torch.int32)
    small = torch.zeros(16, dtype=torch.float64, device="cuda")
    buf, out = _guarded(16)
    args = (ptr.data_ptr(), rows.data_ptr(), small.data_ptr(), small.data_ptr(), out.data_ptr())
    assert lib.rome_product_dev(h, C.byref(R.make_opts(N=257)), 6, V, *args) == ROME_ERR_UNSUPPORTED_N     # SE(3): N <= 256
    assert lib.rome_product_bw_dev(h, C.byref(R.make_opts(N=257)), 6, V, args[0], args[1], args[2], small.data_ptr(), args[3],
                                   args[4]) == ROME_ERR_UNSUPPORTED_N
    assert lib.rome_product_dev(h, C.byref(R.make_opts(N=64)), 4, V, *args) == ROME_ERR_INVALID_ARG
    assert lib.rome_product_bw_dev(h, C.byref(R.make_opts(N=64)), 4, V, args[0], args[1], args[2], small.data_ptr(), args[3], args[4]) == ROME_ERR_INVALID_ARG
    assert lib.rome_product_dev(h, C.byref(R.make_opts(N=64)), 3, 0, *args) == ROME_OK                     # V = 0: nothing to do
    DG.ctx.synchronize()
    assert bool(torch.isnan(buf).all()), "an error path / V = 0 wrote to bel_out"


@pytest.mark.parametrize("D", PR.DIMS)
def test_belief_stats_against_the_references(D):
    for N in PR.SHAPE_N[D]:
        ref = PR.stats_reference(D, N)
        bel = _dev(ref.bel, torch.float64)
        keep = bel.clone()
        n = PR.STATS_V * D
        mbuf, mean = _guarded(n); sbuf, sd = _guarded(n)
        torch.cuda.synchronize()
        R._lib.check(DG._lib.rome_belief_stats_dev(DG.ctx.handle, D, PR.STATS_V, N, bel.data_ptr(), mean.data_ptr(), sd.data_ptr()), DG.ctx.handle)
        DG.ctx.synchronize()
        assert _guards_intact(mbuf, n) and _guards_intact(sbuf, n) and torch.equal(bel, keep)
        m, s = mean.cpu().numpy().reshape(PR.STATS_V, D), sd.cpu().numpy().reshape(PR.STATS_V, D)
        fig, bad = ref.check(m, s)
        print("STATS gpu D=%d N=%-3d mean %.3f / %.3f  sd %.3f of the bound" % (D, N, fig["t"], fig["r"], fig["sd"]))
        assert not bad, (D, N, bad)
        hm, hs = R.belief_stats(ref.bel)                                        # the host-pointer entry: the same kernel
        assert np.array_equal(np.asarray(hm), m) and np.array_equal(np.asarray(hs), s), (D, N)


@pytest.mark.parametrize("bandwidth", ["silverman", "lcv"])
def test_device_graph_product_step_against_np_product(bandwidth):
    """a hexagon with one landmark: the CSR and the proposal rows DeviceGraph built, its Philox streams, and (lcv) the bandwidths the
    device selected, under the same rule -- np_product on exactly what product_step was given"""
    N = 64
    fg = R.generateGraph_Hexagonal(N=N)
    R.dead_reckon_init(fg, seed=5)
    dg = R.DeviceGraph(fg); dg.upload_beliefs(fg)
    opts = R.make_opts(N=N, solver=1, seed=4242, stream_offset=31)
    dg.conv_step(opts, 1)
    before = {vt: dg.bel[vt].cpu().numpy().copy() for vt in (R.Pose2, R.Point2)}
    dg.product_step(opts, 1, bandwidth)
    dg.ctx.synchronize()
    for vt, D, off in ((R.Pose2, 3, dg.STREAM_PROD2), (R.Point2, 2, dg.STREAM_PRODL)):
        c = dg.csr[vt]
        t = {"D": D, "N": N, "ptr": np.asarray(c["ptr_h"], dtype=np.int32), "rows": c["rows"].cpu().numpy().astype(np.int32),
             "prop": dg.prop[vt].cpu().numpy(), "bel": before[vt], "seed": 4242, "stream_offset": 31 + (1 << 32) + off,
             "bw": dg.prop_bw[vt].cpu().numpy() if bandwidth == "lcv" else None}
        assert len(t["ptr"]) - 1 == before[vt].shape[0] and np.diff(t["ptr"]).max() >= 2
        ref = PR.Reference(t)
        assert ref.gap >= PR.GAP_FACTOR * ref.delta(0.0), (vt, ref.gap)          # the margin rule holds for this table too (reference alone)
        assert all(eq or g >= PR.GAP_FACTOR * PR.ULP64 * D for g, eq in ref.lnh)
        fig, bad = ref.check(dg.bel[vt].cpu().numpy())
        assert not bad, (bandwidth, vt, bad)


def test_output_bits_are_the_recorded_ones():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("product_bits", os.path.join(root, "scripts", "product_bits.py"))
    bits = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bits)
    with open(os.path.join(root, "tests", "golden", "product_bits.json")) as f:
        want = json.load(f)["sha256"]
    got = bits.hashes(lambda name, make: PR.reference(name).table)           # the tables the tests above ran, not rebuilt
    assert sorted(got) == sorted(want) and len(got) == len(TABLES) + sum(len(PR.SHAPE_N[D]) for D in PR.DIMS)
    diff = [k for k in got if got[k] != want[k]]
    assert not diff, diff
