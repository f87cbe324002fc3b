"""The KDE kernels (rome_kde_bandwidth[_dev]: k_kde_bandwidth<1 | 4 | 8>, k_kde_bandwidth_fast<7 | 10 | 13>; rome_kde_max[_dev]: k_kde_max)
against the references of tests/kde_ref.py at every launch shape: EVERY task of every table is decided by rule 1 (same iterates, 64 ulp),
rule 2 (optimum in the reference's basin) or rule 3 (root of the derivative within the caller's stopping rule).  The rules, the bounds and
the CPU conditions that make them total are stated in kde_ref's docstring and checked in tests/test_kde_ref_host.py; nothing here comes
from a GPU run, except tests/golden/kde_bits.json: the sha256 of the output bytes of every run and table below, written by
scripts/kde_bits.py on an MI355X from the library of commit 9f5f8f2, the last one before rome_kde.hip was rewritten to say each thing
once (profiles/kde_one_body.md).  That commit passes every rule test here, so the recorded bits are bits the rules accept."""
import importlib.util
import json
import os

import numpy as np
import pytest

import kde_ref as KR

pytestmark = pytest.mark.gpu
R = torch = DG = None
GUARD = 64                                     # doubles of NaN before and after every output
TABLES = dict(KR.all_tables())
MAX_TABLES = dict(KR.all_max_tables())
ROME_ERR_INVALID_ARG = -1


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


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")


def _guarded(n, shift=0):
    """n doubles between two NaN guard blocks; shift = 1 puts the block one double off 16-byte alignment"""
    buf = torch.full((2 * GUARD + n + shift,), float("nan"), dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD + shift:GUARD + shift + n]


def _guards_intact(buf, n, shift=0):
    return bool(torch.isnan(buf[:GUARD + shift]).all()) and bool(torch.isnan(buf[GUARD + shift + n:]).all())


def _args(tols):
    return (0.0, 0.0) if tols == KR.DEFAULT_TOLS else tols                       # 0 selects the reference's stopping rules


def run_bandwidth(bel_h, mask, tols, shift=0):
    """one launch of rome_kde_bandwidth_dev -> host (V, dim); asserts the guards and that the input is bit-unchanged"""
    V, dim, N = bel_h.shape
    bel = _dev(bel_h)
    keep = bel.clone()
    buf, out = _guarded(V * dim, shift)
    assert out.data_ptr() % 16 == 8 * (shift % 2)
    torch.cuda.synchronize()
    R._lib.check(DG._lib.rome_kde_bandwidth_dev(DG.ctx.handle, dim, V, N, bel.data_ptr(), mask, *_args(tols), out.data_ptr()), DG.ctx.handle)
    DG.ctx.synchronize()
    assert _guards_intact(buf, V * dim, shift), "a guard block was written"
    assert torch.equal(bel, keep), "the input was modified"
    return out.cpu().numpy().reshape(V, dim)


def _launches(name):
    """every (mask, run) of a table: device entry, once more, one double off alignment, host entry -- the same bits; -> the checks"""
    ref = KR.reference(name)
    t = ref.table
    assert (ref.V * ref.dim) % KR.KDE_WAVES != 0                                  # the last block has idle waves
    out = []
    for i, (mask, tols) in enumerate(ref.runs):
        h = run_bandwidth(t["bel"], mask, tols)
        assert np.array_equal(h, run_bandwidth(t["bel"], mask, tols)), "a second launch gives other bits"
        if i == 0:
            assert np.array_equal(h, run_bandwidth(t["bel"], mask, tols, shift=1)), "other bits one double off 16-byte alignment"
        assert np.array_equal(h, R.kde_bandwidth(t["bel"], mask, *_args(tols))), "rome_kde_bandwidth differs from rome_kde_bandwidth_dev"
        fig, bad = ref.check(mask, tols, h)
        print("KDE gpu %-28s %-6s mask %-8s tols %-14s rule 1 %.2e  rule 2 %.2e (%d by f)  rule 3 %.2e" % (
            name, KR.launch_shape(ref.N)["cls"], bin(mask), tols, fig["1"], fig["2"], fig["2f"], fig["3"]))
        out.append((mask, tols, h, bad))
    return ref, out


def _names(*families):
    return [n for n in TABLES if KR.family(n) in families]


@pytest.mark.parametrize("name", _names("shape"))
def test_bandwidth_every_launch_shape(name):
    for mask, tols, h, bad in _launches(name)[1]:
        assert not bad, (name, mask, tols, bad)


@pytest.mark.parametrize("name", _names("circ"))
def test_bandwidth_circular_nowrap_wrapped_uniform(name):
    for mask, tols, h, bad in _launches(name)[1]:
        assert not bad, (name, mask, tols, bad)


@pytest.mark.parametrize("name", _names("mask"))
def test_bandwidth_mask_bit_of_every_coordinate(name):
    ref, runs = _launches(name)
    assert len(runs) == 2 and runs[0][0] ^ runs[1][0] == (1 << ref.dim) - 1     # the mask and its complement
    for mask, tols, h, bad in runs:
        assert not bad, (name, mask, tols, bad)


@pytest.mark.parametrize("name", _names("outlier", "wide"))
def test_bandwidth_outlier_and_wide_tables(name):
    for mask, tols, h, bad in _launches(name)[1]:
        assert not bad, (name, mask, tols, bad)


@pytest.mark.parametrize("name", _names("degenerate"))
def test_bandwidth_degenerate_tables(name):
    for mask, tols, h, bad in _launches(name)[1]:
        assert np.isfinite(h).all() and (h > 0).all()
        assert not bad, (name, mask, tols, bad)
        if name == "degenerate equal":                                            # minm = 1e-6, f monotone in h
            assert (h <= 1e-5).all(), h


def run_max(t, shift=0):
    V, dim, N = t["bel"].shape
    bel, bw = _dev(t["bel"]), _dev(t["bw"])
    keep = bel.clone(), bw.clone()
    buf, out = _guarded(V * dim, shift)
    torch.cuda.synchronize()
    R._lib.check(DG._lib.rome_kde_max_dev(DG.ctx.handle, dim, V, N, bel.data_ptr(), bw.data_ptr(), t["G"], out.data_ptr()), DG.ctx.handle)
    DG.ctx.synchronize()
    assert _guards_intact(buf, V * dim, shift), "a guard block was written"
    assert torch.equal(bel, keep[0]) and torch.equal(bw, keep[1]), "an input was modified"
    return out.cpu().numpy().reshape(V, dim)


@pytest.mark.parametrize("name", list(MAX_TABLES))
def test_kde_max_every_grid_and_particle_shape(name):
    ref = KR.max_reference(name)
    t = ref.table
    m = run_max(t)
    assert np.isfinite(m).all()
    assert np.array_equal(m, run_max(t, shift=1)) and np.array_equal(m, R.kde_max(t["bel"], t["bw"], t["G"]))
    worst, bad = ref.check(m)
    print("KDEMAX gpu %-28s grid point within %.3f of the bound" % (name, worst))
    assert not bad, (name, bad)


def test_kde_max_refuses_257_grid_points_and_no_particles():
    lib, h = DG._lib, DG.ctx.handle
    t = KR.max_table("pair", 3, 65)
    V, dim, N = t["bel"].shape
    bel, bw = _dev(t["bel"]), _dev(t["bw"])
    buf, out = _guarded(V * dim)
    assert lib.rome_kde_max_dev(h, dim, V, N, bel.data_ptr(), bw.data_ptr(), 257, out.data_ptr()) == ROME_ERR_INVALID_ARG
    assert lib.rome_kde_max_dev(h, dim, V, 0, bel.data_ptr(), bw.data_ptr(), 64, out.data_ptr()) == ROME_ERR_INVALID_ARG
    with pytest.raises(Exception):
        R.kde_max(t["bel"], t["bw"], 257)
    with pytest.raises(Exception):
        R.kde_max(np.zeros((V, dim, 0)), t["bw"], 64)
    DG.ctx.synchronize()
    assert bool(torch.isnan(buf).all()), "a refused call wrote to its output"


def test_output_bits_are_the_recorded_ones():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kde_bits", os.path.join(root, "scripts", "kde_bits.py"))
    bits = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bits)
    with open(os.path.join(root, "tests", "golden", "kde_bits.json")) as f:
        want = json.load(f)["sha256"]
    runs = [bits.run_key(name, mask, tols) for name, make in TABLES.items() for t in [make()] for mask in t["masks"] for tols in t["runs"]]
    assert sorted(want) == sorted(runs + list(MAX_TABLES)) and len(want) == len(runs) + len(MAX_TABLES)
    got = bits.hashes()
    assert sorted(got) == sorted(want)
    diff = [k for k in got if got[k] != want[k]]
    assert not diff, diff
