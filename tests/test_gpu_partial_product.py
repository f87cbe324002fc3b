"""The partial-aware product on the GPU: k_product_coord<S> through rome_product_partial_dev / rome_product_partial against
tests/partial_product_ref.py -- every output particle of every table decided (the rule in that module's docstring) --, the error paths,
and product_step / solveGraph with partial_product="coordinate" on the reference's chain (test/testPartialPose3.jl:455-501) and on a pose
seen by range only.  Every kernel launch made here has NaN guard blocks round `bel` and leaves its inputs bit-unchanged."""
import ctypes as C
import math

import numpy as np
import pytest

import partial_product_ref as PP
import rome_jl_amd as R
from rome_jl_amd import _lib
from test_partial_product_host import _chain_graph, _range_graph

pytestmark = pytest.mark.gpu
GUARD = 64                                                   # doubles of NaN on either side of bel (even: keeps bel 16-byte aligned)
SEED = 0x50415254


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _launch(t, misalign=False):
    """rome_product_partial_dev on one table -> bel afterwards (V, D, N); asserts the guards and the inputs"""
    import torch
    lib, ctx = _lib.load(), R.default_context()
    D, N, V = t["D"], t["N"], t["V"]
    tk = t["tasks"]
    T = len(tk["task_var"])
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")
    one = lambda a: a if len(a) else np.zeros(1, np.int32)
    ins = {"prop": dev(t["prop"]), "bw": None if t["bw"] is None else dev(t["bw"]), "jbw": None if t["jbw"] is None else dev(t["jbw"])}
    ins.update({k: dev(one(tk["task_" + k]), torch.int32) for k in ("var", "coord", "ptr", "rows", "joint")})
    n, off = V * D * N, GUARD + (1 if misalign else 0)
    buf = torch.full((off + n + GUARD,), float("nan"), dtype=torch.float64, device="cuda:0")
    bel = buf[off:off + n]
    assert bel.data_ptr() % 16 == (8 if misalign else 0)
    bel.copy_(dev(t["bel"]).reshape(-1))
    o = R.make_opts(N=N, seed=t["seed"], stream_offset=t["stream_offset"])
    ptr = lambda x: None if x is None else x.data_ptr()
    torch.cuda.synchronize()
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.rome_product_partial_dev(ctx.handle, C.byref(o), D, V, T, ptr(ins["var"]), ptr(ins["coord"]), ptr(ins["ptr"]), ptr(ins["rows"]),
                                            ptr(ins["joint"]), ptr(ins["prop"]), ptr(ins["bw"]), ptr(ins["jbw"]), t["circ"], bel.data_ptr()),
               ctx.handle)
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.isnan(h[:off]).all() and np.isnan(h[off + n:]).all(), "a guard block was written"
    for k, src in (("prop", t["prop"]), ("bw", t["bw"]), ("jbw", t["jbw"])):
        assert src is None or np.array_equal(_bits(ins[k].cpu().numpy()), _bits(src)), k
    for k in ("var", "coord", "ptr", "rows", "joint"):
        assert np.array_equal(ins[k].cpu().numpy(), one(tk["task_" + k])), k
    return h[off:off + n].reshape(V, D, N).copy()


def _decide(name, out):
    ref = PP.reference(name)
    fig, bad = ref.check(out)
    print("PARTPROD %-30s out %.3f  pick %.3f of the bound" % (name, fig["out"], fig["pick"]))
    assert bad == [], (name, bad[:3])


# ------------------------------------------------------------------ 1. the kernel, every shape
@pytest.mark.parametrize("mode", PP.MODES)
@pytest.mark.parametrize("N", PP.SHAPE_N)
@pytest.mark.parametrize("D", PP.DIMS)
def test_shapes(D, N, mode):
    """S = 1, 2, 4, 8 at their emptiest and full, N = 1 and 2; M = 1, 2, 3, 9 with and without the joint line; Euclidean and circular
    lines (clusters across ±π); two and more tasks on one variable, lines and variables without a task; rows scattered among unused ones,
    pass-through lines NaN"""
    name = "shape D=%d N=%d %s" % (D, N, mode)
    _decide(name, _launch(dict(PP.all_tables())[name]()))


@pytest.mark.parametrize("kind", ["zero", "far", "tie"])
@pytest.mark.parametrize("D", PP.DIMS)
def test_floor_far_apart_and_ties(D, kind):
    """zero: a density without spread under Silverman's rule -> the 1e-6 floor, and it is the base; far: densities 1000 h apart (every
    weight underflows without the running maximum), the joint line as base; tie: bit-equal bandwidths -> the lowest l"""
    name = "%s D=%d" % (kind, D)
    _decide(name, _launch(dict(PP.all_tables())[name]()))


@pytest.mark.parametrize("D", PP.DIMS)
def test_bel_one_double_off_16_byte_alignment(D):
    for N in (65, 512):
        name = "shape D=%d N=%d %s" % (D, N, PP.SUPPLIED)
        _decide(name, _launch(dict(PP.all_tables())[name](), misalign=True))


def test_no_tasks_is_a_no_op():
    t = dict(PP.shape_table(3, 65, PP.SILVERMAN))
    t["tasks"] = {k: np.zeros(1 if k == "task_ptr" else 0, np.int32) for k in t["tasks"]}
    assert np.array_equal(_launch(t), t["bel"])
    lib, ctx = _lib.load(), R.default_context()
    o = R.make_opts(N=65)
    assert lib.rome_product_partial_dev(ctx.handle, C.byref(o), 3, 0, 0, *[None] * 8, 0, None) == _lib.OK          # T = 0: nothing is required
    assert lib.rome_product_partial(ctx.handle, C.byref(o), 3, 0, 0, *[None] * 8, 0, None, 0) == _lib.OK


# ------------------------------------------------------------------ 2. error paths
def test_error_paths():
    import torch
    lib, ctx = _lib.load(), R.default_context()
    t = PP.shape_table(3, 65, PP.SUPPLIED)
    tk = t["tasks"]
    T = len(tk["task_var"])
    dev = lambda a, dt=torch.float64: torch.as_tensor(np.ascontiguousarray(a), dtype=dt, device="cuda:0")
    tabs = [dev(tk["task_" + k], torch.int32) for k in ("var", "coord", "ptr", "rows", "joint")]
    prop, bel = dev(t["prop"]), dev(t["bel"])
    before = bel.clone()
    args = [x.data_ptr() for x in tabs] + [prop.data_ptr(), None, None, t["circ"], bel.data_ptr()]
    o = R.make_opts(N=65)
    for dim in (0, 1, 4, 5, 7):
        assert lib.rome_product_partial_dev(ctx.handle, C.byref(o), dim, t["V"], T, *args) == _lib.ERR_INVALID_ARG
    for k in (0, 1, 2, 3, 4, 5, 9):                                              # every required pointer
        a = list(args); a[k] = None
        assert lib.rome_product_partial_dev(ctx.handle, C.byref(o), 3, t["V"], T, *a) == _lib.ERR_INVALID_ARG, k
    assert lib.rome_product_partial_dev(None, C.byref(o), 3, t["V"], T, *args) == _lib.ERR_INVALID_ARG
    assert lib.rome_product_partial_dev(ctx.handle, None, 3, t["V"], T, *args) == _lib.ERR_INVALID_ARG
    assert lib.rome_product_partial_dev(ctx.handle, C.byref(o), 3, t["V"], -1, *args) == _lib.ERR_INVALID_ARG
    for dim in PP.DIMS:                                                          # 512 at every dim: stage 2 is 1-D
        big = R.make_opts(N=_lib.MAX_PARTICLES_PRODUCT + 1)
        assert lib.rome_product_partial_dev(ctx.handle, C.byref(big), dim, t["V"], T, *args) == _lib.ERR_UNSUPPORTED_N
        with pytest.raises(R.RomeError) as e:
            R.product_partial(big, dim, dict(task_var=[0], task_coord=[0], task_ptr=[0, 1], task_rows=[0], task_joint=[0]),
                              np.zeros((1, dim, big.n_particles)), np.zeros((1, dim, big.n_particles)))
        assert e.value.code == _lib.ERR_UNSUPPORTED_N
    torch.cuda.synchronize()
    assert torch.equal(bel, before)                                              # nothing was launched


# ------------------------------------------------------------------ 3. the host entry
@pytest.mark.parametrize("D", PP.DIMS)
def test_host_entry_is_bit_equal_to_dev(D):
    for mode in PP.MODES:
        t = PP.shape_table(D, 65, mode)
        want = _launch(t)
        o = R.make_opts(N=65, seed=t["seed"], stream_offset=t["stream_offset"])
        prop, bel = t["prop"].copy(), t["bel"].copy()
        got = R.product_partial(o, D, t["tasks"], prop, bel, prop_bw=t["bw"], joint_bw=t["jbw"], circular_mask=t["circ"])
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(prop), _bits(t["prop"])) and np.array_equal(bel, t["bel"])
    assert np.array_equal(R.product_partial(o, D, t["tasks"], t["prop"], t["bel"], prop_bw=t["bw"], joint_bw=t["jbw"]), want)   # the default mask


# ------------------------------------------------------------------ 4. product_step
def _chain_device_graph(N=100, seed=11):
    rng = np.random.default_rng(seed)
    fg = _chain_graph(N)
    for i in range(5):                                       # dead-reckoned poses of the chain: a quarter turn and 10 m per step, z = i
        m = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
        th = i * math.pi / 2
        m[:3] = [sum(10.0 * math.cos(k * math.pi / 2) for k in range(i)), sum(10.0 * math.sin(k * math.pi / 2) for k in range(i)), float(i)]
        m[5] = math.atan2(math.sin(th), math.cos(th))
        fg.initVariable("x%d" % i, m[:, None] + rng.standard_normal((6, N)) * np.array([[0.3]] * 3 + [[0.02]] * 3))
    dg = R.DeviceGraph(fg)
    dg.upload_beliefs(fg)
    return fg, dg


@pytest.mark.parametrize("product,bandwidth", [("importance", "silverman"), ("importance", "lcv"), ("gibbs", "silverman")])
def test_product_step_coordinate_on_the_chain(product, bandwidth):
    """after conv_step, z, ω_x, ω_y of x1 .. x4 ARE the ZRP proposal (the one density covering them) and x, y, ω_z of x4 ARE its one XYYaw
    proposal, bit for bit; x0's z, ω_x, ω_y are its prior's (the joint result).  Under "off" every one of these lines is resampled from a
    6-D product and jittered."""
    N = 100
    fg, dg = _chain_device_graph(N)
    o = R.make_opts(N=N, solver=1, seed=SEED)
    dg.conv_step(o, sweep=0)
    prop = dg.prop[R.Pose3].cpu().numpy()
    dg.product_step(o, sweep=0, product=product, bandwidth=bandwidth, partial_product="coordinate")
    bel = dg.bel[R.Pose3].cpu().numpy()
    assert np.array_equal(dg.prop[R.Pose3].cpu().numpy(), prop) and np.isfinite(bel).all()
    ix = dg.packed.index
    for i in range(1, 5):
        assert np.array_equal(bel[ix["x%d" % i]][[2, 3, 4]], prop[8 + i][[2, 3, 4]]), i
    assert np.array_equal(bel[ix["x4"]][[0, 1, 5]], prop[7][[0, 1, 5]])
    assert np.array_equal(bel[ix["x0"]][[2, 3, 4]], prop[0][[2, 3, 4]])
    for i in range(4):                                                           # two densities: a new line, within the densities' range
        b = bel[ix["x%d" % i]]
        assert not np.array_equal(b[0], prop[2 * i + 2][0]) and np.abs(b[5]).max() <= math.pi
        assert abs(b[0].mean() - prop[2 * i + 2][0].mean()) < 1.0


def test_product_step_coordinate_keeps_the_heading_of_a_range_only_pose():
    """three Pose2Point2Range factors and nothing else on the pose: no density covers its heading, so the line stays, bit for bit"""
    N = 100
    rng = np.random.default_rng(5)
    res = {}
    for mode in ("coordinate", "off"):
        fg = _range_graph(N)
        fg.initVariable("x0", np.array([[0.5], [-0.5], [3.0]]) + rng.standard_normal((3, N)) * np.array([[1.0], [1.0], [0.4]]))
        for k, xy in enumerate(([10.0, 0.0], [0.0, 10.0], [-7.0, -7.0])):
            fg.initVariable("l%d" % k, np.array(xy)[:, None] + 0.1 * rng.standard_normal((2, N)))
        dg = R.DeviceGraph(fg); dg.upload_beliefs(fg)
        before = dg.bel[R.Pose2].cpu().numpy()
        o = R.make_opts(N=N, solver=1, seed=SEED)
        dg.conv_step(o, sweep=1)
        dg.product_step(o, sweep=1, partial_product=mode)
        res[mode] = (before, dg.bel[R.Pose2].cpu().numpy())
    before, after = res["coordinate"]
    assert np.array_equal(after[0, 2], before[0, 2])
    assert not np.array_equal(after[0, 0], before[0, 0]) and np.isfinite(after).all()
    before, after = res["off"]
    assert not np.array_equal(after[0, 2], before[0, 2])                        # today's product resamples and jitters it


def test_off_is_bit_equal_to_the_default():
    N = 100
    out = []
    for kw in ({}, {"partial_product": "off"}):
        fg, dg = _chain_device_graph(N)
        o = R.make_opts(N=N, solver=1, seed=SEED)
        dg.conv_step(o, sweep=0)
        dg.product_step(o, sweep=0, **kw)
        out.append(dg.bel[R.Pose3].cpu().numpy())
    assert np.array_equal(out[0], out[1])
    fg, dg = _chain_device_graph(N)
    with pytest.raises(ValueError, match="partial_product"):
        dg.product_step(R.make_opts(N=N), partial_product="coordinates")


# ------------------------------------------------------------------ 5. the reference's chain through solveGraph
def _solve_chain(**kw):
    N = 100
    fg = _chain_graph(N)
    dg = R.solveGraph(fg, n_sweeps=10, seed=SEED, partial_product="coordinate", **kw)
    assert dg.has_partial3()
    vals = {l: fg.getVal(l) for l in fg.variables}
    assert all(np.isfinite(v).all() for v in vals.values())
    z = [vals["x%d" % i][2].mean() for i in range(5)]
    m = vals["x4"][:3].mean(axis=1)
    dist = float(np.linalg.norm(m - [0.0, 0.0, 4.0]))
    print("solveGraph(coordinate, %s): mean z %s, x4 mean translation %s, distance from (0, 0, 4): %.4f" % (kw, np.round(z, 4), m, dist))
    return z, m, dist


def test_chain_solve_graph_coordinate():
    """test/testPartialPose3.jl:455-501 through solveGraph with the partial-aware product.  z of x_i is a copy of N = 100 samples of
    N(i, 0.1²): its mean has σ = 0.01, the bound 0.05 is 5σ (without the feature the means are about 2e-6: z never leaves 0).  The mean
    translation of x4 must lie within the reference's own 0.3 of (0, 0, 4) (:493).  Measured on the MI355X: mean z 1.002, 2.007, 2.999,
    3.979; x4 at (−0.038, −0.005, 3.979), 0.043 from (0, 0, 4)."""
    z, m, dist = _solve_chain()
    for i in range(1, 5):
        assert abs(z[i] - i) < 0.05, (i, z[i])
    assert dist < 0.3, (m, dist)                                                 # isapprox(..., atol=0.3): the 2-norm


def test_chain_solve_graph_coordinate_gibbs():
    """the same with product="gibbs" for stage 1 (stage 2 is the one definition under both settings).  Measured on the MI355X: the same
    z means (the ZRP copies); x4 at (−0.051, −0.023, 3.979), 0.060 from (0, 0, 4)."""
    z, m, dist = _solve_chain(product="gibbs")
    for i in range(1, 5):
        assert abs(z[i] - i) < 0.05, (i, z[i])
    assert dist < 0.3, (m, dist)                                                 # isapprox(..., atol=0.3): the 2-norm
