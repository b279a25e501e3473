"""The five-weight operator on the GPU (tb_kernel_w5, probe_cone_w5): the raw op at
the raw ops' shape and all four edge kinds, periodic axes and the roll identity,
both shift identities at the depth ceiling, captured graphs and set_weights()
between steps, the probe cone, LoopbackGroup ranks and the dynamic item queue.
Bitwise against the golden (models.reference weights=) on rough signed data.
(Every compiled instance once: tests/test_weights_instances.py.)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver, LoopbackGroup
from heat2d.ops import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cycles as Y  # noqa: E402
from weights_worker import NP, ROUGH, bits, problem, signed_field, signed_rect  # noqa: E402

pytestmark = pytest.mark.gpu
GSTEPS = 57
_GOLD = {}


def gold(n, dtype, arith, bc_x="dirichlet", bc_y="dirichlet", steps=GSTEPS, weights=ROUGH, T0=None):
    key = (n, dtype, arith, bc_x, bc_y, steps, tuple(weights), None if T0 is None else T0.tobytes())
    if key not in _GOLD:
        g = np.ascontiguousarray(R.owned(R.ftcs(problem(n, steps), steps, dtype=NP[dtype],
                                                T0=signed_field(n, dtype) if T0 is None else T0, arith=arith, bc_x=bc_x,
                                                bc_y=bc_y, weights=weights)))
        g.setflags(write=False)
        _GOLD[key] = g
    return _GOLD[key]


@pytest.fixture(scope="module", autouse=True)
def drop_goldens():
    yield
    _GOLD.clear()


def run(n, dtype, tb, arith, bc_x="dirichlet", bc_y="dirichlet", steps=GSTEPS, weights=ROUGH, ranks=1, T0=None, calls=None,
        prepare=False, **kw):
    p = problem(n, steps)
    T0 = signed_field(n, dtype) if T0 is None else T0
    sizes = [steps] if calls is None else list(calls)
    assert sum(sizes) == steps
    full = 0 if calls is None else sum(1 for m in sizes if m == tb)
    args = dict(dtype=dtype, backend="hip", tb=tb, arith=arith, bc_x=bc_x, bc_y=bc_y, weights=weights, device=0, **kw)
    s = LoopbackGroup(p, ranks, **args) if ranks > 1 else HeatSolver(p, **args)
    s.upload(T0)
    for m in sizes:
        if prepare:
            s.prepare(m)
        s.step(m)
    out = s.download()
    hists = [s.cycle_hist(i) for i in range(ranks)] if ranks > 1 else [s.cycle_hist()]
    s.close()
    for h in hists:
        assert full == 0 or (Y.ran(h, tb, full) and max(h) == tb), (tb, sizes, hists)
    return out


# ------------------------------------------------------------------ the raw op

def _raw_op(device, dtype, k, arith, row0, n=150, ncols=261, nrows=70):
    """One tb_step(weights=) launch on rows [row0, row0 + 70) of a 150 x 261 grid: k fused levels are k golden
    steps, and nothing is written outside the output rows but pinned values in the last vector's pad."""
    import torch

    from heat2d.ops import kernels as K
    dt = NP[dtype]
    rng = np.random.default_rng(7)
    T0 = (10.0 ** rng.uniform(-1, 1, (n + 2, ncols + 2)) * rng.choice([-1.0, 1.0], (n + 2, ncols + 2))).astype(dt)
    L = K.make_layout(nrows, ncols, halo=24, row0=row0, nrows_global=n)
    host = np.full((L.rows_alloc(), L.pitch), 3.25, dtype=dt)  # (pad columns and rows off the grid: finite)
    for a in range(L.rows_alloc()):
        g = row0 - L.halo + a  # global owned row; the frame-inclusive row is g + 1
        if -1 <= g <= n:
            host[a, L.cpad - 1:L.cpad + ncols + 1] = T0[g + 1]
    src = torch.from_numpy(host.reshape(-1).copy()).to(device)
    dst = torch.full_like(src, float("nan"))  # NaN guard bands around the rows written
    K.tb_step(src, dst, L, k, 0.0, arith=arith, weights=ROUGH)
    out = K.view2d(dst.cpu(), L).numpy().copy()
    T = T0.copy()
    for _ in range(k):
        T = R.ftcs_step(T, 0.0, arith, weights=ROUGH)
    own = out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols].copy()
    assert np.array_equal(bits(own), bits(T[row0 + 1:row0 + 1 + nrows, 1:-1])), (dtype, k, arith, row0)
    out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols] = np.nan
    rr, cc = np.nonzero(~np.isnan(out))
    assert ((rr >= L.halo) & (rr < L.halo + nrows)).all(), "kernel wrote outside its output rows"
    assert (cc >= L.cpad + ncols).all() and (cc < L.cpad + ncols + 8).all(), "kernel wrote beyond one vector of right pad"
    assert np.array_equal(bits(out[rr, cc]), bits(host[rr, cc])), "frame / pad write changed a value"


@pytest.mark.parametrize("k", [1, 2, 7, 16, 17, 20, 24])
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_raw_op(native, gpu, dtype, arith, k):
    """Windows at the first frame row, clear of both and at the last: with the frame-column strips and (fp64)
    the strips between them, all four edge kinds."""
    assert N.max_tb_w5() == 24  # (the last depth above is the ceiling)
    for row0 in (0, 40, 80):
        _raw_op("cuda:0", dtype, k, arith, row0)


# ------------------------------------------------------------------ the solver

BCS = [("periodic", "dirichlet"), ("dirichlet", "periodic"), ("periodic", "periodic")]


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", BCS, ids=["px", "py", "pxy"])
def test_periodic_axes_and_roll_identity(native, gpu, bc_x, bc_y, dtype, arith):
    n, tb = 261, 20
    calls = Y.calls(tb, GSTEPS, 2)
    got = run(n, dtype, tb, arith, bc_x, bc_y, calls=calls)
    assert np.array_equal(bits(got), bits(gold(n, dtype, arith, bc_x, bc_y)))
    a, b = (37 if bc_x == "periodic" else 0), (101 if bc_y == "periodic" else 0)
    T0 = signed_field(n, dtype)
    Tr = T0.copy()
    Tr[1:-1, 1:-1] = np.roll(R.owned(T0), (a, b), axis=(0, 1))
    if bc_x == "periodic" and bc_y != "periodic":  # (the pinned frame columns move with their rows)
        Tr[1:-1, 0], Tr[1:-1, -1] = np.roll(T0[1:-1, 0], a), np.roll(T0[1:-1, -1], a)
    if bc_y == "periodic" and bc_x != "periodic":
        Tr[0, 1:-1], Tr[-1, 1:-1] = np.roll(T0[0, 1:-1], b), np.roll(T0[-1, 1:-1], b)
    rolled = run(n, dtype, tb, arith, bc_x, bc_y, T0=Tr, calls=calls)
    assert np.array_equal(bits(rolled), bits(np.roll(got, (a, b), axis=(0, 1))))


def shifted(F, steps, axis, periodic):
    own = R.owned(F)
    if periodic:
        return np.roll(own, steps, axis=axis)
    out = np.empty_like(own)
    for k in range(own.shape[axis]):
        src = k - steps
        if axis == 0:
            out[k, :] = own[src, :] if src >= 0 else F[0, 1:-1]
        else:
            out[:, k] = own[:, src] if src >= 0 else F[1:-1, 0]
    return out


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "dirichlet"])
@pytest.mark.parametrize("which", ["columns", "rows"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_shift_identities_at_the_depth_ceiling(native, gpu, dtype, which, periodic):
    """(0, 0, 0, 1, 0) moves every row one column per step, (0, 0, 1, 0, 0) the field one row per step: two
    passes of depth 24 and a remainder on n = 301, in both forms."""
    w, axis = {"columns": ((0, 0, 0, 1, 0), 1), "rows": ((0, 0, 1, 0, 0), 0)}[which]
    bc = ["dirichlet", "dirichlet"]
    if periodic:
        bc[axis] = "periodic"
    tb = N.max_tb_w5()
    steps = 2 * tb + 3
    T0 = signed_field(301, dtype)
    want = shifted(T0, steps, axis, periodic)
    for arith in ("exact", "fma"):
        got = run(301, dtype, tb, arith, bc[0], bc[1], steps=steps, weights=w, calls=Y.calls(tb, steps, 2))
        assert np.array_equal(bits(got), bits(want)), arith


@pytest.mark.parametrize("kw", [dict(graph=True), dict(graph=True, autotune=1), dict(autotune=1)],
                         ids=["pair-graphs", "schedule-graph", "autotune"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_graphs_give_the_eager_bits(native, gpu, dtype, kw):
    got = run(261, dtype, 8, "fma", steps=GSTEPS, prepare=True, **kw)
    assert np.array_equal(bits(got), bits(gold(261, dtype, "fma")))


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_set_weights_between_steps_under_graphs(native, gpu, dtype):
    """Captured launches carry the weights by value: set_weights() between steps drops them and takes effect;
    None returns to the scalar-r run's bits."""
    n, tb = 261, 8
    p, T0 = problem(n, GSTEPS), signed_field(n, dtype)
    other = (0.2, 0.05, 0.3, 0.1, 0.3)
    s = HeatSolver(p, dtype=dtype, backend="hip", tb=tb, arith="exact", device=0, graph=True, weights=ROUGH)
    s.upload(T0)
    s.prepare(20)
    assert s.step_cycles(20) == Y.balanced(tb, 20, graph=True)
    s.step(20)
    s.set_weights(other)
    s.prepare(20)
    s.step(20)
    s.set_weights(None)
    assert s.info()["weights"]["set"] is False
    s.prepare(17)
    s.step(17)
    got = s.download()
    s.close()
    T = R.ftcs(p, 20, dtype=NP[dtype], T0=T0, arith="exact", weights=ROUGH)
    T = R.ftcs(p, 20, dtype=NP[dtype], T0=T, arith="exact", weights=other)
    plain = HeatSolver(p, dtype=dtype, backend="hip", tb=tb, arith="exact", device=0, graph=True)
    plain.upload(T)
    plain.prepare(17)
    plain.step(17)
    want = plain.download()
    plain.close()
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(want), bits(R.owned(R.ftcs(p, 17, dtype=NP[dtype], T0=T, arith="exact"))))


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_probes(native, gpu, dtype, arith):
    """The cone on the device: probes on the first and last owned row and column, under Dirichlet and under
    periodic axes; the last row of a call equals download() at the probes."""
    n = 261
    pts = np.array([[1, 1], [1, 261], [261, 1], [261, 261], [1, 130], [130, 261], [100, 100], [2, 261]])
    for bc_x, bc_y in (("dirichlet", "dirichlet"), ("periodic", "periodic"), ("periodic", "dirichlet")):
        s = HeatSolver(problem(n, GSTEPS), dtype=dtype, backend="hip", tb=20, arith=arith, device=0, bc_x=bc_x, bc_y=bc_y,
                       weights=ROUGH, probes=pts, probe_steps=GSTEPS)
        s.upload(signed_field(n, dtype))
        for m in Y.calls(20, GSTEPS, 2):
            s.step(m)
            assert np.array_equal(s.probe_history()[-1], s.download()[pts[:, 0] - 1, pts[:, 1] - 1])
        H = s.probe_history()
        s.close()
        want = R.probe_history(problem(n, GSTEPS), GSTEPS, pts, dtype=NP[dtype], T0=signed_field(n, dtype), arith=arith,
                               bc_x=bc_x, bc_y=bc_y, weights=ROUGH)
        assert np.array_equal(bits(H), bits(want)), (bc_x, bc_y)


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_raw_probe_cone(native, gpu, dtype, arith):
    """The device cone against its CPU twin on a 70 x 261 window."""
    import torch

    from heat2d.ops import kernels as K
    L = K.make_layout(70, 261, halo=24)
    rng = np.random.default_rng(3)
    host = (10.0 ** rng.uniform(-1, 1, L.elems()) * rng.choice([-1.0, 1.0], L.elems())).astype(NP[dtype])
    f = torch.from_numpy(host)
    pts = np.array([[1, 1], [70, 261], [35, 1], [1, 100]])
    for bc_x, bc_y in (("dirichlet", "dirichlet"), ("dirichlet", "periodic")):
        kw = dict(arith=arith, bc_x=bc_x, bc_y=bc_y, weights=ROUGH)
        want = K.probe_cone(f, L, 20, 0.0, pts, **kw).numpy()
        assert np.array_equal(bits(K.probe_cone(f.cuda(), L, 20, 0.0, pts, **kw).cpu().numpy()), bits(want))


@pytest.mark.parametrize("bc_x", ["dirichlet", "periodic"])
@pytest.mark.parametrize("ranks", [2, 3])
def test_loopback_ranks(native, gpu, ranks, bc_x):
    for dtype in ("fp64", "fp32"):
        one = run(261, dtype, 8, "fma", bc_x=bc_x)
        assert np.array_equal(bits(one), bits(gold(261, dtype, "fma", bc_x)))
        assert np.array_equal(bits(run(261, dtype, 8, "fma", bc_x=bc_x, ranks=ranks)), bits(one))


# ------------------------------------------------------------------ fresh processes

def worker(tmp_path, a, **env):
    out = subprocess.run([sys.executable, os.path.join(HERE, "weights_worker.py"), str(tmp_path), json.dumps(a)],
                         env=dict(os.environ, HEAT2D_PLAN_CACHE="off", **env), capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    return json.loads((tmp_path / "info.json").read_text()), np.load(tmp_path / "result.npy")


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_dynamic_queue_under_graph_replay(native, gpu, tmp_path, dtype):
    """301 rows x 2897 columns, HEAT2D_DYNAMIC=1 HEAT2D_MAX_WAVES=40, graph=True: the dynamic item queue (more
    items than waves) replayed from the captured pair graph, every rect on tb_kernel_w5."""
    tb = 8
    a = {"n": 2897, "rows": 301, "steps": 4 * tb + 5, "tb": tb, "dtype": dtype, "arith": "exact", "graph": True,
         "calls": [20, 17]}
    info, got = worker(tmp_path, a, HEAT2D_DYNAMIC="1", HEAT2D_MAX_WAVES="40")
    plan = info["plan"]
    assert info["first_call_cycles"] == Y.balanced(tb, 20, graph=True) == [8, 8, 4], info
    Y.assert_ran(info["cycle_hist"], tb, 2)
    print(f"{dtype}: plan {plan}")
    assert plan["dynamic"] == 1 and plan["main_waves"] == 40 and plan["main_items"] > plan["main_waves"]
    assert plan["pipe"] == 0 and info["info"]["weights"]["set"]
    want = R.owned(R.ftcs(problem(2897, a["steps"]), a["steps"], dtype=NP[dtype], T0=signed_rect(2897, 301, dtype),
                          arith="exact", weights=ROUGH))
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("order", ["edge-first", "concurrent", "single"])
def test_split_orders_and_single_launch(native, gpu, tmp_path, order):
    a = {"n": 261, "steps": GSTEPS, "tb": 8, "dtype": "fp64", "arith": "fma"}
    info, got = worker(tmp_path, a, HEAT2D_SPLIT_ORDER=order, **({"HEAT2D_BANDS": "3"} if order == "single" else {}))
    print(f"split order {order}: plan {info['plan']}")
    assert info["plan"]["order"] == order
    assert np.array_equal(bits(got), bits(gold(261, "fp64", "fma")))


def test_forced_pipe_falls_back(native, gpu, tmp_path):
    """HEAT2D_PIPE=1 with weights: the wave-pair kernel is not offered."""
    a = {"n": 700, "steps": GSTEPS, "tb": 20, "dtype": "fp64", "arith": "exact"}
    info, got = worker(tmp_path, a, HEAT2D_PIPE="1")
    assert info["plan"]["pipe"] == 0, info["plan"]
    assert np.array_equal(bits(got), bits(gold(700, "fp64", "exact")))
