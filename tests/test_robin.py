"""Robin (convective) walls on either axis (bc_x: rows, decomposed over ranks;
bc_y: columns), bitwise against the NumPy golden at every pass depth, launch
plan and rank count.

Convention: the insulated geometry (the wall half a cell outside the first and
last owned point) with the affine ghost value G = a * C + b of the adjacent
owned point C beyond the wall — the product rounded, then the add ("exact"), or
one fma ("fma") — refreshed before every single step (models.reference.ftcs
robin=). A frame refreshed once per fused pass is stale from level 2 on, so the
engine forms the ghost inside the march (tb_impl.hpp March ROB).

Data: rough values 10**uniform(-1, 1), frame included; r = 0.2371; four
different pairs PAIRS, all with |a| <= 1; np.array_equal unless a case says
otherwise. STEPS = 23 on the CPU (two cycles of depth 8 and a remainder), 57 on
the GPU (two cycles of depth 24 and a remainder).

Bounds. u = eps / 2 of the dtype.
  linear steady state: the four adds of the sum and the ghost's two operations
    are each relative u on values of size max|T|; the exact update of the
    steady field is 0, so one step moves no point by more than 16 u max|T|.
  heat balance: summing the exact update over the owned points, interior faces
    cancel and every wall face leaves r (G - C); each of the n^2 points rounds
    a handful of operations on values <= 8 max|T| scaled by r < 1/4:
    |sum T' - sum T - r sum(G - C)| <= 4 n^2 u max|T|, sums in float64.
"""
import os
import sys

import numpy as np
import pytest

import heat2d
from heat2d.models import reference as R
from heat2d.models.heat2d import (HeatSolver, LoopbackGroup, robin_from_flux, robin_from_h, robin_wall_temperature)
from heat2d.ops import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cycles as Y  # noqa: E402
from periodic_worker import problem, rough_field  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
PAIRS = {"x_lo": (0.8125, 0.37), "x_hi": (0.6, -0.21), "y_lo": (0.93, 0.055), "y_hi": (-0.45, 1.3)}
IDENT = {k: (1.0, -0.0) for k in PAIRS}
COMBOS = [("robin", "robin"), ("robin", "dirichlet"), ("dirichlet", "robin"), ("robin", "periodic"),
          ("periodic", "robin"), ("robin", "insulated"), ("insulated", "robin")]
IDS = ["xy", "x", "y", "x-py", "px-y", "x-iy", "ix-y"]
GPU_COMBOS = [c for c in COMBOS if c[0] == "robin" or c == ("dirichlet", "robin")]  # RR, RD, DR, R/periodic, R/insulated
GPU_IDS = ["xy", "x", "y", "x-py", "x-iy"]
STEPS, GSTEPS = 23, 57
SIGMA = 0.2371

_GOLD = {}


def pairs_for(bc_x, bc_y, pairs=PAIRS):
    """The pairs of exactly the Robin sides of (bc_x, bc_y)."""
    return {k: v for k, v in pairs.items() if (bc_x if k[0] == "x" else bc_y) == "robin"}


def gold(n, dtype, bc_x, bc_y, steps=STEPS, sigma=SIGMA, arith="exact", framed=False, pairs=PAIRS):
    """The golden run from rough_field (computed once, read-only): owned points, or with its frame."""
    key = (n, dtype, bc_x, bc_y, steps, sigma, arith, tuple(sorted(pairs.items())))
    if key not in _GOLD:
        g = R.ftcs(problem(n, steps, sigma), steps, dtype=NP[dtype], T0=rough_field(n, dtype), arith=arith, bc_x=bc_x,
                   bc_y=bc_y, robin=pairs_for(bc_x, bc_y, pairs))
        g = np.ascontiguousarray(g)
        g.setflags(write=False)
        _GOLD[key] = g
    return _GOLD[key] if framed else R.owned(_GOLD[key])


@pytest.fixture(scope="module", autouse=True)
def drop_goldens():
    yield
    _GOLD.clear()


def run(n, dtype, backend, tb, bc_x, bc_y, steps=STEPS, sigma=SIGMA, arith="exact", ranks=1, prepare=False, calls=None,
        pairs=PAIRS, framed=False, **kw):
    """One run of `steps` steps, as one step(steps) call or as the step() calls of `calls`
    (tests/cycles.py calls()): then cycle_hist() must show the full cycles of depth tb."""
    p = problem(n, steps, sigma)
    T0 = rough_field(n, dtype)
    dev = dict(device=0) if backend == "hip" else {}
    rob = None if pairs is None else pairs_for(bc_x, bc_y, pairs)
    sizes = [steps] if calls is None else list(calls)
    assert sum(sizes) == steps
    full = 0 if calls is None else sum(1 for m in sizes if m == tb)
    if ranks > 1:
        s = LoopbackGroup(p, ranks, dtype=dtype, backend=backend, tb=tb, arith=arith, bc_x=bc_x, bc_y=bc_y, robin=rob,
                          **dev, **kw)
        s.upload(T0)
        for m in sizes:
            s.step(m)
        out, hists, slabs = s.download(), [s.cycle_hist(i) for i in range(ranks)], s.slabs()
        s.close()
        for h in hists:
            assert full == 0 or (Y.ran(h, tb, full) and max(h) == tb), (tb, sizes, hists)
        return (out, slabs) if framed else out
    s = HeatSolver(p, dtype=dtype, backend=backend, tb=tb, arith=arith, bc_x=bc_x, bc_y=bc_y, robin=rob, **dev, **kw)
    s.upload(T0)
    for m in sizes:
        if prepare:
            s.prepare(m)
        s.step(m)
    out, hist = (s.download_field() if framed else s.download()), s.cycle_hist()
    s.close()
    assert full == 0 or (Y.ran(hist, tb, full) and max(hist) == tb), (tb, sizes, hist)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ------------------------------------------------------------------ CPU: the golden

def test_helpers_by_hand():
    p = problem(101, 1)  # dx = 1 / 100
    assert p.delta == 0.01
    a, b = robin_from_h(p, 50.0, 300.0)  # beta = 0.5
    assert a == 1.5 / 2.5 and b == 2 * 0.5 * 300.0 / 2.5 == 120.0
    assert robin_from_h(p, 0.0, 7.0) == (1.0, 0.0)
    assert robin_from_flux(p, 25.0) == (1.0, 0.25)
    assert robin_wall_temperature(3.5) == (-1.0, 7.0)
    assert heat2d.robin_from_h is robin_from_h and heat2d.robin_wall_temperature is robin_wall_temperature


def test_robin_keys_and_values():
    T0 = rough_field(9, "fp64")
    with pytest.raises(ValueError, match="x_hi"):
        R.wrap_frame(T0, "robin", "dirichlet", {"x_lo": (1, 0)})
    with pytest.raises(ValueError, match="y_lo"):
        R.wrap_frame(T0, "robin", "dirichlet", {"x_lo": (1, 0), "x_hi": (1, 0), "y_lo": (1, 0)})
    with pytest.raises(ValueError, match="x_lo"):
        R.ftcs_step(T0, 0.2, bc_x="robin")
    with pytest.raises(ValueError, match="finite"):
        R.wrap_frame(T0, "robin", "dirichlet", {"x_lo": (np.inf, 0), "x_hi": (1, 0)})
    with pytest.raises(ValueError, match="finite"):  # finite in float64, not in the run's dtype
        R.wrap_frame(T0.astype(np.float32), "robin", "dirichlet", {"x_lo": (1e300, 0), "x_hi": (1, 0)})
    with pytest.raises(ValueError, match="bc_y"):
        R.wrap_frame(T0, "robin", "mirror", {"x_lo": (1, 0), "x_hi": (1, 0)})
    with pytest.raises(ValueError, match="jacobi"):
        R.ftcs_step(T0, 0.25, "jacobi", "robin", "dirichlet", robin={"x_lo": (1, 0), "x_hi": (1, 0)})
    for kw in (dict(source=np.zeros_like(T0)), dict(rmap=np.full_like(T0, 0.2)),
               dict(faces=(np.full_like(T0, 0.1), np.full_like(T0, 0.1)))):
        with pytest.raises(ValueError, match="Dirichlet"):
            R.ftcs_step(T0, 0.2, "exact", "robin", "dirichlet", robin={"x_lo": (1, 0), "x_hi": (1, 0)}, **kw)
    # without robin= nothing changes
    assert R.wrap_frame(T0) is T0
    assert np.array_equal(R.wrap_frame(T0, "insulated", "periodic"), R.wrap_frame(T0, "insulated", "periodic", None, "fma"))


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_frame_holds_the_ghosts(dtype, arith):
    """x first, then y over the filled rows: the corner is the y ghost of the x ghost."""
    t = NP[dtype]
    T = gold(31, dtype, "robin", "robin", steps=5, arith=arith, framed=True)
    g = lambda k, C: R.robin_ghost(C, *PAIRS[k], arith)  # noqa: E731
    assert np.array_equal(T[0, 1:-1], g("x_lo", T[1, 1:-1])) and np.array_equal(T[-1, 1:-1], g("x_hi", T[-2, 1:-1]))
    assert np.array_equal(T[:, 0], g("y_lo", T[:, 1])) and np.array_equal(T[:, -1], g("y_hi", T[:, -2]))  # frame rows too
    if arith == "exact":
        assert T[0, 0] == t(PAIRS["y_lo"][0]) * (t(PAIRS["x_lo"][0]) * T[1, 1] + t(PAIRS["x_lo"][1])) + t(PAIRS["y_lo"][1])
    # one Robin axis: the Dirichlet axis keeps its frame, with ghosts at its ends
    T0 = rough_field(31, dtype)
    T = gold(31, dtype, "dirichlet", "robin", steps=5, arith=arith, framed=True)
    assert np.array_equal(T[0, 1:-1], T0[0, 1:-1]) and np.array_equal(T[:, 0], g("y_lo", T[:, 1]))


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_insulated_identity(dtype):
    """(1, -0.0) on every Robin side is the insulated wall in bits: 1 * C + (-0.0) and fma(1, C, -0.0)
    return every C unchanged, both zeros included. (1, +0.0) differs only where a -0.0 sits at a wall."""
    t = NP[dtype]
    ext = np.array([np.finfo(t).tiny, -np.finfo(t).max, np.finfo(t).smallest_subnormal], dtype=t)
    assert np.array_equal(bits(R.robin_ghost(ext, 1.0, -0.0, "exact")), bits(ext))
    C = np.array([0.0, -0.0, 1.5, -2.25e-30, 7.0e20, -1.0 / 3.0], dtype=t)  # (reference.fma emulates the normal range)
    for arith in ("exact", "fma"):
        assert np.array_equal(bits(R.robin_ghost(C, 1.0, -0.0, arith)), bits(C)), arith
        plus = R.robin_ghost(C, 1.0, 0.0, arith)
        assert np.array_equal(bits(plus) != bits(C), np.signbit(C) & (C == 0)), arith
    T0 = rough_field(77, dtype)
    T0[1, 5] = T0[40, 1] = -0.0
    p = problem(77, 8)
    a = R.ftcs(p, 8, dtype=t, T0=T0, bc_x="robin", bc_y="robin", robin=IDENT)
    assert np.array_equal(bits(a), bits(R.ftcs(p, 8, dtype=t, T0=T0, bc_x="insulated", bc_y="insulated")))
    # the contracted form: at r = 1/4 the insulated golden's "fma" (the exact expression) has the fused bits
    p4 = problem(77, 8, 0.25)
    a = R.ftcs(p4, 8, dtype=t, T0=T0, arith="fma", bc_x="robin", bc_y="robin", robin=IDENT)
    assert np.array_equal(bits(a), bits(R.ftcs(p4, 8, dtype=t, T0=T0, arith="fma", bc_x="insulated", bc_y="insulated")))
    # (1, +0.0): one step differs from the insulated one in the frame entries beside the two -0.0 only
    plus = {k: (1.0, 0.0) for k in PAIRS}
    b = R.wrap_frame(T0, "robin", "robin", plus)
    i = R.wrap_frame(T0, "insulated", "insulated")
    assert sorted(map(tuple, np.argwhere(bits(b) != bits(i)))) == [(0, 5), (40, 0)]


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_ambient_fixed_point(dtype, arith):
    """a = 0.5, b = 1.5 and the owned points uniformly 3.0: the ghost is 3.0 and every step returns 3.0 in bits."""
    T = np.full((35, 35), 3.0, dtype=NP[dtype])
    rob = {k: (0.5, 1.5) for k in PAIRS}
    for _ in range(6):
        T = R.ftcs_step(T, SIGMA, arith, "robin", "robin", robin=rob)
        assert np.array_equal(bits(R.owned(T)), bits(np.full((33, 33), 3.0, dtype=NP[dtype])))


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_linear_steady_state(dtype, arith):
    """y Robin (1, -0.0), x Robin from robin_from_h with two (beta, t_inf) pairs, a field linear in the row
    index whose two coefficients solve the two ghost relations in float64: one golden step moves no point by
    more than 16 u max|T|."""
    n, t = 77, NP[dtype]
    p = problem(n, 1)
    lo = robin_from_h(p, 0.3 / p.delta, 2.0)   # beta = 0.3
    hi = robin_from_h(p, 0.8 / p.delta, 9.0)   # beta = 0.8
    # T_i = c0 + c1 i (i = 1..n owned): ghost relations T_0 = a_lo T_1 + b_lo, T_{n+1} = a_hi T_n + b_hi
    A = np.array([[1 - lo[0], -lo[0]], [1 - hi[0], (n + 1) - hi[0] * n]])
    c0, c1 = np.linalg.solve(A, np.array([lo[1], hi[1]]))
    T = np.broadcast_to((c0 + c1 * np.arange(n + 2))[:, None], (n + 2, n + 2)).astype(t)
    rob = {"x_lo": lo, "x_hi": hi, "y_lo": (1.0, -0.0), "y_hi": (1.0, -0.0)}
    T1 = R.ftcs_step(T, SIGMA, arith, "robin", "robin", robin=rob)
    u = float(np.finfo(t).eps) / 2
    moved = float(np.abs(R.owned(T1).astype(np.float64) - R.owned(T).astype(np.float64)).max())
    bound = 16 * u * float(np.abs(T).max())
    print(f"linear steady state {dtype} {arith}: max move {moved:.3e}, bound {bound:.3e}")
    assert c1 != 0 and moved <= bound


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_heat_balance(dtype, arith):
    """sum(T') - sum(T) over the owned points = r * sum over wall-adjacent points of (G - C), within 4 n^2 u max|T|."""
    n, t = 77, NP[dtype]
    T = R.wrap_frame(rough_field(n, dtype), "robin", "robin", PAIRS, arith)
    T1 = R.ftcs_step(T, SIGMA, arith, "robin", "robin", robin=PAIRS)
    f = T.astype(np.float64)
    flux = ((f[0, 1:-1] - f[1, 1:-1]).sum() + (f[-1, 1:-1] - f[-2, 1:-1]).sum() + (f[1:-1, 0] - f[1:-1, 1]).sum() +
            (f[1:-1, -1] - f[1:-1, -2]).sum())
    got = R.owned(T1).astype(np.float64).sum() - f[1:-1, 1:-1].sum()
    want = float(t(SIGMA)) * flux
    bound = 4 * n * n * float(np.finfo(t).eps) / 2 * float(np.abs(R.owned(T)).max())
    print(f"heat balance {dtype} {arith}: change {got:.6e}, r * wall flux {want:.6e}, |diff| {abs(got - want):.3e}, bound {bound:.3e}")
    assert abs(got - want) <= bound


def walls_differing(a, b):
    """Which walls have a wall-adjacent owned point where the owned arrays a and b differ."""
    d = a != b
    return {"x_lo": bool(d[0].any()), "x_hi": bool(d[-1].any()), "y_lo": bool(d[:, 0].any()), "y_hi": bool(d[:, -1].any())}


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_negative_controls(dtype):
    """n = 77, 8 steps, rough data, PAIRS. Each variant differs from the golden at one or more wall-adjacent
    points of every wall it concerns. Measured shares of the 4 * 77 - 4 = 304 wall-adjacent points that differ
    (fp64 / fp32): frozen ghost 100 % / 100 %, lo/hi swapped on x 60 % / 60 %, x pairs given to y 60 % / 60 %
    (after 8 steps the change has reached the ends of the other axis' wall lines too), fma for exact 39 % /
    31 %, b before the multiply 100 % / 100 %."""
    n, K, t = 77, 8, NP[dtype]
    p, T0 = problem(n, K), rough_field(n, dtype)
    g = gold(n, dtype, "robin", "robin", steps=K)
    ring = np.zeros((n, n), bool)
    ring[0] = ring[-1] = ring[:, 0] = ring[:, -1] = True

    def share(v):
        return 100.0 * float(np.mean((v != g)[ring]))

    # the ghost frozen over a 4-step pass: the frame refreshed once per 4 steps, then 4 Dirichlet steps
    T = T0
    for q in range(K):
        if q % 4 == 0:
            T = R.wrap_frame(T, "robin", "robin", PAIRS)
        T = R.ftcs_step(T, p.r)
    frozen = R.owned(T)
    swapped = R.owned(R.ftcs(p, K, dtype=t, T0=T0, bc_x="robin", bc_y="robin",
                             robin=dict(PAIRS, x_lo=PAIRS["x_hi"], x_hi=PAIRS["x_lo"])))
    x_to_y = R.owned(R.ftcs(p, K, dtype=t, T0=T0, bc_x="robin", bc_y="robin",
                            robin=dict(PAIRS, y_lo=PAIRS["x_lo"], y_hi=PAIRS["x_hi"])))
    fma = gold(n, dtype, "robin", "robin", steps=K, arith="fma")
    # b added before the multiply: G = a * (C + b)
    T = T0
    for _ in range(K):
        o = T[1:-1, 1:-1]
        rows = np.concatenate([t(PAIRS["x_lo"][0]) * (o[:1] + t(PAIRS["x_lo"][1])), o,
                               t(PAIRS["x_hi"][0]) * (o[-1:] + t(PAIRS["x_hi"][1]))], axis=0)
        T = np.concatenate([t(PAIRS["y_lo"][0]) * (rows[:, :1] + t(PAIRS["y_lo"][1])), rows,
                            t(PAIRS["y_hi"][0]) * (rows[:, -1:] + t(PAIRS["y_hi"][1]))], axis=1)
        T = R.ftcs_step(T, p.r)
    b_first = R.owned(T)
    for name, v, walls in (("frozen ghost", frozen, PAIRS), ("lo/hi swapped on x", swapped, ("x_lo", "x_hi")),
                           ("x pairs given to y", x_to_y, ("y_lo", "y_hi")), ("fma for exact", fma, PAIRS),
                           ("b before the multiply", b_first, PAIRS)):
        w = walls_differing(v, g)
        print(f"{name} ({dtype}): differs at {share(v):.0f} % of the wall-adjacent points; walls {w}")
        assert all(w[k] for k in walls), (name, w)


# ------------------------------------------------------------------ CPU: the twin

@pytest.mark.parametrize("tb", [1, 2, 7, 8])
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS, ids=IDS)
def test_cpu_twin_bitwise(native, bc_x, bc_y, dtype, arith, tb):
    for n in (77, 301):
        got = run(n, dtype, "cpu", tb, bc_x, bc_y, arith=arith, calls=Y.calls(tb, STEPS, 2))
        assert np.array_equal(got, gold(n, dtype, bc_x, bc_y, arith=arith)), n


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", [("robin", "robin"), ("robin", "dirichlet")], ids=["xy", "x"])
def test_cpu_twin_three_uneven_ranks(native, bc_x, bc_y, dtype, arith):
    """77 rows on 3 loopback ranks (26 / 26 / 25): Robin x only on the outer ranks."""
    got, slabs = run(77, dtype, "cpu", 7, bc_x, bc_y, arith=arith, ranks=3, framed=True)
    assert [m for _, m in slabs] == [26, 26, 25]
    assert np.array_equal(got, gold(77, dtype, bc_x, bc_y, arith=arith))


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_twin_insulated_identity(native, dtype, arith):
    """(1, -0.0) through the twin: the bits of bc = "insulated" in both forms, at a fused depth."""
    a = run(77, dtype, "cpu", 8, "robin", "robin", arith=arith, pairs=IDENT)
    b = run(77, dtype, "cpu", 8, "insulated", "insulated", arith=arith, pairs=None)
    assert np.array_equal(bits(a), bits(b))
    assert not np.array_equal(a, gold(77, dtype, "robin", "robin", arith=arith))


def test_cpu_frame_roundtrip(native):
    """upload() ignores the frame entries of a Robin axis and keeps those of a Dirichlet one;
    download_field() returns the ghost values / the kept frame, after upload and after the march."""
    n, T0 = 40, rough_field(40, "fp64")
    for arith in ("exact", "fma"):
        for bc_x, bc_y in COMBOS:
            rob = pairs_for(bc_x, bc_y)
            s = HeatSolver(problem(n, 9), backend="cpu", tb=4, arith=arith, bc_x=bc_x, bc_y=bc_y, robin=rob)
            s.upload(T0)
            assert np.array_equal(s.download_field(), R.wrap_frame(T0, bc_x, bc_y, rob, arith)), (bc_x, bc_y, arith)
            s.step(9)
            want = R.ftcs(problem(n, 9), 9, T0=T0, arith=arith, bc_x=bc_x, bc_y=bc_y, robin=rob)
            assert np.array_equal(s.download_field(), want), (bc_x, bc_y, arith)
            s.close()


def test_info_and_auto(native):
    s = HeatSolver(problem(40, 1), backend="cpu", dtype="fp32", bc_x="robin", robin={"x_lo": (0.1, 0.2), "x_hi": (0.3, 1 / 3)})
    i = s.info()
    assert (i["bc_x"], i["bc_y"]) == ("robin", "dirichlet")
    f = np.float32
    assert i["robin"] == {"x_lo": (float(f(0.1)), float(f(0.2))), "x_hi": (float(f(0.3)), float(f(1 / 3))),
                          "max_tb": N.max_tb_rob()}
    assert s.robin == {k: v for k, v in i["robin"].items() if k != "max_tb"}
    assert i["arith"] == N.ARITH["exact"]  # auto at r = 0.2371
    s.close()
    s = HeatSolver(problem(40, 1, 0.25), backend="cpu", bc_y="robin", robin=pairs_for("dirichlet", "robin"))
    assert s.info()["arith"] == N.ARITH["fma"] and s.info()["robin"]["y_hi"] == PAIRS["y_hi"]  # never jacobi
    s.close()
    s = HeatSolver(problem(40, 1), backend="cpu", bc_x="insulated")
    assert s.info()["robin"] == {"max_tb": 0}
    s.close()
    g = LoopbackGroup(problem(40, 1, 0.25), 2, backend="cpu", bc_x="robin", bc_y="robin", robin=PAIRS)
    assert g.arith_code(1) == N.ARITH["fma"] and g.robin_info(1)["x_hi"] == PAIRS["x_hi"]
    g.close()


def test_refusals(native):
    p = problem(80, 4)
    rx = dict(bc_x="robin", robin=pairs_for("robin", "dirichlet"))
    for arith in ("jacobi", "fast"):
        with pytest.raises(RuntimeError, match="Robin"):
            HeatSolver(problem(80, 4, 0.25), backend="cpu", arith=arith, **rx)
    with pytest.raises(RuntimeError, match="Robin"):
        HeatSolver(p, backend="cpu", engine="jit", **rx)
    with pytest.raises(RuntimeError, match="Robin"):
        HeatSolver(p, backend="cpu", copy_swap=True, **rx)
    F = np.full((82, 82), 0.1)
    for kw in (dict(source=np.zeros((82, 82))), dict(rmap=F), dict(faces=(F, F))):
        with pytest.raises(RuntimeError, match="Dirichlet"):
            HeatSolver(p, backend="cpu", **rx, **kw)
    with pytest.raises(ValueError, match="x_hi"):
        HeatSolver(p, backend="cpu", bc_x="robin", robin={"x_lo": (1, 0)})
    with pytest.raises(ValueError, match="y_lo"):
        HeatSolver(p, backend="cpu", bc_x="robin", robin=PAIRS)
    with pytest.raises(ValueError, match="x_lo"):
        HeatSolver(p, backend="cpu", robin={"x_lo": (1, 0)})  # no Robin axis
    with pytest.raises(ValueError, match="finite"):
        HeatSolver(p, backend="cpu", bc_x="robin", robin={"x_lo": (1, float("nan")), "x_hi": (1, 0)})
    with pytest.raises(ValueError, match="x_lo"):
        LoopbackGroup(p, 2, backend="cpu", bc_x="robin")
    with pytest.raises(ValueError, match="bc_y"):
        HeatSolver(p, backend="cpu", bc_y="neumann")


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_probes(native, dtype, arith):
    """The history of probes at the walls (one beside a corner) against probe_history(robin=); its last row
    equals download() at the probes."""
    n, steps = 77, 19
    pts = np.array([[1, 1], [1, 40], [77, 77], [30, 1], [52, 77], [40, 40], [77, 2]])
    for bc_x, bc_y in (("robin", "robin"), ("robin", "insulated"), ("periodic", "robin")):
        rob = pairs_for(bc_x, bc_y)
        s = HeatSolver(problem(n, steps), dtype=dtype, backend="cpu", tb=7, arith=arith, bc_x=bc_x, bc_y=bc_y, robin=rob,
                       probes=pts, probe_steps=steps)
        s.upload(rough_field(n, dtype))
        s.step(steps)
        H, out = s.probe_history(), s.download()
        s.close()
        want = R.probe_history(problem(n, steps), steps, pts, dtype=NP[dtype], T0=rough_field(n, dtype), arith=arith,
                               bc_x=bc_x, bc_y=bc_y, robin=rob)
        assert np.array_equal(H, want), (bc_x, bc_y)
        assert np.array_equal(H[-1], out[pts[:, 0] - 1, pts[:, 1] - 1])


def raw_window(dtype, seed=3):
    from heat2d.ops import kernels as K
    L = K.make_layout(70, 261, halo=24)
    host = (10.0 ** np.random.default_rng(seed).uniform(-1, 1, L.elems())).astype(NP[dtype])
    return K, L, host


@pytest.mark.parametrize("arith", ["exact", "fma"])
def test_raw_op_cpu(native, arith):
    """The CPU raw op with bc = 16 | 32 on a 70 x 261 window: 20 fused levels = 20 golden steps, and the frame
    of the rows written holds the ghosts. The raw probe cone gives the same values at the probes."""
    import torch
    K, L, host = raw_window("fp64")
    f = torch.from_numpy(host)
    own = K.view2d(f, L).numpy()[24:94, 32:32 + 261].copy()
    g = f.clone()
    K.tb_step(f, g, L, 20, SIGMA, arith=arith, bc_x="robin", bc_y="robin", robin=PAIRS)
    T = np.pad(own, 1, mode="edge")
    hist = []
    pts = np.array([[1, 1], [70, 261], [35, 1], [1, 100]])
    for _ in range(20):
        T = R.ftcs_step(T, SIGMA, arith, "robin", "robin", robin=PAIRS)
        hist.append(T[pts[:, 0], pts[:, 1]])
    T = R.wrap_frame(T, "robin", "robin", PAIRS, arith)
    assert np.array_equal(K.view2d(g, L).numpy()[23:95, 31:32 + 262], T)  # the owned points and their ghosts
    H = K.probe_cone(f, L, 20, SIGMA, pts, arith=arith, bc_x="robin", bc_y="robin", robin=PAIRS)
    assert np.array_equal(H.numpy(), np.array(hist))
    with pytest.raises(ValueError, match="x_hi"):
        K.tb_step(f, g, L, 4, SIGMA, bc_x="robin", robin={"x_lo": (1, 0)})
    with pytest.raises(ValueError, match="Dirichlet"):
        K.tb_step(f, g, L, 4, SIGMA, bc_x="robin", robin=pairs_for("robin", "dirichlet"), source=f.clone())


def py(cwd, *args):
    import subprocess
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2")
    return subprocess.run([sys.executable, "-m", "heat2d", *args], cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=300)


def cli(cwd, *args):
    import subprocess
    return subprocess.run([N.CLI_PATH, "--cpu", *args], cwd=cwd, capture_output=True, text=True, timeout=300)


DRIVER_FLAGS = [f"--robin-{k.replace('_', '-')}={a},{b}" for k, (a, b) in PAIRS.items()]  # (= form: a may be negative)
DRIVER_BC = ["--bc-x", "robin", "--bc-y", "robin"]


def driver(which):
    """(run, the flags both drivers share) of the native CLI or the Python driver, on the CPU twin in fp32."""
    base = ["--arith", "exact", "--ic", "hat-cuda", "--quiet", "--dtype", "fp32"]
    return (cli, base) if which == "cli" else (py, ["--backend", "cpu", *base])


@pytest.mark.parametrize("writer", ["cli", "py"])
def test_checkpoint_written_by_one_driver_resumed_by_the_other(native, tmp_path, writer):
    """meta.json records the converted pairs exactly (hex floats); the other driver's restart takes them from
    there and reaches the golden bitwise; a contradicting flag fails before the first step, the same flag
    again does not."""
    import json

    from heat2d.utils import checkpoint, io
    (tmp_path / "input.dat").write_text("50 0.2371 0.05 1.0 30 1\n")
    (wrun, wbase), (rrun, rbase) = driver(writer), driver("py" if writer == "cli" else "cli")
    w = wrun(tmp_path, *wbase, *DRIVER_BC, *DRIVER_FLAGS, "--ntime", "12", "--checkpoint", "ck", "--output", "none")
    assert w.returncode == 0, w.stdout + w.stderr
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    assert meta["bc_x"] == "robin" and meta["bc_y"] == "robin" and meta["step"] == 12
    f32 = np.float32
    assert checkpoint.robin_from_meta(meta) == {k: (float(f32(a)), float(f32(b))) for k, (a, b) in PAIRS.items()}
    assert all(v.lstrip("-").startswith("0x") for pair in meta["robin"].values() for v in pair)
    for run, base in ((rrun, rbase), (wrun, wbase)):  # the contradiction fails in either driver
        bad = run(tmp_path, *base, "--restart", "ck", "--robin-x-lo", "0.5,0.37", "--output", "none")
        assert bad.returncode != 0 and "conflicts with the checkpoint" in bad.stdout + bad.stderr
        bad = run(tmp_path, *base, "--restart", "ck", "--bc-y", "insulated", "--output", "none")
        assert bad.returncode != 0 and "conflicts with the checkpoint" in bad.stdout + bad.stderr
    same = rrun(tmp_path, *rbase, "--restart", "ck", "--robin-x-lo", "0.8125,0.37", "--output", "none")
    assert same.returncode == 0, same.stdout + same.stderr
    r = rrun(tmp_path, *rbase, "--restart", "ck")
    assert r.returncode == 0, r.stdout + r.stderr
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    ref = R.owned(R.ftcs(prob, dtype=f32, bc_x="robin", bc_y="robin", robin=PAIRS))
    assert np.array_equal(io.read_xyz(str(tmp_path / "soln00000.dat"))[2].astype(f32), ref)
    assert not np.array_equal(ref, R.owned(R.ftcs(prob, dtype=f32, bc_x="insulated", bc_y="insulated")))


@pytest.mark.parametrize("which", ["cli", "py"])
def test_driver_flags(native, tmp_path, which):
    """Either driver: a missing side and a surplus side fail before the first step, |a| > 1 draws the stability
    warning, jacobi is refused, auto at r = 1/4 resolves to fma (never jacobi) and the run is the golden's."""
    import json

    from heat2d.utils import io
    (tmp_path / "input.dat").write_text("49 0.25 0.05 1.0 9 1\n")  # (r == 1/4 exactly at this n, on a Sterbenz-safe IC)
    run, base = driver(which)
    miss = run(tmp_path, *base, *DRIVER_BC, *DRIVER_FLAGS[:3], "--output", "none")
    assert miss.returncode != 0 and "y-hi" in (miss.stdout + miss.stderr).replace("_", "-")
    extra = run(tmp_path, *base, "--bc-x", "robin", *DRIVER_FLAGS, "--output", "none")
    assert extra.returncode != 0 and "y-lo" in (extra.stdout + extra.stderr).replace("_", "-")
    noisy = [f for f in base if f != "--quiet"]
    warn = run(tmp_path, *noisy, "--bc-x", "robin", "--robin-x-lo", "1.5,0", "--robin-x-hi", "1,0", "--output", "none")
    assert warn.returncode == 0 and "|a| > 1" in warn.stderr, warn.stdout + warn.stderr
    quiet = run(tmp_path, *noisy, *DRIVER_BC, *DRIVER_FLAGS, "--output", "none")
    assert quiet.returncode == 0 and "|a| > 1" not in quiet.stderr, quiet.stdout + quiet.stderr
    jac = run(tmp_path, *[("jacobi" if f == "exact" else f) for f in base], "--bc-x", "robin", "--robin-x-lo", "1,0",
              "--robin-x-hi", "1,0", "--output", "none")
    assert jac.returncode != 0 and "Robin" in jac.stdout + jac.stderr
    auto = run(tmp_path, *[("auto" if f == "exact" else f) for f in base], *DRIVER_BC, *DRIVER_FLAGS, "--json", "out.json")
    assert auto.returncode == 0, auto.stdout + auto.stderr
    rec = json.loads((tmp_path / "out.json").read_text())
    assert "jacobi" not in str(rec.get("arith_used", rec.get("arith")))
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    assert prob.r == 0.25 and prob.ic.sterbenz_safe()  # where a Dirichlet run's auto is jacobi
    ref = R.owned(R.ftcs(prob, dtype=np.float32, arith="fma", bc_x="robin", bc_y="robin", robin=PAIRS))
    assert np.array_equal(io.read_xyz(str(tmp_path / "soln00000.dat"))[2].astype(np.float32), ref)


# ------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("tb", [1, 4, 16, 24])
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", GPU_COMBOS, ids=GPU_IDS)
def test_hip_bitwise(native, gpu, bc_x, bc_y, dtype, arith, tb):
    """Two cycles of depth tb and the remainder (tb 24 = kMaxTBRob: 24, 24, 9), asserted from cycle_hist()."""
    assert N.max_tb_rob() == 24
    got = run(261, dtype, "hip", tb, bc_x, bc_y, steps=GSTEPS, arith=arith, prepare=True, calls=Y.calls(tb, GSTEPS, 2))
    assert np.array_equal(got, gold(261, dtype, bc_x, bc_y, steps=GSTEPS, arith=arith))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_single_call(native, gpu, dtype):
    """ONE step(57) call at tb 16: balanced cycles (15, 14, 14, 14) with Robin walls."""
    assert Y.balanced(16, GSTEPS) == [15, 14, 14, 14]
    got = run(261, dtype, "hip", 16, "robin", "robin", steps=GSTEPS, prepare=True)
    assert np.array_equal(got, gold(261, dtype, "robin", "robin", steps=GSTEPS))


@pytest.mark.gpu
@pytest.mark.parametrize("bc_x,bc_y", [("robin", "robin"), ("robin", "dirichlet")], ids=["xy", "x"])
def test_hip_loopback(native, gpu, bc_x, bc_y):
    """3 loopback ranks at n = 302 (101 / 101 / 100), Robin on both axes and on x only."""
    for dtype in ("fp64", "fp32"):
        got, slabs = run(302, dtype, "hip", 20, bc_x, bc_y, steps=GSTEPS, ranks=3, framed=True, calls=Y.calls(20, GSTEPS, 2))
        assert [m for _, m in slabs] == [101, 101, 100]
        assert np.array_equal(got, gold(302, dtype, bc_x, bc_y, steps=GSTEPS)), dtype


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_frame_images(native, gpu, dtype, arith):
    """download_field() on the GPU: the frame holds the ghost values after upload and after the march."""
    for bc_x, bc_y in GPU_COMBOS:
        rob = pairs_for(bc_x, bc_y)
        s = HeatSolver(problem(261, GSTEPS), dtype=dtype, backend="hip", tb=20, arith=arith, device=0, bc_x=bc_x, bc_y=bc_y,
                       robin=rob)
        T0 = rough_field(261, dtype)
        s.upload(T0)
        assert np.array_equal(s.download_field(), R.wrap_frame(T0, bc_x, bc_y, rob, arith)), (bc_x, bc_y)
        for m in Y.calls(20, GSTEPS, 2):
            s.step(m)
        got, hist = s.download_field(), s.cycle_hist()
        s.close()
        assert np.array_equal(got, gold(261, dtype, bc_x, bc_y, steps=GSTEPS, arith=arith, framed=True)), (bc_x, bc_y)
        Y.assert_ran(hist, 20, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_insulated_identity(native, gpu, dtype, arith):
    """tb_kernel_rob with (1, -0.0) against tb_kernel_ins, in bits, frame included."""
    kw = dict(steps=GSTEPS, arith=arith, prepare=True, calls=Y.calls(20, GSTEPS, 2), framed=True)
    a = run(261, dtype, "hip", 20, "robin", "robin", pairs=IDENT, **kw)
    b = run(261, dtype, "hip", 20, "insulated", "insulated", pairs=None, **kw)
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(graph=True), dict(autotune=1)], ids=["graph", "autotune"])
def test_hip_plan_variants(native, gpu, kw):
    got = run(261, "fp64", "hip", 8, "robin", "robin", steps=GSTEPS, prepare=True, **kw)
    assert np.array_equal(got, gold(261, "fp64", "robin", "robin", steps=GSTEPS))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n", [("fp64", 181), ("fp32", 213)])
def test_hip_narrow_last_strip(native, gpu, dtype, n):
    """Depth 20 with a last strip of 5 columns (fp64: 88 useful columns per strip, fp32: 208): narrower than
    the strip halo, so the strip before it reaches the wall column too."""
    got = run(n, dtype, "hip", 20, "robin", "robin", steps=GSTEPS, prepare=True, calls=Y.calls(20, GSTEPS, 2))
    assert np.array_equal(got, gold(n, dtype, "robin", "robin", steps=GSTEPS))


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_probes(native, gpu, dtype, arith):
    """Probes with Robin walls, one beside each corner; the last row equals download() at the probes."""
    n = 261
    pts = np.array([[1, 1], [1, 261], [261, 1], [261, 261], [1, 130], [130, 261], [100, 100], [2, 261]])
    s = HeatSolver(problem(n, GSTEPS), dtype=dtype, backend="hip", tb=20, arith=arith, device=0, bc_x="robin",
                   bc_y="robin", robin=PAIRS, probes=pts, probe_steps=GSTEPS)
    s.upload(rough_field(n, dtype))
    for m in Y.calls(20, GSTEPS, 2):
        s.step(m)
    H, out = s.probe_history(), s.download()
    s.close()
    want = R.probe_history(problem(n, GSTEPS), GSTEPS, pts, dtype=NP[dtype], T0=rough_field(n, dtype), arith=arith,
                           bc_x="robin", bc_y="robin", robin=PAIRS)
    assert np.array_equal(H, want)
    assert np.array_equal(H[-1], out[pts[:, 0] - 1, pts[:, 1] - 1])


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_raw_op(native, gpu, dtype, arith):
    """One tb_step launch with bc = 16 | 32 on a 70 x 261 window, and the probe cone, against the CPU raw ops."""
    import torch
    K, L, host = raw_window(dtype)
    f = torch.from_numpy(host)
    want = f.clone()
    kw = dict(arith=arith, bc_x="robin", bc_y="robin", robin=PAIRS)
    K.tb_step(f, want, L, 20, SIGMA, **kw)
    fd = f.cuda()
    gd = fd.clone()
    K.tb_step(fd, gd, L, 20, SIGMA, **kw)
    assert np.array_equal(gd.cpu().numpy(), want.numpy())  # owned points, ghost values, and nothing else written
    pts = np.array([[1, 1], [70, 261], [35, 1], [1, 100]])
    assert np.array_equal(K.probe_cone(fd, L, 20, SIGMA, pts, **kw).cpu().numpy(), K.probe_cone(f, L, 20, SIGMA, pts, **kw).numpy())


def worker(tmp_path, a, **env):
    import json
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(HERE, "robin_worker.py"), str(tmp_path), json.dumps(a)],
                         env=dict(os.environ, HEAT2D_PLAN_CACHE="off", **env), capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    return json.loads((tmp_path / "info.json").read_text()), np.load(tmp_path / "result.npy")


def gold_rect(n, rows, dtype, steps, arith="exact"):
    """The golden of a rows x n domain from source_worker's rough field (the worker's data)."""
    from source_worker import rough_field as rf
    return R.owned(R.ftcs(problem(n, steps), steps, dtype=NP[dtype], T0=rf(n, dtype, rows=rows), arith=arith, bc_x="robin",
                          bc_y="robin", robin=PAIRS))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_dynamic_queue_under_graph_replay(native, gpu, tmp_path, dtype):
    """301 rows x 2897 columns, HEAT2D_DYNAMIC=1 HEAT2D_MAX_WAVES=40, graph=True: the dynamic item queue (more
    items than waves) replayed from the captured pair graph, with the wall-column strips carved out of the
    interior launch onto tb_kernel_rob."""
    tb = 8
    # step(20): with the pair graph 8, 8 (one replay) and 4; eager balanced cycles would be 7, 7, 6
    a = {"n": 2897, "rows": 301, "steps": 4 * tb + 5, "tb": tb, "dtype": dtype, "arith": "exact", "graph": True,
         "bc_x": "robin", "bc_y": "robin", "calls": [20, 17]}
    info, got = worker(tmp_path, a, HEAT2D_DYNAMIC="1", HEAT2D_MAX_WAVES="40")
    plan = info["plan"]
    assert info["first_call_cycles"] == Y.balanced(tb, 20, graph=True) == [8, 8, 4] != Y.balanced(tb, 20), info
    Y.assert_ran(info["cycle_hist"], tb, 2)
    assert Y.hist_of(Y.depths(tb, [20, 17], graph=True)) == {int(k): v for k, v in info["cycle_hist"].items()}, info
    print(f"{dtype}: plan {plan}")
    assert plan["dynamic"] == 1 and plan["main_waves"] == 40 and plan["main_items"] > plan["main_waves"]
    assert plan["pipe"] == 0 and (info["info"]["bc_x"], info["info"]["bc_y"]) == ("robin", "robin")
    assert np.array_equal(got, gold_rect(2897, 301, dtype, 4 * tb + 5))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["edge-first", "concurrent", "single"])
def test_hip_split_orders_and_single_launch(native, gpu, tmp_path, order):
    """The two split orders and a single-launch plan, from a fresh process each."""
    a = {"n": 261, "steps": GSTEPS, "tb": 8, "dtype": "fp64", "arith": "exact", "bc_x": "robin", "bc_y": "robin"}
    info, got = worker(tmp_path, a, HEAT2D_SPLIT_ORDER=order, **({"HEAT2D_BANDS": "3"} if order == "single" else {}))
    print(f"split order {order}: plan {info['plan']}")
    assert info["plan"]["order"] == order
    from source_worker import rough_field as rf
    want = R.owned(R.ftcs(problem(261, GSTEPS), GSTEPS, T0=rf(261, "fp64"), bc_x="robin", bc_y="robin", robin=PAIRS))
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_hip_forced_pipe_falls_back(native, gpu, tmp_path):
    """HEAT2D_PIPE=1 under Robin y: the wave-pair kernel is not offered, as under insulated y."""
    a = {"n": 700, "steps": GSTEPS, "tb": 20, "dtype": "fp64", "arith": "exact", "bc_x": "robin", "bc_y": "robin"}
    info, got = worker(tmp_path, a, HEAT2D_PIPE="1")
    assert info["plan"]["pipe"] == 0, info["plan"]
    from source_worker import rough_field as rf
    want = R.owned(R.ftcs(problem(700, GSTEPS), GSTEPS, T0=rf(700, "fp64"), bc_x="robin", bc_y="robin", robin=PAIRS))
    assert np.array_equal(got, want)
