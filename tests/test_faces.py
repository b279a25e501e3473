"""Conservative heat conduction, u_t = div(k grad u), from per-face diffusion
numbers (RX, RY): RX[i,j] the face between (i,j) and (i,j+1), RY[i,j] the face
between (i,j) and (i+1,j), already multiplied by dt / dx^2,

    exact: T' = C + (((RY[i,j]*(S-C) + RX[i,j]*(E-C)) + RY[i-1,j]*(N-C)) + RX[i,j-1]*(W-C))
    fma:   p = RY[i,j]*(S-C); p = fma(RX[i,j], E-C, p); p = fma(RY[i-1,j], N-C, p);
           p = fma(RX[i,j-1], W-C, p); T' = C + p

bitwise against the NumPy golden (models.reference.ftcs(faces=)) at every pass
depth, launch plan and rank count, on the CPU twin and on the HIP engine
(tb_kernel_div, csrc/kernels/tb_impl.hpp).

Data (fixed seeds, tests/faces_worker.py): field values 10**uniform(-1, 1),
frame included; cells of two materials 100 : 1, each times uniform(0.5, 1);
faces 0.25 times the harmonic mean of their two cells (face sum <= 1), 3 % of
them exactly 0, a block of cells with all four faces 0; NaN in every entry no
point uses (the engine must ignore them).

Negative controls of the data come first: only an engine that multiplies the
right difference by the right face, in the right order and form, can pass the
bitwise tests.
"""
import hashlib
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import heat2d
from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver, LoopbackGroup, faces_sum_max
from heat2d.ops import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cycles as Y  # noqa: E402
from faces_worker import BLOCK, face_sum, problem, rough_faces, rough_field, signed_field, two_materials  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
_DEPTH = []


def depth_max():
    """The conservative-form kernels' deepest pass (common.hpp kMaxTBDiv), as the library
    reports it (tests/test_faces_isa.py holds it against the instances in the code objects)."""
    if not _DEPTH:
        s = HeatSolver(problem(8, 1), backend="cpu", faces=(np.full((10, 10), 0.1), np.full((10, 10), 0.1)))
        _DEPTH.append(s.info()["faces"]["max_tb"])
        s.close()
    return _DEPTH[0]


_GOLD = {}


def gold(n, dtype, steps, arith="exact", rows=None, seed=1, framed=False, closed=False):
    """The golden run (computed once, read-only). rows: the first rows x n of the grid."""
    key = (n, dtype, steps, arith, rows, seed, closed)
    if key not in _GOLD:
        T0, F = rough_field(n, dtype, rows=rows), rough_faces(n, dtype, rows=rows, seed=seed, closed=closed)
        g = np.ascontiguousarray(R.ftcs(problem(n, steps), steps, dtype=NP[dtype], T0=T0, arith=arith, faces=F))
        g.setflags(write=False)
        _GOLD[key] = g
    return _GOLD[key] if framed else R.owned(_GOLD[key])


def run(n, dtype, backend, tb, steps, arith="exact", ranks=1, rows=None, prepare=False, full=0, closed=False, sizes=None,
        **kw):
    """full > 0: the steps as tests/cycles.py calls(tb, steps, full) — `full` cycles of depth
    tb, asserted from cycle_hist(), then the remainder. sizes: explicit step() calls."""
    p = problem(n, steps)
    T0, F = rough_field(n, dtype, rows=rows), rough_faces(n, dtype, rows=rows, closed=closed)
    dev = dict(device=0) if backend == "hip" else {}
    sizes = sizes or (Y.calls(tb, steps, full) if full else [steps])
    assert sum(sizes) == steps
    if ranks > 1:
        s = LoopbackGroup(p, ranks, dtype=dtype, backend=backend, tb=tb, arith=arith, faces=F, **dev, **kw)
        s.upload(T0)
        for m in sizes:
            s.step(m)
        out = s.download()
        s.close()
        return out
    s = HeatSolver(p, dtype=dtype, backend=backend, tb=tb, arith=arith, faces=F, rows=rows, **dev, **kw)
    s.upload(T0)
    for m in sizes:
        if prepare:
            s.prepare(m)
        s.step(m)
    out, hist = s.download(), s.cycle_hist()
    s.close()
    if full:
        Y.assert_ran(hist, tb, full)
    return out


# ------------------------------------------------------------------ CPU: the golden and its data

def closed_setup(n, dtype):
    """The closed domain: rough signed data (tests/faces_worker.py signed_field), two materials,
    every face to the frame 0."""
    T0 = signed_field(n, dtype)
    RX, RY = rough_faces(n, dtype, closed=True)
    assert (RX[1:-1, 0] == 0).all() and (RX[1:-1, -2] == 0).all() and (RY[0, 1:-1] == 0).all() and (RY[-2, 1:-1] == 0).all()
    return T0, (RX, RY)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_conserves_heat(dtype):
    """n = 77, 200 steps, closed domain: |fsum(T_n) - fsum(T_0)| over the owned points is at most
    4 eps n^2 steps max|T0| (four roundings per point and step on values the maximum principle
    keeps below 2 max|T0|; the face products themselves cancel exactly between the two cells of
    a face); and a block of points whose four faces are zero keeps its bits.
    Measured: heat -335.612; drift 1.1e-13 (fp64, bound 1.05e-08); fp32 far below its bound 5.65
    (printed)."""
    n, steps, dt = 77, 200, NP[dtype]
    T0, F = closed_setup(n, dtype)
    p = problem(n, steps)
    assert face_sum(*F).max() <= 1.0
    bound = 4 * float(np.finfo(dt).eps) * n * n * steps * float(np.abs(T0).max())
    h0 = math.fsum(R.owned(T0).astype(np.float64).ravel())
    for arith in ("exact", "fma"):
        g = R.ftcs(p, steps, dtype=dt, T0=T0, arith=arith, faces=F)
        drift = abs(math.fsum(R.owned(g).astype(np.float64).ravel()) - h0)
        print(f"{dtype} {arith}: heat {h0:.6g}, drift {drift:.3g}, bound {bound:.3g}")
        assert drift <= bound, (drift, bound)
        assert np.abs(g).max() <= np.abs(T0).max()
        assert np.array_equal(g[BLOCK].view(np.uint8), T0[BLOCK].view(np.uint8))
        assert np.array_equal(g[0], T0[0]) and np.array_equal(g[:, -1], T0[:, -1])


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_rmap_form_drifts_on_the_same_data(dtype):
    """The control of the conservation test: the rmap= golden at r = 0.25 k on the same closed
    domain drifts by more than 1000 times the bound above, so the test tells the two forms apart.
    In fp32 the bound is 5.65, so the control asks for a drift above 5654, 9.5 % of max|T0| per
    point: the data must be such that the map form's defect shows, and tests/faces_worker.py
    signed_field() says why its signs follow the material (with signs independent of the material
    the defect averages out: drift 32.8 of a total heat 388). Measured: the rmap= form drifts by
    11912.7 (total heat -335.6) in both dtypes."""
    n, steps, dt = 77, 200, NP[dtype]
    T0, F = closed_setup(n, dtype)
    p = problem(n, steps)
    bound = 4 * float(np.finfo(dt).eps) * n * n * steps * float(np.abs(T0).max())
    h0 = math.fsum(R.owned(T0).astype(np.float64).ravel())
    M = (0.25 * two_materials(n)).astype(dt)
    gm = R.ftcs(p, steps, dtype=dt, T0=T0, arith="exact", rmap=M)
    drift_map = abs(math.fsum(R.owned(gm).astype(np.float64).ravel()) - h0)
    print(f"{dtype}: the rmap= form drifts by {drift_map:.6g}")
    assert drift_map > 1000 * bound, (drift_map, bound)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_negative_controls(dtype):
    """n = 77, 8 steps, default_rng(5) data: wrong faces, the other forms and the other order,
    each against the golden."""
    n, K, dt = 77, 8, NP[dtype]
    rng = np.random.default_rng(5)
    p = problem(n, K)
    T0 = (10.0 ** rng.uniform(-1, 1, (n + 2, n + 2))).astype(dt)
    k = rng.choice([1.0, 0.01], T0.shape) * rng.uniform(0.5, 1.0, T0.shape)
    RX = np.zeros(T0.shape)
    RY = np.zeros(T0.shape)
    RX[:, :-1] = 0.25 * 2 * k[:, :-1] * k[:, 1:] / (k[:, :-1] + k[:, 1:])
    RY[:-1, :] = 0.25 * 2 * k[:-1, :] * k[1:, :] / (k[:-1, :] + k[1:, :])
    RX, RY = RX.astype(dt), RY.astype(dt)
    g = R.owned(R.ftcs(p, K, dtype=dt, T0=T0, faces=(RX, RY)))

    def differs(other):
        return float(np.mean(R.owned(other) != g))

    def with_faces(fx, fy, arith="exact"):
        return R.ftcs(p, K, dtype=dt, T0=T0, arith=arith, faces=(np.ascontiguousarray(fx), np.ascontiguousarray(fy)))

    def flux_difference_order():
        T = T0.copy()
        for _ in range(K):
            c = T[1:-1, 1:-1]
            S, E, Nn, W = T[2:, 1:-1], T[1:-1, 2:], T[:-2, 1:-1], T[1:-1, :-2]
            ys, xe, yn, xw = RY[1:-1, 1:-1], RX[1:-1, 1:-1], RY[:-2, 1:-1], RX[1:-1, :-2]
            Q = T.copy()
            Q[1:-1, 1:-1] = c + ((xe * (E - c) - xw * (c - W)) + (ys * (S - c) - yn * (c - Nn)))
            T = Q
        return T

    d = {"RX rolled by one column": (differs(with_faces(np.roll(RX, 1, axis=1), RY)), 0.99),
         "RY rolled by one row": (differs(with_faces(RX, np.roll(RY, 1, axis=0))), 0.99),
         "RX and RY swapped": (differs(with_faces(RY, RX)), 0.99),
         "both transposed": (differs(with_faces(RX.T, RY.T)), 0.99),
         "the rmap= form": (differs(R.ftcs(p, K, dtype=dt, T0=T0, rmap=(0.25 * k).astype(dt))), 0.99),
         "the flux-difference order": (differs(flux_difference_order()), 0.10),
         "fma against exact": (differs(with_faces(RX, RY, "fma")), 0.10)}
    for name, (v, _) in d.items():
        print(f"{dtype}: {name}: differs at {100 * v:.1f} % of the owned points")
    for name, (v, least) in d.items():
        assert v > least, (name, v)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_defaults_and_constant_faces(dtype):
    """faces=None is today's function, bit for bit. Constant faces RX = RY = 0.2 are the scalar
    r = 0.2 run in exact arithmetic only: the two forms round differently, so their bits differ
    (measured: at 67 % of the points) while the values agree within a few ulp."""
    n, dt = 77, NP[dtype]
    p, T0 = problem(n, 8), rough_field(n, dtype)
    assert np.array_equal(R.ftcs(p, 8, dtype=dt, T0=T0, faces=None), R.ftcs(p, 8, dtype=dt, T0=T0))
    assert np.array_equal(R.ftcs_step(T0, p.r, faces=None), R.ftcs_step(T0, p.r))
    c = np.full(T0.shape, 0.2)
    a = R.owned(R.ftcs(p, 1, dtype=dt, T0=T0, faces=(c, c)))
    b = R.owned(R.ftcs(p, 1, dtype=dt, T0=T0))
    frac = float(np.mean(a != b))
    print(f"{dtype}: constant faces differ in bits from the scalar r at {100 * frac:.1f} % of the points")
    assert frac > 0  # they differ in bits: no equality is claimed
    assert np.abs(a.astype(np.float64) - b).max() <= 16 * float(np.finfo(dt).eps) * float(np.abs(T0).max())


def test_golden_refusals():
    p, T0 = problem(40, 2), rough_field(40, "fp64")
    F = rough_faces(40, "fp64")
    for kw, why in ((dict(rmap=np.zeros_like(T0)), "rmap"), (dict(source=np.zeros_like(T0)), "source"),
                    (dict(bc_x="periodic"), "Dirichlet"), (dict(bc_y="insulated"), "Dirichlet"),
                    (dict(arith="jacobi"), "exact")):
        with pytest.raises(ValueError, match=why):
            R.ftcs(p, 2, T0=T0, faces=F, **kw)
    with pytest.raises(ValueError, match="frame-inclusive"):
        R.ftcs(p, 2, T0=T0, faces=(F[0][1:], F[1]))


# ------------------------------------------------------------------ CPU twin

@pytest.mark.parametrize("tb", [1, 2, 7, 8])
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_twin_bitwise(native, dtype, arith, tb):
    for n, steps in ((77, 8), (301, 11)):
        got = run(n, dtype, "cpu", tb, steps, arith)
        assert np.array_equal(got, gold(n, dtype, steps, arith)), n


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_loopback_uneven_slabs(native, dtype):
    """3 ranks on 77 rows (26 / 26 / 25): RY[i-1] of a slab's first row is the row above the seam."""
    for arith in ("exact", "fma"):
        got = run(77, dtype, "cpu", 7, 23, arith, ranks=3)
        assert np.array_equal(got, gold(77, dtype, 23, arith)), arith


def test_cpu_gloo_ranks(native, tmp_path):
    """3 gloo ranks on 77 rows, the CPU twin behind the torch.distributed transport: every rank
    slices its rows of the global arrays, the row above each seam included."""
    a = {"n": 77, "steps": 23, "tb": 7, "dtype": "fp64", "arith": "exact"}
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2", MASTER_ADDR="127.0.0.1", HEAT2D_COMM_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "faces_worker.py"), "gloo", str(r), "3", str(port),
                               str(tmp_path), json.dumps(a)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(3)]
    try:
        outs = [p.communicate(timeout=240)[0].decode(errors="replace") for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    p = problem(77, 23)
    T0 = R.initial_field(p)  # (the ranks upload owned points; the frame is the problem's)
    T0[1:-1, 1:-1] = R.owned(rough_field(77, "fp64"))
    assert np.array_equal(np.load(tmp_path / "result.npy"), R.owned(R.ftcs(p, 23, T0=T0, faces=rough_faces(77, "fp64"))))


def test_refusals(native):
    p, F = problem(40, 4, 0.25), rough_faces(40, "fp64")
    Z = np.zeros((42, 42))
    for kw, why in ((dict(arith="jacobi"), "jacobi"), (dict(arith="fast"), "fast"), (dict(bc_x="periodic"), "Dirichlet"),
                    (dict(bc_y="periodic"), "Dirichlet"), (dict(bc_x="insulated"), "Dirichlet"),
                    (dict(bc_y="insulated"), "Dirichlet"), (dict(copy_swap=True), "copy-swap"),
                    (dict(source=Z), "heat source"), (dict(rmap=Z + 0.1), "diffusivity map")):
        with pytest.raises(RuntimeError, match=why):
            HeatSolver(p, backend="cpu", faces=F, **kw)
    with pytest.raises(RuntimeError, match="jit|HIP"):
        HeatSolver(p, backend="cpu", engine="jit", faces=F)
    with pytest.raises(ValueError, match="frame-inclusive"):
        HeatSolver(p, backend="cpu", faces=(F[0][1:], F[1]))
    with pytest.raises(ValueError, match="pair"):
        HeatSolver(p, backend="cpu", faces=F[0])
    for bad in (-0.01, np.nan, np.inf):
        for w, at in ((0, (7, 9)), (0, (7, 0)), (1, (0, 9)), (1, (40, 9))):  # used faces, the frame-adjacent ones too
            Fb = [F[0].copy(), F[1].copy()]
            Fb[w][at] = bad
            with pytest.raises(ValueError, match="finite and >= 0"):
                HeatSolver(p, backend="cpu", faces=tuple(Fb))
    assert np.isnan(F[0][:, -1]).all() and np.isnan(F[1][-1]).all()  # unused entries are ignored, whatever they hold
    s = HeatSolver(p, backend="cpu")  # built without faces: none can be set later
    with pytest.raises(RuntimeError, match="without face coefficients"):
        s.set_faces(F)
    s.set_faces(None)
    s.close()


def test_auto_resolves_to_exact_and_info(native):
    inp = heat2d.parse_input_text("64 0.25 0.05 1.0 6 0")
    p = heat2d.make_problem(inp, "ghost", "uniform")
    F = rough_faces(p.n_owned, "fp64")
    s = HeatSolver(p, backend="cpu", arith="auto", tb=24, faces=F)
    info = s.info()
    s.step(6)
    got = s.download()
    s.close()
    assert info["arith"] == N.ARITH["exact"] and s.arith == "exact"
    assert info["faces"] == {"enabled": True, "set": True, "max_tb": depth_max()} and 8 <= depth_max() == info["tb"]
    assert np.array_equal(got, R.owned(R.ftcs(p, 6, arith="exact", faces=F)))
    g = LoopbackGroup(p, 2, backend="cpu", arith="auto", faces=F)
    assert g.arith_code(0) == N.ARITH["exact"] and g.arith_code(1) == N.ARITH["exact"]
    g.close()
    s = HeatSolver(p, backend="cpu")
    assert s.info()["faces"] == {"enabled": False, "set": False, "max_tb": 0}
    s.close()


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_set_faces_none_and_fresh(native, dtype):
    """set_faces(None): the run equals the scalar-r run; fresh faces between two step() calls:
    the golden run the same way."""
    n, dt, p = 77, NP[dtype], problem(77, 20)
    T0, F1, F2 = rough_field(n, dtype), rough_faces(n, dtype), rough_faces(n, dtype, seed=2)
    s = HeatSolver(p, dtype=dtype, backend="cpu", tb=7, arith="exact", faces=F1)
    s.set_faces(None)
    assert s.info()["faces"]["set"] is False and s.faces_sha256 is None
    s.upload(T0)
    s.step(20)
    assert np.array_equal(s.download(), R.owned(R.ftcs(p, 20, dtype=dt, T0=T0)))
    s.upload(T0)
    s.set_faces(F1)
    s.step(9)
    s.set_faces(F2)
    s.step(11)
    got = s.download()
    s.close()
    mid = R.ftcs(p, 9, dtype=dt, T0=T0, faces=F1)
    assert np.array_equal(got, R.owned(R.ftcs(p, 11, dtype=dt, T0=mid, faces=F2)))


def test_step_stats_takes_the_unfused_path(native):
    p, F = problem(77, 12), rough_faces(77, "fp64")
    s = HeatSolver(p, backend="cpu", tb=5, arith="exact", faces=F)
    s.upload(rough_field(77, "fp64"))
    st = s.step_stats(12)
    got = s.download()
    s.close()
    g = gold(77, "fp64", 12).astype(np.float64)
    assert np.array_equal(got, g) and st["min"] == g.min() and st["max"] == g.max()


def test_raw_op_cpu(native):
    """tb_step(faces=) on a middle slab: rows 40..110 of a 150-row grid, 8 fused levels = 8 golden steps."""
    _raw_op("cpu", "fp64", 8)


def _raw_op(device, dtype, k, n=150, ncols=261, row0=40, nrows=70, arith="exact"):
    """Against the golden and against heat2d_cpu_tb_div on the same buffers."""
    import torch

    from heat2d.ops import kernels as K
    dt = NP[dtype]
    rng = np.random.default_rng(7)
    T0 = (10.0 ** rng.uniform(-1, 1, (n + 2, ncols + 2))).astype(dt)
    RX = rng.uniform(0.0025, 0.25, T0.shape)
    RY = rng.uniform(0.0025, 0.25, T0.shape)
    RX[rng.uniform(size=T0.shape) < 0.03] = 0.0
    RY[rng.uniform(size=T0.shape) < 0.03] = 0.0
    RX, RY = RX.astype(dt), RY.astype(dt)
    L = K.make_layout(nrows, ncols, halo=24, row0=row0, nrows_global=n)
    host = np.full((L.rows_alloc(), L.pitch), 3.25, dtype=dt)  # (pad columns: finite, pinned)
    g0 = row0 - L.halo
    host[:, L.cpad - 1:L.cpad + ncols + 1] = T0[g0 + 1:g0 + 1 + L.rows_alloc()]
    src = torch.from_numpy(host.reshape(-1).copy()).to(device)
    dst = torch.full_like(src, float("nan"))  # NaN guard bands around the rows written
    K.tb_step(src, dst, L, k, 0.0, arith=arith, faces=K.faces_field(RX, RY, L, src.dtype, device))
    out = K.view2d(dst.cpu(), L).numpy().copy()
    T = T0.copy()
    for _ in range(k):
        T = R.ftcs_step(T, 0.0, arith, faces=(RX, RY))
    own = out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols].copy()
    assert np.array_equal(own, T[row0 + 1:row0 + 1 + nrows, 1:-1])
    if device != "cpu":  # the CPU twin's raw op (heat2d_cpu_tb_div) on the same buffers
        csrc, cdst = src.cpu(), torch.full_like(src, float("nan")).cpu()
        K.tb_step(csrc, cdst, L, k, 0.0, arith=arith, faces=K.faces_field(RX, RY, L, csrc.dtype, "cpu"))
        twin = K.view2d(cdst, L).numpy()[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols]
        assert np.array_equal(own, twin)
    # The only writes allowed outside the output rectangle (as tests/test_ops.py run_guard): the
    # device kernel's last 16-B vector of a row may cover the right frame column / pad of the
    # SAME rows, written back with src's pinned values.
    out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols] = np.nan
    rr, cc = np.nonzero(~np.isnan(out))
    assert ((rr >= L.halo) & (rr < L.halo + nrows)).all(), "kernel wrote outside its output rows"
    assert (cc >= L.cpad + ncols).all() and (cc < L.cpad + ncols + 8).all(), "kernel wrote beyond one vector of right pad"
    assert np.array_equal(out[rr, cc], host[rr, cc]), "frame / pad write changed a value"
    return own


def test_memory_planner_counts_both_buffers(native):
    for dtype, es in (("fp32", 4), ("fp64", 8)):
        for nranks in (1, 3):
            a = heat2d.footprint(1000, nranks, dtype)
            b = heat2d.footprint(1000, nranks, dtype, faces=True)
            one = a["field_bytes"] // 2
            assert a["field_bytes"] == 2 * one and b["field_bytes"] == 4 * one
            assert b["total_bytes"] - a["total_bytes"] == 2 * one and b["work_bytes"] == a["work_bytes"]
            rows = N.decompose(1000, nranks, 0)[1]
            L = N.make_layout(rows, 1000, 24, 0, 1000)
            assert one == L.elems() * es
    budget = 8 << 30
    with_faces = heat2d.plan_max_grid("fp64", 1, free_bytes=budget, reserve=0, faces=True)["n"]
    with_map = heat2d.plan_max_grid("fp64", 1, free_bytes=budget, reserve=0, rmap=True)["n"]
    assert with_faces < with_map < heat2d.plan_max_grid("fp64", 1, free_bytes=budget, reserve=0)["n"]
    assert heat2d.footprint(with_faces, 1, "fp64", faces=True)["total_bytes"] <= budget
    assert heat2d.footprint(with_faces + 1, 1, "fp64", faces=True)["total_bytes"] > budget


def test_faces_from_k():
    p = problem(12, 1)
    m = 14
    rng = np.random.default_rng(3)
    k = rng.uniform(0.1, 2.0, (m, m)).astype(np.float32)
    k[rng.uniform(size=(m, m)) < 0.2] = 0.0  # insulating cells
    scale = np.float64(p.r) / np.float64(p.nu)
    for mean in ("harmonic", "arithmetic"):
        RX, RY = heat2d.faces_from_k(p, k, mean=mean) if mean != "harmonic" else heat2d.faces_from_k(p, k)
        assert RX.dtype == RY.dtype == np.float64 and RX.shape == RY.shape == (m, m)
        for i in range(m):
            for j in range(m):
                for A, (i2, j2) in ((RX, (i, j + 1)), (RY, (i + 1, j))):
                    if i2 >= m or j2 >= m:
                        want = 0.0
                    else:
                        a, b = float(k[i, j]), float(k[i2, j2])
                        if a == 0.0 or b == 0.0:
                            want = 0.0
                        else:
                            want = float(scale * (2.0 * a * b / (a + b) if mean == "harmonic" else 0.5 * (a + b)))
                    assert A[i, j] == want, (mean, i, j)
    assert (heat2d.faces_from_k(p, k)[0][:, :-1][(k[:, :-1] == 0) | (k[:, 1:] == 0)] == 0).all()
    with pytest.raises(ValueError, match="mean"):
        heat2d.faces_from_k(p, k, mean="geometric")
    with pytest.raises(ValueError, match="frame-inclusive"):
        heat2d.faces_from_k(p, k[1:])
    # a uniform k gives the scalar r on every face
    RX, RY = heat2d.faces_from_k(p, np.full((m, m), p.nu))
    assert np.allclose(RX[:, :-1], p.r, rtol=1e-15, atol=0) and np.allclose(RY[:-1], p.r, rtol=1e-15, atol=0)
    assert faces_sum_max(RX, RY) == pytest.approx(4 * p.r)


# ------------------------------------------------------------------ CPU: checkpoints and the drivers

def test_checkpoint_faces_sha256(native, tmp_path):
    """Written; a restart without faces, with other faces, and of a checkpoint without the key, fail."""
    from heat2d.utils import checkpoint
    n, p = 77, problem(77, 20)
    F = rough_faces(n, "fp64")
    T0 = R.initial_field(p)  # (a checkpoint holds the owned points; the frame is the problem's)
    T0[1:-1, 1:-1] = R.owned(rough_field(n, "fp64"))
    s = HeatSolver(p, backend="cpu", tb=4, arith="exact", faces=F)
    s.upload(T0)
    s.step(9)
    checkpoint.save(s, str(tmp_path / "ck"), step=9)
    sha = s.faces_sha256
    s.close()
    sd = checkpoint.resolve(str(tmp_path / "ck"))
    meta = json.loads(open(os.path.join(sd, "meta.json")).read())
    assert meta["faces_sha256"] == sha == hashlib.sha256(F[0].tobytes() + F[1].tobytes()).hexdigest()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", faces=F)
    assert checkpoint.load(r, sd)["step"] == 9
    r.step(11)
    assert np.array_equal(r.download(), R.owned(R.ftcs(p, 20, T0=T0, faces=F)))
    r.close()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact")
    with pytest.raises(ValueError, match="with face coefficients"):
        checkpoint.load(r, sd)
    checkpoint.save(r, str(tmp_path / "ck0"), step=0)
    assert "faces_sha256" not in json.loads(open(os.path.join(checkpoint.resolve(str(tmp_path / "ck0")), "meta.json")).read())
    r.close()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", faces=rough_faces(n, "fp64", seed=2))
    with pytest.raises(ValueError, match="differ from the checkpoint"):
        checkpoint.load(r, sd)
    with pytest.raises(ValueError, match="without face coefficients"):
        checkpoint.load(r, checkpoint.resolve(str(tmp_path / "ck0")))
    r.close()


def py(cwd, *args):
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2")
    return subprocess.run([sys.executable, "-m", "heat2d", *args], cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=300)


def test_drivers_faces(native, tmp_path):
    """--faces through both drivers on the CPU backend: the golden's field (auto is exact), the
    checkpoint's digest, py <-> cli restarts, the restarts that must fail, a wrong shape, and the
    face-sum warning."""
    from heat2d.utils import io
    n = 64
    (tmp_path / "input.dat").write_text(f"{n} 0.25 0.05 1.0 30 1\n")
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "uniform")
    F = rough_faces(n, "fp64")
    np.save(tmp_path / "faces.npy", np.stack(F))
    np.save(tmp_path / "other.npy", np.stack(rough_faces(n, "fp64", seed=2)))
    np.save(tmp_path / "bad.npy", np.stack(F)[:, :, 1:])
    np.save(tmp_path / "flat.npy", F[0])
    sha = hashlib.sha256(np.stack(F).tobytes()).hexdigest()
    gold30 = R.owned(R.ftcs(prob, 30, arith="exact", faces=F))
    cli = [N.CLI_PATH, "--cpu", "--quiet", "--ic", "uniform"]
    pyargs = ["--backend", "cpu", "--ic", "uniform", "--quiet", "--output", "npy"]

    def run_cli(*args):
        return subprocess.run([*cli, *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)

    def meta_of(d):
        with open(tmp_path / d / "latest") as f:
            return json.loads((tmp_path / d / f.read().strip() / "meta.json").read_text())

    # the native CLI writes, both drivers resume
    out = run_cli("--faces", "faces.npy", "--ntime", "12", "--checkpoint", "ckc", "--output", "none", "--json", "w.json")
    assert out.returncode == 0, out.stdout + out.stderr
    assert "unstable" not in out.stderr
    assert json.loads((tmp_path / "w.json").read_text())["arith_used"] == "exact (auto)"
    assert meta_of("ckc")["faces_sha256"] == sha and meta_of("ckc")["step"] == 12
    out = run_cli("--restart", "ckc", "--faces", "faces.npy", "--gpus", "3", "--output", "npy")
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.concatenate([np.load(tmp_path / f"soln{r:05d}.npy") for r in range(3)], axis=0), gold30)
    out = py(tmp_path, *pyargs, "--faces", "faces.npy", "--restart", "ckc")
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.load(tmp_path / "soln00000.npy"), gold30)
    # the Python driver writes, the native CLI resumes
    out = py(tmp_path, *pyargs, "--faces", "faces.npy", "--ntime", "12", "--checkpoint", "ckp")
    assert out.returncode == 0, out.stdout + out.stderr
    assert meta_of("ckp")["faces_sha256"] == sha
    out = run_cli("--restart", "ckp", "--faces", "faces.npy")
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(io.read_xyz(str(tmp_path / "soln00000.dat"))[2], gold30)
    # restarts that fail before the first step, whichever driver wrote the checkpoint
    for ck in ("ckc", "ckp"):
        bad = run_cli("--restart", ck)
        assert bad.returncode != 0 and "face coefficients" in bad.stdout + bad.stderr
        bad = run_cli("--restart", ck, "--faces", "other.npy")
        assert bad.returncode != 0 and "differ from the checkpoint" in bad.stdout + bad.stderr
        bad = py(tmp_path, *pyargs, "--restart", ck)
        assert bad.returncode != 0 and "face coefficients" in bad.stdout + bad.stderr
        bad = py(tmp_path, *pyargs, "--restart", ck, "--faces", "other.npy")
        assert bad.returncode != 0 and "differ from the checkpoint" in bad.stdout + bad.stderr
    for f in ("bad.npy", "flat.npy"):
        bad = run_cli("--faces", f)
        assert bad.returncode != 0 and "shape" in bad.stdout + bad.stderr
        bad = py(tmp_path, *pyargs, "--faces", f)
        assert bad.returncode != 0 and "shape" in bad.stdout + bad.stderr
    # an f8 file in an fp32 run: converted, and the digest is the converted arrays'
    out = run_cli("--dtype", "fp32", "--faces", "faces.npy", "--ntime", "5", "--checkpoint", "ck32", "--output", "none")
    assert out.returncode == 0, out.stdout + out.stderr
    assert meta_of("ck32")["faces_sha256"] == hashlib.sha256(np.stack(F).astype(np.float32).tobytes()).hexdigest()
    # without faces meta.json has no such key
    out = run_cli("--ntime", "3", "--checkpoint", "ck0", "--output", "none")
    assert out.returncode == 0 and "faces_sha256" not in meta_of("ck0")
    # the stability warning: the largest face sum of an owned point above 1
    hot = np.stack(F)
    hot[0, 5, 5] = 0.9
    np.save(tmp_path / "hot.npy", hot)
    want = f"max face sum = {faces_sum_max(hot[0], hot[1]):.6g} > 1"
    for out in (run_cli("--faces", "hot.npy", "--ntime", "2", "--output", "none"),
                py(tmp_path, *pyargs, "--faces", "hot.npy", "--ntime", "2")):
        assert out.returncode == 0 and want in out.stderr, out.stdout + out.stderr


# ------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_loopback_three_ranks(native, gpu, dtype):
    """n = 302 on 3 loopback ranks, uneven slabs (101 / 101 / 100): depth D, then a deeper and a
    shallower cycle (step(D), step(D + 5): depths D, then balanced 11 and 10 at D = 16)."""
    D = depth_max()
    p = problem(302, 2 * D + 5)
    for arith in ("exact", "fma"):
        g = LoopbackGroup(p, 3, dtype=dtype, backend="hip", tb=D, arith=arith, device=0, faces=rough_faces(302, dtype))
        assert [r for _, r in g.slabs()] == [101, 101, 100]
        g.upload(rough_field(302, dtype))
        g.step(D)
        g.step(D + 5)
        got = g.download()
        hist = g.cycle_hist(0)
        g.close()
        Y.assert_ran(hist, D, 1)  # depth D ran, and shallower cycles after it
        for k in Y.depths(D, [D, D + 5]):  # (D = 16: 16, then 11 and 10)
            Y.assert_ran(hist, k)
        assert np.array_equal(got, gold(302, dtype, 2 * D + 5, arith)), arith


def worker(tmp_path, a, **env):
    out = subprocess.run([sys.executable, os.path.join(HERE, "faces_worker.py"), str(tmp_path), json.dumps(a)],
                         env=dict(os.environ, HEAT2D_PLAN_CACHE="off", **env), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    return json.loads((tmp_path / "info.json").read_text()), np.load(tmp_path / "result.npy")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_dynamic_queue_under_graph_replay(native, gpu, tmp_path, dtype):
    """301 rows x 2897 columns, HEAT2D_MAX_WAVES small, graph=True: the dynamic item queue (more
    items than waves) replayed from the captured pair graph, every launch on tb_kernel_div."""
    tb = 8
    a = {"n": 2897, "rows": 301, "steps": 4 * tb + 5, "tb": tb, "dtype": dtype, "sigma": 0.2, "arith": "exact", "graph": True,
         "calls": [2 * tb, 2 * tb, 5]}  # two replays of the pair graph, then a shallower cycle
    info, got = worker(tmp_path, a, HEAT2D_DYNAMIC="1", HEAT2D_MAX_WAVES="40")
    plan = info["plan"]
    Y.assert_ran(info["cycle_hist"], tb, 4)
    print(f"{dtype}: plan {plan}")
    assert plan["dynamic"] == 1 and plan["main_waves"] == 40 and plan["main_items"] > plan["main_waves"]
    assert plan["pipe"] == 0 and plan["main_strip_w"] == (128 if dtype == "fp64" else 256)
    assert info["info"]["tb"] == tb and info["info"]["faces"]["set"] and info["info"]["arith"] == N.ARITH["exact"]
    assert np.array_equal(got, gold(2897, dtype, 4 * tb + 5, "exact", rows=301))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_set_faces_between_steps(native, gpu, dtype):
    """graph=True: set_faces drops the captured graph, and the next step() is the golden of the
    new faces; None returns to the scalar-r kernels."""
    n, dt, tb = 301, NP[dtype], 8
    p = problem(n, 4 * tb)
    T0, F1, F2 = rough_field(n, dtype), rough_faces(n, dtype), rough_faces(n, dtype, seed=2)
    s = HeatSolver(p, dtype=dtype, backend="hip", tb=tb, arith="exact", device=0, graph=True, faces=F1)
    s.upload(T0)
    s.prepare(2 * tb)
    s.step(2 * tb)
    mid = R.ftcs(p, 2 * tb, dtype=dt, T0=T0, faces=F1)
    assert np.array_equal(s.download(), R.owned(mid))
    s.set_faces(F2)
    s.step(2 * tb)
    assert np.array_equal(s.download(), R.owned(R.ftcs(p, 2 * tb, dtype=dt, T0=mid, faces=F2)))
    s.set_faces(None)
    assert s.info()["faces"]["set"] is False
    s.upload(T0)
    s.step(2 * tb)
    assert np.array_equal(s.download(), R.owned(R.ftcs(p, 2 * tb, dtype=dt, T0=T0)))
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_raw_op(native, gpu, dtype):
    """tb_step(faces=) on a middle slab against the golden and heat2d_cpu_tb_div; NaN guard bands
    around the rows written: the new kernel writes nothing outside its rects."""
    for k, arith in ((8, "exact"), (depth_max(), "fma")):
        _raw_op("cuda", dtype, k, arith=arith)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_closed_domain(native, gpu, dtype):
    """The closed domain at n = 301, 48 steps (three cycles of depth 16), bitwise: the golden
    conserves heat (the CPU test above), so the engine does."""
    D = depth_max()
    steps = 3 * D
    got = run(301, dtype, "hip", D, steps, "exact", full=3, closed=True)
    g = gold(301, dtype, steps, "exact", closed=True)
    assert np.array_equal(got, g)
    bi, bj = BLOCK
    T0 = rough_field(301, dtype)
    assert np.array_equal(got[bi.start - 1:bi.stop - 1, bj.start - 1:bj.stop - 1].view(np.uint8), T0[BLOCK].view(np.uint8))


@pytest.mark.gpu
def test_hip_depth_clamp_and_refusals(native, gpu):
    F = rough_faces(301, "fp64")
    s = HeatSolver(problem(301, 4), backend="hip", device=0, tb=24, faces=F)
    info = s.info()
    s.close()
    assert info["tb"] == depth_max() and info["faces"]["max_tb"] == depth_max()
    Z = np.zeros((303, 303))
    for kw, why in ((dict(arith="jacobi"), "jacobi"), (dict(engine="jit"), "jit"), (dict(copy_swap=True), "copy-swap"),
                    (dict(bc_y="insulated"), "Dirichlet"), (dict(source=Z), "heat source"), (dict(rmap=Z), "diffusivity map")):
        with pytest.raises(RuntimeError, match=why):
            HeatSolver(problem(301, 4, 0.25), backend="hip", device=0, faces=F, **kw)
