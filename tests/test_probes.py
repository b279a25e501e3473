"""Probe points: the temperature at a few owned points after EVERY step, the
levels inside a fused pass included (HeatSolver probes=, csrc/kernels/probe_cone.hip).

Every comparison is bitwise. The golden is models.reference.probe_history (a
loop over ftcs_step); for scalar-r "fma" at an r that is no power of two, where
that golden keeps the exact expression, the oracle is the engine itself at
tb = 1, stepped one step at a time.
"""
import functools
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver, LoopbackGroup

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cycles as Y  # noqa: E402
import instance_matrix as M  # noqa: E402
from faces_worker import rough_faces  # noqa: E402
from probes_worker import plan_points  # noqa: E402
from source_worker import problem, rough_field, rough_source  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
# arith -> the sigma at which models.reference.ftcs has the engine's bits
SIGMA = {"exact": 0.2, "fma": 0.25, "jacobi": 0.25}
BCS = [("periodic", "periodic"), ("insulated", "insulated"), ("periodic", "insulated")]
PHYSICS = [(ph, ar) for ph in ("source", "rmap", "faces") for ar in ("exact", "fma")]


def corners(n):
    return [(1, 1), (1, n), (n, 1), (n, n)]


SEAMS77 = [(26, 40), (27, 40), (52, 13), (53, 64)]  # both sides of both seams of 26 / 26 / 25 rows


def rough_rmap(n, dtype, seed=2):
    """Frame-inclusive diffusion numbers in (0.0025, 0.25), 3 % exactly 0 (held points)."""
    rng = np.random.default_rng(2000 + seed)
    Rm = rng.uniform(0.0025, 0.25, (n + 2, n + 2))
    Rm[rng.uniform(size=Rm.shape) < 0.03] = 0.0
    return Rm.astype(NP[dtype])


def physics_kw(ph, n, dtype):
    if ph == "source":
        return {"source": rough_source(n, dtype)}
    if ph == "rmap":
        return {"rmap": rough_rmap(n, dtype)}
    if ph == "faces":
        return {"faces": rough_faces(n, dtype)}  # (NaN in the entries no point uses)
    return {}


@functools.lru_cache(maxsize=None)
def _golden(n, steps, probes, dtype, arith="exact", bc=("dirichlet", "dirichlet"), ph=None, sigma=None, own_frame=False):
    sg = SIGMA[arith] if sigma is None else sigma
    T0 = rough_field(n, dtype)
    if own_frame:  # the owned points uploaded inside the problem's own Dirichlet frame
        T0, rough = R.initial_field(problem(n, steps, sg), NP[dtype]), T0
        T0[1:-1, 1:-1] = rough[1:-1, 1:-1]
    H = R.probe_history(problem(n, steps, sg), steps, np.array(probes), dtype=NP[dtype], T0=T0,
                        arith=arith, bc_x=bc[0], bc_y=bc[1], **physics_kw(ph, n, dtype))
    H.setflags(write=False)
    return H


def golden(n, steps, probes, dtype, **kw):
    return _golden(n, steps, tuple(map(tuple, probes)), dtype, **kw)


def solver(n, steps, dtype, backend, tb, arith="exact", bc=("dirichlet", "dirichlet"), ph=None, sigma=None, **kw):
    if backend == "hip":
        kw.setdefault("device", 0)
    s = HeatSolver(problem(n, steps, SIGMA[arith] if sigma is None else sigma), dtype=dtype, backend=backend, tb=tb,
                   arith=arith, bc_x=bc[0], bc_y=bc[1], **physics_kw(ph, n, dtype), **kw)
    s.upload(rough_field(n, dtype))
    return s


def at(field, probes):
    p = np.array(probes)
    return field[p[:, 0] - 1, p[:, 1] - 1]


# ------------------------------------------------------------------ the golden

def test_golden_rows_are_points_of_successive_steps():
    n, dt = 33, np.float32
    p, T = problem(n, 9), rough_field(n, "fp32")
    pts = corners(n) + [(17, 5), (17, 5)]
    H = R.probe_history(p, 9, pts, dtype=dt, T0=T)
    assert H.shape == (9, 6) and H.dtype == dt
    for q in range(9):
        T = R.ftcs_step(T, p.r)
        assert np.array_equal(H[q], [T[i, j] for i, j in pts])
    S = rough_source(n, "fp32")
    Hs = R.probe_history(p, 3, pts, dtype=dt, T0=rough_field(n, "fp32"), arith="fma", source=S)
    T = rough_field(n, "fp32")
    for q in range(3):
        T = R.ftcs_step(T, p.r, "fma", source=S)
        assert np.array_equal(Hs[q], [T[i, j] for i, j in pts])


def test_golden_refuses_what_ftcs_step_refuses():
    n = 16
    p, S = problem(n, 2), rough_source(n, "fp64")
    with pytest.raises(ValueError):
        R.probe_history(p, 2, [(1, 1)], source=S, bc_x="periodic")
    with pytest.raises(ValueError):
        R.probe_history(p, 2, [(1, 1)], source=S, rmap=S)
    with pytest.raises(ValueError):
        R.probe_history(p, 2, [(1, 1)], arith="jacobi")  # r = 0.2
    for bad in ([(0, 1)], [(1, n + 1)], [(1.5, 2.0)], [1, 2]):
        with pytest.raises(ValueError):
            R.probe_history(p, 2, bad)


# ------------------------------------------------------------------ the kernel alone

RAW_N, RAW_COLS, RAW_ROWS = 150, 261, 70
# window row0 -> its probes: the grid corners on the first / last window, the
# middle window's first and last row (ends and middle) and its centre
RAW_WINDOWS = {0: [(1, 1), (1, RAW_COLS)], 80: [(RAW_N, 1), (RAW_N, RAW_COLS)],
               40: [(41, 1), (41, 131), (41, RAW_COLS), (110, 1), (110, 130), (110, RAW_COLS), (75, 130)]}


@functools.lru_cache(maxsize=None)
def _raw_data(dtype, ph):
    rng = np.random.default_rng(7)
    shape = (RAW_N + 2, RAW_COLS + 2)
    T0 = (10.0 ** rng.uniform(-1, 1, shape)).astype(NP[dtype])
    kw = {}
    if ph == "source":
        kw["source"] = (T0 * 10.0 ** rng.uniform(-3, -1, shape) * rng.choice([-1.0, 1.0], shape)).astype(NP[dtype])
    if ph == "rmap":
        kw["rmap"] = rng.uniform(0.0025, 0.25, shape).astype(NP[dtype])
    if ph == "faces":
        RX, RY = rng.uniform(0.0025, 0.25, shape), rng.uniform(0.0025, 0.25, shape)
        RX[rng.uniform(size=shape) < 0.03] = 0.0
        RY[rng.uniform(size=shape) < 0.03] = 0.0
        kw["faces"] = (RX.astype(NP[dtype]), RY.astype(NP[dtype]))
    return T0, kw


@functools.lru_cache(maxsize=None)
def _raw_golden(dtype, arith, ph, row0):
    """24 steps of the golden at the window's probes: depth k's history is its first k rows."""
    T0, kw = _raw_data(dtype, ph)
    H = R.probe_history(problem(RAW_N, 24, SIGMA[arith]), 24, RAW_WINDOWS[row0], dtype=NP[dtype], T0=T0, arith=arith, **kw)
    H.setflags(write=False)
    return H


def _raw_op(device, dtype, arith, ph, depths):
    """_raw_op's shape of tests/test_faces.py: n = 150, 261 columns, windows of 70 rows."""
    import torch

    from heat2d.ops import kernels as K
    T0, kw = _raw_data(dtype, ph)
    r = problem(RAW_N, 24, SIGMA[arith]).r
    for row0, pts in RAW_WINDOWS.items():
        L = K.make_layout(RAW_ROWS, RAW_COLS, halo=24, row0=row0, nrows_global=RAW_N)
        host = np.full((L.rows_alloc(), L.pitch), 3.25, dtype=NP[dtype])  # (pad columns and rows off the grid)
        for i in range(-L.halo, RAW_ROWS + L.halo):
            g = row0 + i  # global owned row; frame-inclusive g + 1
            if -1 <= g <= RAW_N:
                host[i + L.halo, L.cpad - 1:L.cpad + RAW_COLS + 1] = T0[g + 1]
        src = torch.from_numpy(host.reshape(-1).copy()).to(device)
        keep = src.clone()
        co = {}
        if ph == "source":
            co["source"] = K.source_field(kw["source"], L, src.dtype, device)
        if ph == "rmap":
            co["rmap"] = K.rmap_field(kw["rmap"], L, src.dtype, device)
        if ph == "faces":
            co["faces"] = K.faces_field(*kw["faces"], L, src.dtype, device)
        G = _raw_golden(dtype, arith, ph, row0)
        for k in depths:
            H = K.probe_cone(src, L, k, r, pts, arith=arith, **co)
            assert tuple(H.shape) == (k, len(pts))
            assert np.array_equal(H.cpu().numpy(), G[:k]), (row0, k)
        assert torch.equal(src, keep), "the cone wrote into its source field"


@pytest.mark.parametrize("arith", ["exact", "fma", "jacobi"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_twin_every_depth(native, dtype, arith):
    _raw_op("cpu", dtype, arith, None, range(1, 25))


@pytest.mark.parametrize("ph,arith", PHYSICS)
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_twin_physics(native, dtype, ph, arith):
    _raw_op("cpu", dtype, arith, ph, (1, 8, 16))


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fma", "jacobi"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_kernel_every_depth(native, gpu, dtype, arith):
    _raw_op("cuda", dtype, arith, None, range(1, 25))


@pytest.mark.gpu
@pytest.mark.parametrize("ph,arith", PHYSICS)
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_kernel_physics(native, gpu, dtype, ph, arith):
    _raw_op("cuda", dtype, arith, ph, (1, 8, 16))


def test_raw_op_argument_errors(native):
    import torch

    from heat2d.ops import kernels as K
    L = K.make_layout(20, 30, halo=8, row0=10, nrows_global=60)
    src = torch.zeros(L.elems(), dtype=torch.float64)
    for bad in ([(10, 1)], [(31, 1)], [(11, 0)], [(11, 31)], [(11.5, 1.0)], [11, 1], np.zeros((2, 3), dtype=np.int64)):
        with pytest.raises(ValueError):
            K.probe_cone(src, L, 2, 0.2, bad)
    with pytest.raises(ValueError):
        K.probe_cone(src, L, 9, 0.2, [(11, 1)])  # deeper than the halo
    with pytest.raises(ValueError):
        K.probe_cone(src, L, 2, 0.2, [(11, 1)] * (K.MAX_PROBES + 1))
    assert tuple(K.probe_cone(src, L, 2, 0.2, [(11, 1), (11, 1)]).shape) == (2, 2)  # duplicates are allowed


# ------------------------------------------------------------------ the solver's history

def check_history(s, n, steps, pts, dtype, calls=None, **gk):
    for m in calls or [steps]:
        s.step(m)
    H = s.probe_history()
    assert H.dtype == NP[dtype] and H.shape == (steps, len(pts))
    assert np.array_equal(H, golden(n, steps, pts, dtype, **gk))
    assert np.array_equal(H[-1], at(s.download(), pts)), "the last row is not download() at the probes"
    pr = s.info()["probes"]
    assert pr == {"count": len(pts), "capacity": steps, "recorded": steps}
    assert list(s.probe_index) == list(range(len(pts)))


@pytest.mark.parametrize("tb", [1, 2, 7, 8])
@pytest.mark.parametrize("n", [77, 301])
def test_cpu_solver_history(native, n, tb):
    pts = corners(n) + [(n // 2, n // 2), (2, n - 1), (n // 2, n // 2)]
    for dtype in ("fp64", "fp32"):
        s = solver(n, 23, dtype, "cpu", tb, probes=pts)
        check_history(s, n, 23, pts, dtype)
        s.close()


@pytest.mark.parametrize("arith", ["fma", "jacobi"])
def test_cpu_solver_history_arith(native, arith):
    pts = corners(77) + [(39, 39)]
    for dtype in ("fp64", "fp32"):
        s = solver(77, 23, dtype, "cpu", 8, arith=arith, probes=pts)
        check_history(s, 77, 23, pts, dtype, arith=arith)
        s.close()


def _loopback(backend, dtype):
    n, pts = 77, SEAMS77 + corners(77)
    g = LoopbackGroup(problem(n, 23), 3, dtype=dtype, backend=backend, tb=7, arith="exact", probes=pts,
                      **({"device": 0} if backend == "hip" else {}))
    assert [r for _, r in g.slabs()] == [26, 26, 25]
    g.upload(rough_field(n, dtype))
    g.step(23)
    H = g.probe_history()
    assert H.shape == (23, len(pts)) and np.array_equal(H, golden(n, 23, pts, dtype))
    assert np.array_equal(H[-1], at(g.download(), pts))
    with pytest.raises(RuntimeError):  # the capacity defaults to problem.ntime
        g.step(1)
    g.close()


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_loopback_three_ranks(native, dtype):
    _loopback("cpu", dtype)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_cpu_gloo_three_ranks(native, tmp_path):
    n, pts = 77, SEAMS77 + corners(77)
    a = {"n": n, "steps": 23, "tb": 7, "dtype": "fp64", "arith": "exact", "probes": pts}
    port = _free_port()
    env = dict(os.environ, HEAT2D_PLAN_CACHE="off")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "probes_worker.py"), "gloo", str(r), "3", str(port),
                               str(tmp_path), json.dumps(a)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(3)]
    try:
        outs = [p.communicate(timeout=240)[0].decode(errors="replace") for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(o[-2000:] for o in outs)
    H = np.full((23, len(pts)), np.nan)
    seen = []
    for r in range(3):
        idx = np.load(tmp_path / f"I_{r}.npy")
        H[:, idx] = np.load(tmp_path / f"H_{r}.npy")
        seen += list(idx)
    assert sorted(seen) == list(range(len(pts))), "every probe belongs to exactly one rank"
    assert np.array_equal(H, golden(n, 23, pts, "fp64", own_frame=True))


@pytest.mark.parametrize("bc", BCS, ids=lambda b: f"{b[0]}-{b[1]}")
def test_cpu_boundaries(native, bc):
    n, pts = 77, corners(77) + [(39, 39)]
    for dtype in ("fp64", "fp32"):
        s = solver(n, 19, dtype, "cpu", 8, bc=bc, probes=pts)
        check_history(s, n, 19, pts, dtype, bc=bc)
        s.close()


@pytest.mark.parametrize("ph,arith", PHYSICS)
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_physics(native, dtype, ph, arith):
    n, pts = 77, corners(77) + [(39, 39), (11, 21), (12, 22)]  # (two cells of faces_worker.BLOCK)
    s = solver(n, 19, dtype, "cpu", 8, arith=arith, ph=ph, sigma=0.2, probes=pts)
    check_history(s, n, 19, pts, dtype, arith=arith, ph=ph, sigma=0.2)
    s.close()


# ------------------------------------------------------------------ life cycle, refusals, arguments

def _life_cycle(backend, tb, n=77, dtype="fp64", **kw):
    A, B = corners(n) + [(39, 39)], [(5, 6), (70, 3), (5, 6)]
    s = solver(n, 40, dtype, backend, tb, probes=A, probe_steps=12, **kw)
    assert s.info()["probes"] == {"count": 5, "capacity": 12, "recorded": 0}
    s.prepare(5)  # plans, trials, captures: nothing recorded
    assert s.info()["probes"]["recorded"] == 0 and s.probe_history().shape == (0, 5)
    s.step(5)
    s.step(5)  # two step(n) calls: 2 n rows
    H = s.probe_history()
    assert np.array_equal(H, golden(n, 10, A, dtype))
    s.prepare(5)
    assert np.array_equal(s.probe_history(), H) and s.info()["probes"]["recorded"] == 10
    before = s.download()
    with pytest.raises(RuntimeError, match="probe history full"):
        s.step(3)  # 13 > 12: raises before it launches anything
    with pytest.raises(RuntimeError, match="probe history full"):
        s.step_stats(3)
    assert np.array_equal(s.download(), before) and np.array_equal(s.probe_history(), H)
    assert s.steps_done == 10
    s.step(2)  # exactly full
    assert np.array_equal(s.probe_history(), golden(n, 12, A, dtype))
    s.clear_probe_history()
    assert s.info()["probes"] == {"count": 5, "capacity": 12, "recorded": 0}
    s.step(4)
    G = golden(n, 16, A, dtype)
    assert np.array_equal(s.probe_history(), G[12:16])
    s.set_probes(B, 9)  # between steps: new points, an empty history
    assert s.info()["probes"] == {"count": 3, "capacity": 9, "recorded": 0}
    st = s.step_stats(5)  # step_stats records as step does
    assert np.isfinite(st["sum"])
    s.step(3)
    assert np.array_equal(s.probe_history(), golden(n, 24, B, dtype)[16:24])
    s.set_probes(None)  # cleared: nothing recorded, nothing refused
    assert s.info()["probes"] == {"count": 0, "capacity": 0, "recorded": 0}
    s.step(16)
    assert s.probe_history().shape == (0, 0)
    assert np.array_equal(at(s.download(), A), golden(n, 40, A, dtype)[39])  # 10 + 2 + 4 + 5 + 3 + 16 steps
    s.close()


def test_cpu_life_cycle(native):
    _life_cycle("cpu", 7)


def test_capacity_defaults_to_ntime(native):
    s = solver(33, 6, "fp64", "cpu", 4, probes=[(1, 1)])
    assert s.info()["probes"]["capacity"] == 6
    s.close()


def test_refusals(native):
    p = problem(33, 4)
    with pytest.raises(RuntimeError, match="fast"):
        HeatSolver(p, backend="cpu", arith="fast", probes=[(1, 1)])
    with pytest.raises(RuntimeError, match="copy-swap"):
        HeatSolver(p, backend="cpu", copy_swap=True, probes=[(1, 1)])
    s = HeatSolver(p, backend="cpu", arith="fast")
    with pytest.raises(RuntimeError, match="fast"):
        s.set_probes([(1, 1)])
    s.close()


def test_argument_errors(native):
    p = problem(33, 4)
    s = HeatSolver(p, backend="cpu")
    for bad in ([(0, 1)], [(34, 1)], [(1, 0)], [(1, 34)], [(1.5, 2.0)], [("a", "b")], [1, 2], [(1, 2, 3)],
                np.zeros((2, 2, 2), dtype=np.int64), [(1, 1)] * 4097):
        with pytest.raises(ValueError):
            s.set_probes(bad)
        with pytest.raises(ValueError):
            LoopbackGroup(p, 2, backend="cpu", probes=bad)
    with pytest.raises(ValueError):
        s.set_probes([(1, 1)], 0)
    s.set_probes([(1, 1)] * 4096)  # kMaxProbes points, all the same
    assert s.info()["probes"]["count"] == 4096
    s.close()


def test_memory_planner_counts_the_history(native):
    import heat2d
    base = heat2d.footprint(4096, dtype="fp64")
    with_p = heat2d.footprint(4096, dtype="fp64", probes=1024, probe_steps=500)
    extra = 1024 * 500 * 8 + 16 * 1024 + 8  # the history, the index list, the row-base word
    assert with_p["total_bytes"] - base["total_bytes"] == extra and with_p["field_bytes"] == base["field_bytes"]
    assert heat2d.footprint(4096, dtype="fp32", probes=3, probe_steps=7)["total_bytes"] - \
        heat2d.footprint(4096, dtype="fp32")["total_bytes"] == 3 * 7 * 4 + 16 * 3 + 8
    budget = 1 << 30
    a = heat2d.plan_max_grid("fp64", free_bytes=budget, reserve=0)
    b = heat2d.plan_max_grid("fp64", free_bytes=budget, reserve=0, probes=4096, probe_steps=4096)
    assert b["n"] < a["n"] and b["footprint_bytes"] <= budget


def _py(cwd, *args, nproc=1):
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2")
    cmd = [sys.executable, "-m", "heat2d", *args]
    if nproc > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port()), "-m", "heat2d", *args]
    return subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)


def test_drivers_probes(native, tmp_path):
    """--probes through both drivers on the CPU backend, text and .npy: the file written is the
    golden, on 2 ranks the columns come back in the list's order, whatever soln / --output say."""
    import heat2d
    from heat2d.ops import _native as N
    n, steps = 64, 30
    (tmp_path / "input.dat").write_text(f"{n} 0.2 0.05 1.0 {steps} 0\n")
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "uniform")
    # rows of both slabs of 32, out of order, a duplicate, the corners
    pts = [(40, 3), (1, 1), (33, 64), (32, 64), (64, 64), (2, 2), (40, 3), (1, 64), (64, 1)]
    (tmp_path / "p.txt").write_text("# i j\n" + "\n".join(f"{i} {j}  # probe" if k % 2 else f"  {i}\t{j}"
                                                           for k, (i, j) in enumerate(pts)) + "\n\n")
    np.save(tmp_path / "p.npy", np.array(pts, dtype=np.int32))
    gold = R.probe_history(prob, steps, pts, arith="exact")
    assert len(np.unique(gold)) > steps  # (the uniform IC moves at these points)
    cli = [N.CLI_PATH, "--cpu", "--quiet", "--ic", "uniform", "--arith", "exact", "--tb", "7"]
    pyargs = ["--backend", "cpu", "--ic", "uniform", "--quiet", "--arith", "exact", "--tb", "7"]
    runs = 0
    for f in ("p.txt", "p.npy"):
        for ranks in (1, 2):
            for drv in ("cli", "py"):
                out_name = f"h_{drv}_{ranks}_{f[2:]}.npy"
                if drv == "cli":
                    out = subprocess.run([*cli, "--gpus", str(ranks), "--probes", f, "--probes-out", out_name, "--output", "none"],
                                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
                else:
                    out = _py(tmp_path, *pyargs, "--probes", f, "--probes-out", out_name, "--output", "none", nproc=ranks)
                assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
                H = np.load(tmp_path / out_name)
                assert H.dtype == np.float64 and np.array_equal(H, gold), (drv, ranks, f)
                runs += 1
    assert runs == 8
    # the default name, fp32, and a checkpointed restart that records from its restart step
    out = subprocess.run([*cli, "--dtype", "fp32", "--probes", "p.txt", "--ntime", "12", "--checkpoint", "ck", "--output", "none"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    g32 = R.probe_history(prob, steps, pts, dtype=np.float32, arith="exact")
    assert np.array_equal(np.load(tmp_path / "probes.npy"), g32[:12])
    for drv in ("cli", "py"):
        os.remove(tmp_path / "probes.npy")
        if drv == "cli":
            out = subprocess.run([*cli, "--dtype", "fp32", "--probes", "p.npy", "--restart", "ck", "--output", "none"],
                                 cwd=tmp_path, capture_output=True, text=True, timeout=300)
        else:
            out = _py(tmp_path, *pyargs, "--dtype", "fp32", "--probes", "p.npy", "--restart", "ck", "--output", "none")
        assert out.returncode == 0, out.stdout + out.stderr
        assert np.array_equal(np.load(tmp_path / "probes.npy"), g32[12:]), drv
    # files that must fail
    (tmp_path / "bad1.txt").write_text("1 2\n3\n")
    (tmp_path / "bad2.txt").write_text("1 2\n0 5\n")
    (tmp_path / "bad3.txt").write_text("1 2 3\n")
    np.save(tmp_path / "bad4.npy", np.array(pts, dtype=np.float64))
    np.save(tmp_path / "bad5.npy", np.array(pts, dtype=np.int64).T.copy())
    for f in ("bad1.txt", "bad2.txt", "bad3.txt", "bad4.npy", "bad5.npy"):
        bad = subprocess.run([*cli, "--probes", f, "--output", "none"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0 and "--probes" in bad.stdout + bad.stderr, f
        bad = _py(tmp_path, *pyargs, "--probes", f, "--output", "none")
        assert bad.returncode != 0 and "--probes" in bad.stdout + bad.stderr, f


# ------------------------------------------------------------------ negative controls

CONTROL_PTS = corners(77) + SEAMS77 + [(39, 39)]


def _numpy_history(T, r, steps, pts, order="golden", pin=True):
    """The history in plain NumPy, with the summation order or the pinning changed."""
    T = T.copy()
    r, four = T.dtype.type(r), T.dtype.type(4)
    H = np.empty((steps, len(pts)), dtype=T.dtype)
    for q in range(steps):
        P = T if pin else np.pad(T, 1, mode="edge")  # not pinned: the frame updated from an edge-padded field
        c, s, e, n, w = P[1:-1, 1:-1], P[2:, 1:-1], P[1:-1, 2:], P[:-2, 1:-1], P[1:-1, :-2]
        total = (((s + e) + n) + w) if order == "golden" else ((n + w) + (s + e))
        new = c + r * (total - four * c)
        if pin:
            T = T.copy()
            T[1:-1, 1:-1] = new
        else:
            T = new
        H[q] = [T[i, j] for i, j in pts]
    return H


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_control_summation_order(native, dtype):
    """The data discriminates: (N + W) + (S + E) differs from the golden in every column."""
    n, p = 77, problem(77, 24)
    G = golden(n, 24, CONTROL_PTS, dtype)
    assert np.array_equal(_numpy_history(rough_field(n, dtype), p.r, 24, CONTROL_PTS), G)
    other = _numpy_history(rough_field(n, dtype), p.r, 24, CONTROL_PTS, order="swapped")
    diff = other != G
    print(f"{dtype}: {diff.sum()} of {diff.size} entries differ, per-column minimum {diff.sum(axis=0).min()}")
    assert diff.any(axis=0).all(), "a column where the swapped order has the golden's bits"
    s = solver(n, 24, dtype, "cpu", 8, probes=CONTROL_PTS)
    s.step(24)
    assert np.array_equal(s.probe_history(), G) and not np.array_equal(s.probe_history(), other)
    s.close()


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_control_frame_pinning(native, dtype):
    """A history whose Dirichlet frame is updated instead of pinned differs at (1, 1)."""
    n, p = 77, problem(77, 24)
    G = golden(n, 24, CONTROL_PTS, dtype)
    loose = _numpy_history(rough_field(n, dtype), p.r, 24, CONTROL_PTS, pin=False)
    assert (loose[:, 0] != G[:, 0]).any(), "the unpinned frame does not show at (1, 1)"
    s = solver(n, 24, dtype, "cpu", 8, probes=CONTROL_PTS)
    s.step(24)
    assert np.array_equal(s.probe_history(), G)
    s.close()


# ------------------------------------------------------------------ GPU: fused passes

def _worker(tmp_path, a, env):
    out = subprocess.run([sys.executable, os.path.join(HERE, "probes_worker.py"), str(tmp_path), json.dumps(a)],
                         env=dict(os.environ, HEAT2D_PLAN_CACHE="off", **env), capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]


def _check_worker(tmp_path, n, dtype, tb, arith="exact", pipe=None):
    steps = 2 * tb + 3
    H, T = np.load(tmp_path / f"H_{tb}.npy"), np.load(tmp_path / f"T_{tb}.npy")
    pts = [tuple(int(v) for v in p) for p in np.load(tmp_path / f"P_{tb}.npy")]
    info = json.loads((tmp_path / f"info_{tb}.json").read_text())
    Y.assert_ran(info["cycle_hist"], tb, 2)
    assert info["probes"] == {"count": len(pts), "capacity": steps, "recorded": steps}
    assert pts == plan_points(n, dtype, tb, info["plan"]) and len(pts) >= 15
    if pipe is not None:
        assert info["plan"]["pipe"] == pipe
    assert np.array_equal(H, golden(n, steps, pts, dtype, arith=arith, sigma=0.2)), (dtype, tb)
    assert np.array_equal(H[-1], at(T, pts))
    return info


def _tbs(dtype):
    return [1, 7, 16, 24 if dtype == "fp64" else 20]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", list(M.MODES))
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_every_step_through_fused_passes(native, gpu, tmp_path, dtype, mode):
    """2K + 3 steps as calls K, K, 3 at depths 1, 7, 16 and the deepest, in the split plan and in
    the single three-band launch: probes at the corners, across a strip's useful-width boundary
    and across a band seam of the plan the solver reports."""
    n = M.N_OF[dtype]
    _worker(tmp_path, {"n": n, "dtype": dtype, "tbs": _tbs(dtype), "arith": "exact", "sigma": 0.2}, M.MODES[mode])
    for tb in _tbs(dtype):
        info = _check_worker(tmp_path, n, dtype, tb)
        assert (info["plan"]["valid"] == 2) == (mode == "single")


@pytest.mark.gpu
@pytest.mark.parametrize("pipe", [1, 0])
def test_hip_beside_the_wave_pair_kernel(native, gpu, tmp_path, pipe):
    """fp64 at depths 16 and 24 with the wave-pair interior kernel on and off."""
    n = M.N_OF["fp64"]
    _worker(tmp_path, {"n": n, "dtype": "fp64", "tbs": [16, 24], "arith": "exact", "sigma": 0.2},
            {"HEAT2D_PIPE": str(pipe)})
    for tb in (16, 24):
        _check_worker(tmp_path, n, "fp64", tb, pipe=pipe)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_loopback_three_ranks(native, gpu, dtype):
    _loopback("hip", dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("bc", BCS, ids=lambda b: f"{b[0]}-{b[1]}")
def test_hip_boundaries(native, gpu, bc):
    n, pts = 77, corners(77) + [(39, 39)]
    for dtype in ("fp64", "fp32"):
        s = solver(n, 19, dtype, "hip", 8, bc=bc, probes=pts)
        check_history(s, n, 19, pts, dtype, calls=[8, 11], bc=bc)
        Y.assert_ran(s.cycle_hist(), 8)
        s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("ph,arith", PHYSICS)
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_physics(native, gpu, dtype, ph, arith):
    n, pts = 77, corners(77) + [(39, 39), (11, 21), (12, 22)]
    s = solver(n, 19, dtype, "hip", 8, arith=arith, ph=ph, sigma=0.2, probes=pts)
    check_history(s, n, 19, pts, dtype, calls=[8, 11], arith=arith, ph=ph, sigma=0.2)
    Y.assert_ran(s.cycle_hist(), 8)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_graph_replay(native, gpu, dtype):
    """graph=True: prepare(n) captures and records nothing; step(n) twice replays the pair graph
    (2 K of every call's 2 K + 3 steps) and gives 2 n correct rows."""
    n, K = 301, 7
    m = 2 * K + 3
    pts = corners(n) + [(150, 151), (K, K), (n - K, 2)]
    s = solver(n, 2 * m, dtype, "hip", K, graph=True, probes=pts)
    s.prepare(m)
    assert s.info()["probes"]["recorded"] == 0
    assert Y.depths(K, [m, m], graph=True).count(K) >= 2
    check_history(s, n, 2 * m, pts, dtype, calls=[m, m])
    Y.assert_ran(s.cycle_hist(), K, 2)
    s.close()


@pytest.mark.gpu
def test_hip_life_cycle(native, gpu):
    """set_probes between steps, clear, overflow refused before anything is launched, prepare."""
    _life_cycle("hip", 7)
    _life_cycle("hip", 7, graph=True)
    with pytest.raises(RuntimeError, match="jit"):
        HeatSolver(problem(77, 4), backend="hip", device=0, engine="jit", probes=[(1, 1)])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_engine_as_oracle(native, gpu, dtype):
    """Scalar-r fma at sigma 0.2, where ftcs(arith="fma") keeps the exact expression: tb 16
    against the same solver at tb 1 stepped singly, the points downloaded after each step."""
    n, steps = 301, 35
    pts = corners(n) + [(150, 151), (16, 17), (n - 15, 122)]
    one = solver(n, steps, dtype, "hip", 1, arith="fma", sigma=0.2)
    want = np.empty((steps, len(pts)), dtype=NP[dtype])
    for q in range(steps):
        one.step(1)
        want[q] = at(one.download(), pts)
    one.close()
    s = solver(n, steps, dtype, "hip", 16, arith="fma", sigma=0.2, probes=pts)
    for m in (16, 16, 3):
        s.step(m)
    Y.assert_ran(s.cycle_hist(), 16, 2)
    assert np.array_equal(s.probe_history(), want)
    assert not np.array_equal(want, golden(n, steps, pts, dtype, arith="exact", sigma=0.2)), \
        "fma at sigma 0.2 has the exact form's bits: the oracle shows nothing"
    s.close()
