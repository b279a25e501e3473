"""Spatially varying diffusivity, u_t = nu(x, y) lap(u) (the non-divergence form):
the scalar diffusion number r of every fused level is replaced by the element of
a map R = nu(x, y) dt / dx^2,

    exact: T' = C + R[i,j] * ((((S + E) + N) + W) - 4C)
    fma:   T' = fma(R[i,j], fma(-4, C, sum), C)

bitwise against the NumPy golden (models.reference.ftcs(rmap=)) at every pass
depth, launch plan and rank count, on the CPU twin and on the HIP engine
(tb_kernel_var, csrc/kernels/tb_impl.hpp).

Data (fixed seeds): field values 10**uniform(-1, 1), frame included
(tests/source_worker.py rough_field); map values uniform(0.01, 0.25), exactly 0
where a second uniform draw is < 0.03 (embedded fixed points), nonzero frame
entries (the engine must ignore them), no -0.0 anywhere.

Negative controls of the data come first: a map rolled by one row, adjacent
columns swapped pairwise (the fp32 ring-order mistake), the map transposed, the
map replaced by its mean and the other arithmetic form all give other bits than
the golden, so only an engine that multiplies by the right element, of the right
row, in the right form, can pass the bitwise tests.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import heat2d
from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver, LoopbackGroup
from heat2d.ops import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cycles as Y  # noqa: E402
from rmap_worker import problem, rough_field, rough_map  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
_DEPTH = []


def depth_max():
    """The map kernels' deepest pass (common.hpp kMaxTBVar), as the library reports it
    (tests/test_rmap_isa.py holds it against the instances in the code objects)."""
    if not _DEPTH:
        s = HeatSolver(problem(8, 1), backend="cpu", rmap=np.full((10, 10), 0.1))
        _DEPTH.append(s.info()["rmap"]["max_tb"])
        s.close()
    return _DEPTH[0]


def depth(tb):
    return depth_max() if tb == "D" else tb


_GOLD = {}


def gold(n, dtype, steps, arith="exact", rows=None, seed=1, framed=False):
    """The golden run (computed once, read-only). rows: the first rows x n of the grid."""
    key = (n, dtype, steps, arith, rows, seed)
    if key not in _GOLD:
        T0, M = rough_field(n, dtype, rows=rows), rough_map(n, dtype, rows=rows, seed=seed)
        g = np.ascontiguousarray(R.ftcs(problem(n, steps), steps, dtype=NP[dtype], T0=T0, arith=arith, rmap=M))
        g.setflags(write=False)
        _GOLD[key] = g
    return _GOLD[key] if framed else R.owned(_GOLD[key])


def run(n, dtype, backend, tb, steps, arith="exact", ranks=1, rows=None, prepare=False, full=0, **kw):
    """full > 0: the steps as tests/cycles.py calls(tb, steps, full) — `full`
    cycles of depth tb, asserted from cycle_hist(), then the remainder — and
    not as one step() call, whose balanced cycles are all shallower than tb."""
    p = problem(n, steps)
    T0, M = rough_field(n, dtype, rows=rows), rough_map(n, dtype, rows=rows)
    dev = dict(device=0) if backend == "hip" else {}
    if ranks > 1:
        s = LoopbackGroup(p, ranks, dtype=dtype, backend=backend, tb=tb, arith=arith, rmap=M, **dev, **kw)
        s.upload(T0)
        s.step(steps)
        out = s.download()
        s.close()
        assert not full
        return out
    s = HeatSolver(p, dtype=dtype, backend=backend, tb=tb, arith=arith, rmap=M, rows=rows, **dev, **kw)
    s.upload(T0)
    for m in Y.calls(tb, steps, full) if full else [steps]:
        if prepare:
            s.prepare(m)
        s.step(m)
    out, hist = s.download(), s.cycle_hist()
    s.close()
    if full:
        Y.assert_ran(hist, tb, full)
    return out


# ------------------------------------------------------------------ CPU: the golden and its data

@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_defaults_untouched(dtype):
    """ftcs / ftcs_step with rmap=None are today's functions, bit for bit."""
    T0 = rough_field(77, dtype)
    p = problem(77, 8)
    dt, r, four = NP[dtype], NP[dtype](p.r), NP[dtype](4)
    T = T0.copy()
    for _ in range(8):
        c = T[1:-1, 1:-1]
        Q = T.copy()
        Q[1:-1, 1:-1] = c + r * ((((T[2:, 1:-1] + T[1:-1, 2:]) + T[:-2, 1:-1]) + T[1:-1, :-2]) - four * c)
        T = Q
    assert np.array_equal(R.ftcs(p, 8, dtype=dt, T0=T0), T)
    assert np.array_equal(R.ftcs(p, 8, dtype=dt, T0=T0, rmap=None), T)
    assert np.array_equal(R.ftcs_step(T0, p.r, rmap=None), R.ftcs_step(T0, p.r))
    for arith in ("fma", "jacobi"):
        q = problem(77, 3, 0.25)
        assert np.array_equal(R.ftcs(q, 3, dtype=dt, T0=T0, arith=arith, rmap=None), R.ftcs(q, 3, dtype=dt, T0=T0, arith=arith))
    for bc in (dict(bc_x="periodic"), dict(bc_y="insulated")):
        assert np.array_equal(R.ftcs(p, 3, dtype=dt, T0=T0, rmap=None, **bc), R.ftcs(p, 3, dtype=dt, T0=T0, **bc))


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_uniform_map_is_the_scalar_run(dtype):
    """R == problem.r everywhere, exact: the scalar golden bit for bit."""
    p, dt = problem(77, 8), NP[dtype]
    T0 = rough_field(77, dtype)
    M = np.full((79, 79), p.r)
    assert np.array_equal(R.ftcs(p, 8, dtype=dt, T0=T0, arith="exact", rmap=M), R.ftcs(p, 8, dtype=dt, T0=T0, arith="exact"))


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_negative_controls(dtype):
    """n = 77, 8 steps: four wrong maps, each against the golden; and fma against exact."""
    n, K, dt = 77, 8, NP[dtype]
    p, T0, M = problem(n, K), rough_field(n, dtype), rough_map(n, dtype)
    g = gold(n, dtype, K)

    def differs(Mx):
        return np.mean(R.owned(R.ftcs(p, K, dtype=dt, T0=T0, rmap=Mx)) != g)

    rolled = M.copy()
    rolled[1:-1] = np.roll(M[1:-1], 1, axis=0)
    swapped = M.copy()  # owned columns (1, 2), (3, 4), ... exchanged: a lane's (c0, c2, c1, c3) read as (c0, c1, c2, c3)
    m = (n // 2) * 2
    swapped[:, 1:1 + m:2], swapped[:, 2:2 + m:2] = M[:, 2:2 + m:2], M[:, 1:1 + m:2]
    mean = np.full_like(M, M[1:-1, 1:-1].mean())
    d = {"rolled one row": differs(rolled), "columns swapped pairwise": differs(swapped), "transposed": differs(M.T.copy()),
         "replaced by its mean": differs(mean)}
    for k, v in d.items():
        print(f"{dtype}: map {k}: differs at {100 * v:.1f} % of the owned points")
    assert all(v > 0.5 for v in d.values()), d
    d_fma = np.mean(gold(n, dtype, K, "fma") != g)
    print(f"{dtype}: fma differs from exact at {100 * d_fma:.1f} % of the owned points")
    assert d_fma > 0.05


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_zero_holds_and_maximum_principle(dtype, arith):
    """R == 0 keeps a point's bits; R in [0, 1/4] keeps the field inside [min T0, max T0]."""
    n = 77
    T0, M = rough_field(n, dtype), rough_map(n, dtype)
    hold = R.owned(M) == 0
    assert hold.sum() == 177 and (M[0] != 0).all() and (M[-1] != 0).all() and (M[:, 0] != 0).all() and (M[:, -1] != 0).all()
    assert not np.signbit(T0).any() and not np.signbit(M).any()
    g = gold(n, dtype, 8, arith, framed=True)
    assert np.array_equal(R.owned(g)[hold].view(np.uint8), R.owned(T0)[hold].view(np.uint8))
    assert np.array_equal(g[0], T0[0]) and np.array_equal(g[:, -1], T0[:, -1])
    assert T0.min() <= g.min() and g.max() <= T0.max()


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
    """3 ranks on 77 rows (26 / 26 / 25): every member slices its rows of the global map."""
    for arith in ("exact", "fma"):
        got = run(77, dtype, "cpu", 7, 23, arith, ranks=3)
        assert np.array_equal(got, gold(77, dtype, 23, arith)), arith


def test_refusals(native):
    p, M = problem(40, 4, 0.25), rough_map(40, "fp64")
    for kw, why in ((dict(arith="jacobi"), "jacobi"), (dict(arith="fast"), "fast"), (dict(bc_x="periodic"), "Dirichlet"),
                    (dict(bc_y="periodic"), "Dirichlet"), (dict(bc_x="insulated"), "Dirichlet"),
                    (dict(bc_y="insulated"), "Dirichlet"), (dict(copy_swap=True), "copy-swap"),
                    (dict(source=np.zeros_like(M)), "heat source")):
        with pytest.raises(RuntimeError, match=why):
            HeatSolver(p, backend="cpu", rmap=M, **kw)
    with pytest.raises(RuntimeError, match="jit|HIP"):
        HeatSolver(p, backend="cpu", engine="jit", rmap=M)
    with pytest.raises(ValueError, match="frame-inclusive"):
        HeatSolver(p, backend="cpu", rmap=M[1:])
    for bad in (-0.01, np.nan, np.inf):
        Mb = M.copy()
        Mb[7, 9] = bad
        with pytest.raises(ValueError, match="finite and >= 0"):
            HeatSolver(p, backend="cpu", rmap=Mb)
    Mf = M.copy()  # frame entries are ignored, whatever they hold
    Mf[0, :] = np.nan
    Mf[:, -1] = -3.0
    HeatSolver(p, backend="cpu", rmap=Mf).close()
    s = HeatSolver(p, backend="cpu")  # built without a map: none can be set later
    with pytest.raises(RuntimeError, match="without a diffusivity map"):
        s.set_rmap(M)
    s.set_rmap(None)
    s.close()
    T0 = rough_field(40, "fp64")
    with pytest.raises(ValueError, match="exact"):
        R.ftcs(p, 2, T0=T0, arith="jacobi", rmap=M)
    for bc in (dict(bc_x="periodic"), dict(bc_y="periodic"), dict(bc_x="insulated"), dict(bc_y="insulated")):
        with pytest.raises(ValueError, match="Dirichlet"):
            R.ftcs(p, 2, T0=T0, rmap=M, **bc)


def test_auto_resolves_to_exact(native):
    """r = 1/4 on the reference IC (where auto picks jacobi, and with a source fma): exact with a map."""
    inp = heat2d.parse_input_text("64 0.25 0.05 1.0 6 0")
    p = heat2d.make_problem(inp, "ghost", "uniform")
    M = rough_map(p.n_owned, "fp64")
    s = HeatSolver(p, backend="cpu", arith="auto", rmap=M)
    info = s.info()
    s.step(6)
    got = s.download()
    s.close()
    assert info["arith"] == N.ARITH["exact"] and s.arith == "exact"
    assert info["rmap"] == {"enabled": True, "set": True, "max_tb": depth_max()} and depth_max() >= 8
    assert np.array_equal(got, R.owned(R.ftcs(p, 6, arith="exact", rmap=M)))
    g = LoopbackGroup(p, 2, backend="cpu", arith="auto", rmap=M)
    assert g.arith_code(0) == N.ARITH["exact"] and g.arith_code(1) == N.ARITH["exact"]
    g.close()
    s = HeatSolver(p, backend="cpu")
    assert s.info()["rmap"] == {"enabled": False, "set": False, "max_tb": 0}
    s.close()


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_set_rmap_none_and_fresh(native, dtype):
    """set_rmap(None): the run equals the scalar-r run; a fresh map between two
    step() calls: the golden run the same way."""
    n, dt, p = 77, NP[dtype], problem(77, 20)
    T0, M1, M2 = rough_field(n, dtype), rough_map(n, dtype), rough_map(n, dtype, seed=2)
    s = HeatSolver(p, dtype=dtype, backend="cpu", tb=7, arith="exact", rmap=M1)
    s.set_rmap(None)
    assert s.info()["rmap"]["set"] is False and s.rmap_sha256 is None
    s.upload(T0)
    s.step(20)
    assert np.array_equal(s.download(), R.owned(R.ftcs(p, 20, dtype=dt, T0=T0)))
    s.upload(T0)
    s.set_rmap(M1)
    s.step(9)
    s.set_rmap(M2)
    s.step(11)
    got = s.download()
    s.close()
    mid = R.ftcs(p, 9, dtype=dt, T0=T0, rmap=M1)
    assert np.array_equal(got, R.owned(R.ftcs(p, 11, dtype=dt, T0=mid, rmap=M2)))


def test_step_stats_takes_the_unfused_path(native):
    p, M = problem(77, 12), rough_map(77, "fp64")
    s = HeatSolver(p, backend="cpu", tb=5, arith="exact", rmap=M)
    s.upload(rough_field(77, "fp64"))
    st = s.step_stats(12)
    got = s.download()
    s.close()
    g = gold(77, "fp64", 12).astype(np.float64)
    assert np.array_equal(got, g) and st["min"] == g.min() and st["max"] == g.max()


def test_raw_op_cpu(native):
    """tb_step(rmap=) on a middle slab: rows 40..110 of a 150-row grid, 8 fused levels = 8 golden steps."""
    _raw_op("cpu", "fp64", 8)


def _raw_op(device, dtype, k, n=150, ncols=261, row0=40, nrows=70, arith="exact"):
    import torch

    from heat2d.ops import kernels as K
    dt = NP[dtype]
    rng = np.random.default_rng(7)
    T0 = (10.0 ** rng.uniform(-1, 1, (n + 2, ncols + 2))).astype(dt)
    M = rng.uniform(0.01, 0.25, T0.shape)
    M[1:-1, 1:-1][rng.uniform(size=(n, ncols)) < 0.03] = 0.0
    M = M.astype(dt)
    L = K.make_layout(nrows, ncols, halo=24, row0=row0, nrows_global=n)
    host = np.full((L.rows_alloc(), L.pitch), 3.25, dtype=dt)  # (pad columns: finite, pinned)
    g0 = row0 - L.halo
    host[:, L.cpad - 1:L.cpad + ncols + 1] = T0[g0 + 1:g0 + 1 + L.rows_alloc()]
    src = torch.from_numpy(host.reshape(-1).copy()).to(device)
    dst = torch.full_like(src, float("nan"))  # NaN guard bands around the rows written
    q = K.rmap_field(M, L, src.dtype, device)
    K.tb_step(src, dst, L, k, 0.0, arith=arith, rmap=q)
    out = K.view2d(dst.cpu(), L).numpy().copy()
    T = T0.copy()
    for _ in range(k):
        T = R.ftcs_step(T, 0.0, arith, rmap=M)
    own = out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols].copy()
    assert np.array_equal(own, T[row0 + 1:row0 + 1 + nrows, 1:-1])
    # The only writes allowed outside the output rectangle (as tests/test_ops.py run_guard): the
    # device kernel's last 16-B vector of a row may cover the right frame column / pad of the
    # SAME rows, written back with src's pinned values — the map is 0 there.
    out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols] = np.nan
    rr, cc = np.nonzero(~np.isnan(out))
    assert ((rr >= L.halo) & (rr < L.halo + nrows)).all(), "kernel wrote outside its output rows"
    assert (cc >= L.cpad + ncols).all() and (cc < L.cpad + ncols + 8).all(), "kernel wrote beyond one vector of right pad"
    assert np.array_equal(out[rr, cc], host[rr, cc]), "frame / pad write changed a value"
    return own


def test_memory_planner_counts_the_map(native):
    for dtype, es in (("fp32", 4), ("fp64", 8)):
        for nranks in (1, 3):
            a = heat2d.footprint(1000, nranks, dtype)
            b = heat2d.footprint(1000, nranks, dtype, rmap=True)
            one = a["field_bytes"] // 2
            assert a["field_bytes"] == 2 * one and b["field_bytes"] == 3 * one
            assert b["total_bytes"] - a["total_bytes"] == one and b["work_bytes"] == a["work_bytes"]
            rows = N.decompose(1000, nranks, 0)[1]
            L = N.make_layout(rows, 1000, 24, 0, 1000)
            assert one == L.elems() * es
    budget = 8 << 30
    with_map = heat2d.plan_max_grid("fp64", 1, free_bytes=budget, reserve=0, rmap=True)["n"]
    without = heat2d.plan_max_grid("fp64", 1, free_bytes=budget, reserve=0)["n"]
    assert with_map < without
    assert with_map == heat2d.plan_max_grid("fp64", 1, free_bytes=budget, reserve=0, source=True)["n"]
    assert heat2d.footprint(with_map, 1, "fp64", rmap=True)["total_bytes"] <= budget
    assert heat2d.footprint(with_map + 1, 1, "fp64", rmap=True)["total_bytes"] > budget


def test_rmap_from_nu():
    p = problem(40, 1)
    nu = np.random.default_rng(3).uniform(0.0, 2.0 * p.nu, (42, 42)).astype(np.float32)
    M = heat2d.rmap_from_nu(p, nu)
    assert M.dtype == np.float64 and M.shape == (42, 42)
    assert np.array_equal(M, np.float64(p.r) * nu.astype(np.float64) / np.float64(p.nu))
    assert np.array_equal(heat2d.rmap_from_nu(p, np.full((42, 42), p.nu)), np.full((42, 42), np.float64(p.r) * p.nu / p.nu))


# ------------------------------------------------------------------ CPU: checkpoints and the drivers

def test_checkpoint_restart_other_rank_count(native, tmp_path):
    """A checkpoint with a map as 2 ranks write it (two rank files, 39 + 38 rows, and the
    meta.json save() writes), resumed on 1 rank; without a map meta.json keeps its key set."""
    from heat2d.utils import checkpoint
    n, p = 77, problem(77, 20)
    M = rough_map(n, "fp64")
    T0 = R.initial_field(p)  # (a checkpoint holds the owned points; the frame is the problem's)
    T0[1:-1, 1:-1] = R.owned(rough_field(n, "fp64"))
    s = HeatSolver(p, backend="cpu", tb=4, arith="exact", rmap=M)
    s.upload(T0)
    s.step(9)
    mid = s.download()
    checkpoint.save(s, str(tmp_path / "ck1"), step=9)
    sha = s.rmap_sha256
    s.close()
    meta = json.loads(open(os.path.join(checkpoint.resolve(str(tmp_path / "ck1")), "meta.json")).read())
    assert meta["rmap_sha256"] == sha == hashlib.sha256(M.tobytes()).hexdigest()
    sd = checkpoint.step_dir(str(tmp_path / "ck"), 9)
    os.makedirs(sd)
    r1 = N.decompose(n, 2, 1)[0]
    np.save(os.path.join(sd, "rank00000.npy"), mid[:r1])
    np.save(os.path.join(sd, "rank00001.npy"), mid[r1:])
    meta["nranks"] = 2
    with open(os.path.join(sd, "meta.json"), "w") as f:
        json.dump(meta, f)
    # restart with the same map on one rank: bitwise the uninterrupted run
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", rmap=M)
    assert checkpoint.load(r, sd)["step"] == 9
    r.step(11)
    assert np.array_equal(r.download(), R.owned(R.ftcs(p, 20, T0=T0, rmap=M)))
    r.close()
    # without the map, and with another one: refused before the first step
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact")
    with pytest.raises(ValueError, match="with a diffusivity map"):
        checkpoint.load(r, sd)
    checkpoint.save(r, str(tmp_path / "ck0"), step=0)
    assert "rmap_sha256" not in json.loads(open(os.path.join(checkpoint.resolve(str(tmp_path / "ck0")), "meta.json")).read())
    r.close()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", rmap=rough_map(n, "fp64", seed=2))
    with pytest.raises(ValueError, match="differs from the checkpoint"):
        checkpoint.load(r, sd)
    r.close()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", rmap=M)  # a checkpoint without a map
    del meta["rmap_sha256"]
    with open(os.path.join(sd, "meta.json"), "w") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError, match="without a diffusivity map"):
        checkpoint.load(r, sd)
    r.close()


def py(cwd, *args):
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2")
    return subprocess.run([sys.executable, "-m", "heat2d", *args], cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=300)


def test_python_driver_rmap(native, tmp_path):
    """--rmap through python -m heat2d on the CPU backend: the golden's field (auto is exact); the
    checkpoint records the digest; a restart without the file and a wrong-shape file fail; the
    r > 1/4 warning fires on max(R)."""
    n = 50
    (tmp_path / "input.dat").write_text(f"{n} 0.25 0.05 1.0 30 1\n")
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    M = rough_map(n, "fp64")
    np.save(tmp_path / "map.npy", M)
    np.save(tmp_path / "bad.npy", M[:, 1:])
    args = ["--backend", "cpu", "--ic", "hat-cuda", "--quiet", "--output", "npy"]
    out = py(tmp_path, *args, "--rmap", "map.npy", "--ntime", "12", "--checkpoint", "ck")
    assert out.returncode == 0, out.stdout + out.stderr
    assert "unstable" not in out.stderr
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    assert meta["rmap_sha256"] == hashlib.sha256(M.tobytes()).hexdigest() and meta["step"] == 12
    bad = py(tmp_path, *args, "--restart", "ck")
    assert bad.returncode != 0 and "diffusivity map" in bad.stdout + bad.stderr
    out = py(tmp_path, *args, "--rmap", "map.npy", "--restart", "ck")
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.load(tmp_path / "soln00000.npy")
    assert np.array_equal(got, R.owned(R.ftcs(prob, 30, arith="exact", rmap=M)))
    bad = py(tmp_path, *args, "--rmap", "bad.npy")
    assert bad.returncode != 0 and "shape" in bad.stdout + bad.stderr
    Mw = M.copy()
    Mw[5, 5] = 0.3
    np.save(tmp_path / "hot.npy", Mw)
    out = py(tmp_path, *args, "--rmap", "hot.npy", "--ntime", "2")
    assert out.returncode == 0 and "max r = 0.3 > 0.25" in out.stderr, out.stdout + out.stderr


def test_native_cli_rmap(native, tmp_path):
    """--rmap through the native CLI on the CPU backend: auto is exact (not jacobi) at r = 1/4, the
    checkpoint records the digest of the converted array, the Python driver resumes it with the
    same file, a restart without the file, with another file and a wrong-shape file fail."""
    from heat2d.utils import io
    n = 64
    (tmp_path / "input.dat").write_text(f"{n} 0.25 0.05 1.0 30 1\n")
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "uniform")
    assert prob.r == 0.25 and prob.ic.sterbenz_safe()  # where auto without a map is jacobi
    M = rough_map(n, "fp64")
    np.save(tmp_path / "map.npy", M)
    np.save(tmp_path / "bad.npy", M[:, 1:])
    cli = [N.CLI_PATH, "--cpu", "--quiet", "--ic", "uniform"]

    def run_cli(*args):
        return subprocess.run([*cli, *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)

    out = run_cli("--rmap", "map.npy", "--ntime", "12", "--checkpoint", "ck", "--output", "none", "--json", "w.json")
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads((tmp_path / "w.json").read_text())["arith_used"] == "exact (auto)"
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    assert meta["rmap_sha256"] == hashlib.sha256(M.tobytes()).hexdigest() and meta["step"] == 12
    bad = run_cli("--restart", "ck")
    assert bad.returncode != 0 and "diffusivity map" in bad.stdout + bad.stderr
    np.save(tmp_path / "other.npy", rough_map(n, "fp64", seed=2))
    bad = run_cli("--restart", "ck", "--rmap", "other.npy")
    assert bad.returncode != 0 and "differs from the checkpoint" in bad.stdout + bad.stderr
    gold30 = R.owned(R.ftcs(prob, 30, arith="exact", rmap=M))
    out = run_cli("--restart", "ck", "--rmap", "map.npy")
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(io.read_xyz(str(tmp_path / "soln00000.dat"))[2], gold30)
    out = run_cli("--restart", "ck", "--rmap", "map.npy", "--gpus", "3", "--output", "npy")  # 3 ranks resume it too
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.concatenate([np.load(tmp_path / f"soln{r:05d}.npy") for r in range(3)], axis=0)
    assert np.array_equal(got, gold30)
    # the other driver resumes it, given the same file; and refuses it without
    out = py(tmp_path, "--backend", "cpu", "--ic", "uniform", "--quiet", "--output", "npy", "--rmap", "map.npy",
             "--restart", "ck")
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.load(tmp_path / "soln00000.npy"), gold30)
    bad = py(tmp_path, "--backend", "cpu", "--ic", "uniform", "--quiet", "--output", "npy", "--restart", "ck")
    assert bad.returncode != 0 and "diffusivity map" in bad.stdout + bad.stderr
    bad = run_cli("--rmap", "bad.npy")
    assert bad.returncode != 0 and "shape" in bad.stdout + bad.stderr
    # an f8 file in an fp32 run: converted, and the digest is the converted array's
    out = run_cli("--dtype", "fp32", "--rmap", "map.npy", "--ntime", "5", "--checkpoint", "ck32", "--output", "none")
    assert out.returncode == 0, out.stdout + out.stderr
    with open(tmp_path / "ck32" / "latest") as f:
        meta = json.loads((tmp_path / "ck32" / f.read().strip() / "meta.json").read_text())
    assert meta["rmap_sha256"] == hashlib.sha256(M.astype(np.float32).tobytes()).hexdigest()
    # without a map the CLI's auto still picks jacobi on this IC, and meta.json has no map key
    out = run_cli("--ntime", "3", "--checkpoint", "ck0", "--output", "none", "--json", "n.json")
    assert out.returncode == 0 and json.loads((tmp_path / "n.json").read_text())["arith_used"] == "jacobi (auto)"
    with open(tmp_path / "ck0" / "latest") as f:
        assert "rmap_sha256" not in json.loads((tmp_path / "ck0" / f.read().strip() / "meta.json").read_text())


# ------------------------------------------------------------------ GPU

def _depths():
    return [1, 2, 7, 8, 13, "D"]


@pytest.mark.gpu
@pytest.mark.parametrize("tb", _depths())
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_one_strip(native, gpu, dtype, arith, tb):
    """n = 77: one strip; 2 * tb + 3 steps: two full passes and a shallower one
    (step(tb), step(tb), step(3): one step(2 tb + 3) call runs none of depth tb)."""
    if tb == 13 and depth_max() < 13:
        tb = "D"  # (13 only if <= D: the deepest pass then runs twice)
    tb = depth(tb)
    steps = 2 * tb + 3
    got = run(77, dtype, "hip", tb, steps, arith, full=2)
    assert np.array_equal(got, gold(77, dtype, steps, arith))


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [8, "D"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_several_strips(native, gpu, dtype, tb):
    """n = 301, 37 steps: several strips, passes of different depth mix."""
    tb = depth(tb)
    for arith in ("exact", "fma"):
        got = run(301, dtype, "hip", tb, 37, arith, prepare=True)
        assert np.array_equal(got, gold(301, dtype, 37, arith)), arith


def worker(tmp_path, a, **env):
    out = subprocess.run([sys.executable, os.path.join(HERE, "rmap_worker.py"), str(tmp_path), json.dumps(a)],
                         env=dict(os.environ, HEAT2D_PLAN_CACHE="off", **env), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    return json.loads((tmp_path / "info.json").read_text()), np.load(tmp_path / "result.npy")


@pytest.mark.gpu
@pytest.mark.parametrize("env", [{}, {"HEAT2D_SPLIT_ORDER": "single"}, {"HEAT2D_DYNAMIC": "1", "HEAT2D_MAX_WAVES": "40"},
                                 {"HEAT2D_PIPE": "1"}], ids=["split", "single", "dynamic", "pipe"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_split_plans(native, gpu, tmp_path, dtype, env):
    """301 rows x 2897 columns (rows=): the boundary bands and the interior of a split plan, a
    forced single launch, the dynamic item queue, and HEAT2D_PIPE=1 (no wave-pair kernel with a
    map: one-wave strips) — every launch on the map kernel."""
    tb = depth_max() if "HEAT2D_PIPE" in env else 8
    a = {"n": 2897, "rows": 301, "steps": 37, "tb": tb, "dtype": dtype, "sigma": 0.2, "arith": "exact"}
    a["calls"] = Y.calls(tb, 37, 2)  # two cycles of depth tb (the queue's reset between them), then the rest
    info, got = worker(tmp_path, a, **env)
    plan = info["plan"]
    Y.assert_ran(info["cycle_hist"], tb, 2)  # the plan asserted on is the one that ran
    print(f"{dtype} {env}: plan {plan}")
    if "HEAT2D_SPLIT_ORDER" in env:
        assert plan["valid"] == 2
    else:  # a split plan: boundary bands and interior
        assert plan["valid"] in (1, 3) and plan["edge_items"] > 0
    if "HEAT2D_DYNAMIC" in env:  # the queue is used: a dynamic plan with more items than waves
        assert plan["dynamic"] == 1 and plan["main_waves"] == 40 and plan["main_items"] > plan["main_waves"]
    else:
        assert plan["dynamic"] == 0
    # never the wave-pair kernel, HEAT2D_PIPE=1 included: one-wave strips (64 lanes x 16 B)
    assert plan["pipe"] == 0 and plan["main_strip_w"] == (128 if dtype == "fp64" else 256)
    assert info["info"]["tb"] == tb and info["info"]["rmap"]["set"] and info["info"]["arith"] == N.ARITH["exact"]
    assert np.array_equal(got, gold(2897, dtype, 37, "exact", rows=301))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_graph_replay(native, gpu, dtype):
    """graph=True, step(37) twice."""
    p = problem(301, 74)
    s = HeatSolver(p, dtype=dtype, backend="hip", tb=8, arith="exact", device=0, graph=True, rmap=rough_map(301, dtype))
    s.upload(rough_field(301, dtype))
    s.prepare(37)
    s.step(37)
    s.step(37)
    got = s.download()
    s.close()
    assert np.array_equal(got, gold(301, dtype, 74))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_loopback_three_ranks(native, gpu, dtype):
    """n = 301 on 3 loopback ranks (101 / 100 / 100 rows)."""
    p = problem(301, 37)
    g = LoopbackGroup(p, 3, dtype=dtype, backend="hip", tb=8, arith="exact", device=0, rmap=rough_map(301, dtype))
    assert [r for _, r in g.slabs()] == [101, 100, 100]
    g.upload(rough_field(301, dtype))
    g.step(37)
    got = g.download()
    g.close()
    assert np.array_equal(got, gold(301, dtype, 37))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_raw_op(native, gpu, dtype):
    """tb_step(rmap=) on a middle slab; NaN guard bands around the rows written: the new kernel
    writes nothing outside its rects."""
    for k, arith in ((8, "exact"), (depth_max(), "fma")):
        _raw_op("cuda", dtype, k, arith=arith)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_fresh_map_and_none(native, gpu, dtype):
    n, dt, p = 301, NP[dtype], problem(301, 37)
    T0, M1, M2 = rough_field(n, dtype), rough_map(n, dtype), rough_map(n, dtype, seed=2)
    s = HeatSolver(p, dtype=dtype, backend="hip", tb=8, arith="exact", device=0, rmap=M1)
    s.upload(T0)
    s.step(20)
    s.set_rmap(M2)
    s.step(17)
    got = s.download()
    mid = R.ftcs(p, 20, dtype=dt, T0=T0, rmap=M1)
    assert np.array_equal(got, R.owned(R.ftcs(p, 17, dtype=dt, T0=mid, rmap=M2)))
    s.set_rmap(None)
    s.upload(T0)
    s.step(37)
    assert np.array_equal(s.download(), R.owned(R.ftcs(p, 37, dtype=dt, T0=T0)))
    s.close()


@pytest.mark.gpu
def test_hip_depth_clamp_and_refusals(native, gpu):
    M = rough_map(301, "fp64")
    s = HeatSolver(problem(301, 4), backend="hip", device=0, tb=24, rmap=M)
    info = s.info()
    s.close()
    assert info["tb"] == depth_max() and info["rmap"]["max_tb"] == depth_max()
    for kw, why in ((dict(arith="jacobi"), "jacobi"), (dict(engine="jit"), "jit"), (dict(copy_swap=True), "copy-swap"),
                    (dict(bc_y="insulated"), "Dirichlet"), (dict(source=np.zeros_like(M)), "heat source")):
        with pytest.raises(RuntimeError, match=why):
            HeatSolver(problem(301, 4, 0.25), backend="hip", device=0, rmap=M, **kw)
