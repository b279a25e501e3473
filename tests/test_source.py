"""Volumetric heat source, u_t = nu lap(u) + f: the per-step increment S = dt * f
enters every fused level of the march as one separately rounded add,

    exact: T' = (C + r*((((S_+E)+N)+W) - 4C)) + S[i,j]
    fma:   T' = fma(r, fma(-4, C, sum), C)    + S[i,j]

bitwise against the NumPy golden (models.reference.ftcs(source=)) at every pass
depth, launch plan and rank count, on the CPU twin and on the HIP engine
(tb_kernel_src, csrc/kernels/tb_impl.hpp).

Data (fixed seeds): field values 10**uniform(-1, 1), frame included; source
values of both signs with magnitudes 10**uniform(-3, -1) times the field value
at the same point. r = 0.2 (r * x rounds) and 0.25 (r * x exact).

Negative controls of the data come first: adding the source once per pass, a
source shifted by one row, and the source folded into the centre before the
update all give other bits than the golden, so only an engine that adds the
right row at every level, after the update, can pass the bitwise tests.

Closed form: T_0 = 0, zero frame, S = a * mode with mode = sin(pi i / (n + 1))
sin(pi j / (n + 1)) an eigenvector of the update with factor lambda = 1 - 4r +
2r (cos(pi / (n + 1)) + cos(pi / (n + 1))), so T_m = a (1 - lambda^m) / (1 -
lambda) * mode. A step makes a handful of roundings on values <= max|T_m| and
the update is non-expansive in the max norm (r <= 1/4), so the golden is held
to m * eps * max|T_m|; it sits at 0.01-0.15 of that bound.
"""
import dataclasses
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
from source_worker import problem, rough_field, rough_source  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
SIGMAS = [0.2, 0.25]
_DEPTH = []


def depth_max():
    """The source kernels' deepest pass (common.hpp kMaxTBSrc), as the library reports it
    (tests/test_source_isa.py holds it against the instances in the code objects)."""
    if not _DEPTH:
        s = HeatSolver(problem(8, 1), backend="cpu", source=np.zeros((10, 10)))
        _DEPTH.append(s.info()["source"]["max_tb"])
        s.close()
    return _DEPTH[0]


def depth(tb):
    return depth_max() if tb == "D" else tb

_GOLD = {}


def gold(n, dtype, steps, sigma=0.2, arith="exact", rows=None, seed=1, framed=False):
    """The golden run (computed once, read-only). rows: the first rows x n of the grid."""
    key = (n, dtype, steps, sigma, arith, rows, seed)
    if key not in _GOLD:
        T0, S = rough_field(n, dtype, rows=rows), rough_source(n, dtype, rows=rows, seed=seed)
        g = np.ascontiguousarray(R.ftcs(problem(n, steps, sigma), steps, dtype=NP[dtype], T0=T0, arith=arith, source=S))
        g.setflags(write=False)
        _GOLD[key] = g
    return _GOLD[key] if framed else R.owned(_GOLD[key])


def run(n, dtype, backend, tb, steps, sigma=0.2, arith="exact", ranks=1, rows=None, prepare=False, source="rough", full=0, **kw):
    """full > 0: the steps as tests/cycles.py calls(tb, steps, full) — `full`
    cycles of depth tb, asserted from cycle_hist(), then the remainder — and
    not as one step() call, whose balanced cycles are all shallower than tb."""
    p = problem(n, steps, sigma)
    T0 = rough_field(n, dtype, rows=rows)
    S = rough_source(n, dtype, rows=rows) if isinstance(source, str) else source
    dev = dict(device=0) if backend == "hip" else {}
    if ranks > 1:
        s = LoopbackGroup(p, ranks, dtype=dtype, backend=backend, tb=tb, arith=arith, source=S, **dev, **kw)
        s.upload(T0)
        s.step(steps)
        out = s.download()
        s.close()
        assert not full
        return out
    s = HeatSolver(p, dtype=dtype, backend=backend, tb=tb, arith=arith, source=S, rows=rows, **dev, **kw)
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
    """ftcs / ftcs_step with source=None are today's functions, bit for bit."""
    T0 = rough_field(77, dtype)
    p = problem(77, 8, 0.2)
    dt, r, four = NP[dtype], NP[dtype](p.r), NP[dtype](4)
    T = T0.copy()
    for _ in range(8):
        c = T[1:-1, 1:-1]
        Q = T.copy()
        Q[1:-1, 1:-1] = c + r * ((((T[2:, 1:-1] + T[1:-1, 2:]) + T[:-2, 1:-1]) + T[1:-1, :-2]) - four * c)
        T = Q
    assert np.array_equal(R.ftcs(p, 8, dtype=dt, T0=T0), T)
    assert np.array_equal(R.ftcs(p, 8, dtype=dt, T0=T0, source=None), T)
    assert np.array_equal(R.ftcs_step(T0, p.r, source=None), R.ftcs_step(T0, p.r))
    for arith in ("fma", "jacobi"):
        q = problem(77, 3, 0.25)
        assert np.array_equal(R.ftcs(q, 3, dtype=dt, T0=T0, arith=arith, source=None), R.ftcs(q, 3, dtype=dt, T0=T0, arith=arith))
    # a zero source of the right sign changes nothing either (x + -0.0 == x bit for bit)
    assert np.array_equal(R.ftcs(p, 8, dtype=dt, T0=T0, source=np.full_like(T0, -0.0)), T)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_fma_is_one_rounding(dtype):
    """reference.fma against libm's fma / fmaf on data with cancellation."""
    import ctypes
    import ctypes.util
    m = ctypes.CDLL(ctypes.util.find_library("m"))
    f = m.fma if dtype == "fp64" else m.fmaf
    ct = ctypes.c_double if dtype == "fp64" else ctypes.c_float
    f.restype, f.argtypes = ct, [ct] * 3
    rng = np.random.default_rng(5)
    n, dt = 20000, NP[dtype]
    a = (rng.standard_normal(n) * 10 ** rng.uniform(-2, 2, n)).astype(dt)
    b = rng.standard_normal(n).astype(dt)
    c = (-(a.astype(np.float64) * b) * (1 + rng.standard_normal(n) * 10 ** rng.uniform(-9, 0, n))).astype(dt)
    c[::3] = rng.standard_normal(len(c[::3])).astype(dt)
    want = np.array([f(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())], dtype=dt)
    assert np.array_equal(R.fma(a, b, c), want)
    assert np.mean(want != a * b + c) > 0.2  # the data tells one rounding from two


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_negative_controls(dtype, sigma):
    """n = 77, 8 steps: three wrong ways to add the source, each against 8 golden steps."""
    n, K, dt = 77, 8, NP[dtype]
    p = problem(n, K, sigma)
    T0, S = rough_field(n, dtype), rough_source(n, dtype)
    g = gold(n, dtype, K, sigma)
    # the source added once per pass: 8 plain steps, then K * S
    once = R.owned(R.ftcs(p, K, dtype=dt, T0=T0)) + dt(K) * R.owned(S)
    d_once = np.mean(once != g)
    # the source shifted by one row
    Sh = S.copy()
    Sh[1:-1] = np.roll(S[1:-1], 1, axis=0)
    d_shift = np.mean(R.owned(R.ftcs(p, K, dtype=dt, T0=T0, source=Sh)) != g)
    # the source folded into the centre first: (C + S) + r * (...)
    r, four = dt(p.r), dt(4)
    T = T0.copy()
    for _ in range(K):
        c = T[1:-1, 1:-1]
        Q = T.copy()
        Q[1:-1, 1:-1] = (c + S[1:-1, 1:-1]) + r * ((((T[2:, 1:-1] + T[1:-1, 2:]) + T[:-2, 1:-1]) + T[1:-1, :-2]) - four * c)
        T = Q
    d_order = np.mean(R.owned(T) != g)
    print(f"{dtype} r = {sigma}: once per pass differs at {100 * d_once:.1f} %, shifted by a row {100 * d_shift:.1f} %, "
          f"(C + S) first {100 * d_order:.1f} % of the points")
    assert d_once > 0.9 and d_shift > 0.9 and d_order > 0.1


@pytest.mark.parametrize("steps", [50, 400])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_closed_form(dtype, steps):
    n, r, a, dt = 64, 0.2, 0.37, NP[dtype]
    i = np.arange(n + 2)
    mode = np.sin(np.pi * i / (n + 1))[:, None] * np.sin(np.pi * i / (n + 1))[None, :]
    mode[0] = mode[-1] = 0.0
    mode[:, 0] = mode[:, -1] = 0.0
    lam = 1.0 - 4.0 * r + 4.0 * r * np.cos(np.pi / (n + 1))
    want = a * (1.0 - lam ** steps) / (1.0 - lam) * mode
    T = R.ftcs(problem(n, steps, r), steps, dtype=dt, T0=np.zeros((n + 2, n + 2), dt), source=(a * mode).astype(dt))
    err, bound = np.abs(T.astype(np.float64) - want).max(), steps * np.finfo(dt).eps * np.abs(want).max()
    print(f"{dtype} {steps} steps: |golden - closed form| = {err:.3e} = {err / bound:.3f} of the bound {bound:.3e}")
    assert err <= bound


# ------------------------------------------------------------------ CPU twin

@pytest.mark.parametrize("tb", [1, 2, 7, 8])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_twin_bitwise(native, dtype, arith, sigma, tb):
    for n, steps in ((77, 8), (301, 11)):
        got = run(n, dtype, "cpu", tb, steps, sigma, arith)
        assert np.array_equal(got, gold(n, dtype, steps, sigma, arith)), n


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_loopback_uneven_slabs(native, dtype):
    """3 ranks on 77 rows (26 / 26 / 25): every member slices its rows of the global source."""
    for arith in ("exact", "fma"):
        got = run(77, dtype, "cpu", 7, 23, 0.2, arith, ranks=3)
        assert np.array_equal(got, gold(77, dtype, 23, 0.2, arith)), arith


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_pinned_negative_zero_survives(native, dtype):
    """A frame row of -0.0 stays -0.0 although the source array has nonzero frame entries."""
    n, dt = 40, NP[dtype]
    T0, S = rough_field(n, dtype), rough_source(n, dtype)
    T0[0, :] = dt(-0.0)
    T0[-1, 5:9] = dt(-0.0)
    assert (S[0] != 0).all() and (S[:, 0] != 0).all()
    s = HeatSolver(problem(n, 9), dtype=dtype, backend="cpu", tb=4, arith="exact", source=S)
    s.upload(T0)
    s.step(9)
    F = s.download_field()
    s.close()
    assert np.signbit(F[0]).all() and (F[0] == 0).all() and np.signbit(F[-1, 5:9]).all()
    assert np.array_equal(F, R.ftcs(problem(n, 9), 9, dtype=dt, T0=T0, source=S))


def test_refusals(native):
    p, S = problem(40, 4, 0.25), rough_source(40, "fp64")
    for kw, why in ((dict(arith="jacobi"), "jacobi"), (dict(arith="fast"), "fast"), (dict(bc_x="periodic"), "Dirichlet"),
                    (dict(bc_y="periodic"), "Dirichlet"), (dict(bc_x="insulated"), "Dirichlet"),
                    (dict(bc_y="insulated"), "Dirichlet"), (dict(copy_swap=True), "copy-swap")):
        with pytest.raises(RuntimeError, match=why):
            HeatSolver(p, backend="cpu", source=S, **kw)
    with pytest.raises(RuntimeError, match="jit|HIP"):
        HeatSolver(p, backend="cpu", engine="jit", source=S)
    with pytest.raises(ValueError, match="frame-inclusive"):
        HeatSolver(p, backend="cpu", source=S[1:])
    s = HeatSolver(p, backend="cpu")  # built without a source: none can be set later
    with pytest.raises(RuntimeError, match="without a heat source"):
        s.set_source(S)
    s.close()
    with pytest.raises(ValueError, match="exact"):
        R.ftcs(p, 2, T0=rough_field(40, "fp64"), arith="jacobi", source=S)
    with pytest.raises(ValueError, match="Dirichlet"):
        R.ftcs(p, 2, T0=rough_field(40, "fp64"), bc_x="periodic", source=S)


def test_auto_resolves_to_fma_not_jacobi(native):
    """r = 1/4 on the reference IC (where the drivers' auto picks jacobi without a source)."""
    inp = heat2d.parse_input_text("64 0.25 0.05 1.0 6 0")
    p = heat2d.make_problem(inp, "ghost", "uniform")
    S = rough_source(p.n_owned, "fp64")
    s = HeatSolver(p, backend="cpu", arith="auto", source=S)
    info = s.info()
    s.step(6)
    got = s.download()
    s.close()
    assert info["arith"] == N.ARITH["fma"]
    assert info["source"] == {"enabled": True, "set": True, "max_tb": depth_max()} and depth_max() >= 16
    assert np.array_equal(got, R.owned(R.ftcs(p, 6, arith="fma", source=S)))
    s = HeatSolver(problem(64, 6, 0.2), backend="cpu", arith="auto", source=S)
    assert s.info()["arith"] == N.ARITH["exact"]
    s.close()
    g = LoopbackGroup(p, 2, backend="cpu", arith="auto", source=S)
    assert g.arith_code(0) == N.ARITH["fma"] and g.arith_code(1) == N.ARITH["fma"]
    g.close()
    s = HeatSolver(p, backend="cpu")
    assert s.info()["source"] == {"enabled": False, "set": False, "max_tb": 0}
    s.close()


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_set_source_none_and_fresh(native, dtype):
    """set_source(None): the run equals the no-source run; a fresh array between
    two step() calls: the golden run the same way."""
    n, dt, p = 77, NP[dtype], problem(77, 20)
    T0, S1, S2 = rough_field(n, dtype), rough_source(n, dtype), rough_source(n, dtype, seed=2)
    s = HeatSolver(p, dtype=dtype, backend="cpu", tb=7, arith="exact", source=S1)
    s.set_source(None)
    assert s.info()["source"]["set"] is False
    s.upload(T0)
    s.step(20)
    assert np.array_equal(s.download(), R.owned(R.ftcs(p, 20, dtype=dt, T0=T0)))
    s.upload(T0)
    s.set_source(S1)
    s.step(9)
    s.set_source(S2)
    s.step(11)
    got = s.download()
    s.close()
    mid = R.ftcs(p, 9, dtype=dt, T0=T0, source=S1)
    assert np.array_equal(got, R.owned(R.ftcs(p, 11, dtype=dt, T0=mid, source=S2)))


def test_step_stats_takes_the_unfused_path(native):
    p, S = problem(77, 12), rough_source(77, "fp64")
    s = HeatSolver(p, backend="cpu", tb=5, arith="exact", source=S)
    s.upload(rough_field(77, "fp64"))
    st = s.step_stats(12)
    got = s.download()
    s.close()
    g = gold(77, "fp64", 12).astype(np.float64)
    assert np.array_equal(got, g) and st["min"] == g.min() and st["max"] == g.max()


def test_raw_op_cpu(native):
    """tb_step(source=) on a middle slab: rows 40..110 of a 150-row grid, 8 fused levels = 8 golden steps."""
    _raw_op("cpu", "fp64", 8)


def _raw_op(device, dtype, k, n=150, ncols=261, row0=40, nrows=70, sigma=0.2, arith="exact"):
    import torch

    from heat2d.ops import kernels as K
    dt = NP[dtype]
    rng = np.random.default_rng(7)
    T0 = (10.0 ** rng.uniform(-1, 1, (n + 2, ncols + 2))).astype(dt)
    S = (T0 * 10.0 ** rng.uniform(-3, -1, T0.shape) * rng.choice([-1.0, 1.0], T0.shape)).astype(dt)
    L = K.make_layout(nrows, ncols, halo=24, row0=row0, nrows_global=n)
    host = np.full((L.rows_alloc(), L.pitch), 3.25, dtype=dt)  # (pad columns: finite, pinned)
    g0 = row0 - L.halo
    host[:, L.cpad - 1:L.cpad + ncols + 1] = T0[g0 + 1:g0 + 1 + L.rows_alloc()]
    src = torch.from_numpy(host.reshape(-1).copy()).to(device)
    dst = torch.full_like(src, float("nan"))  # NaN guard bands around the rows written
    q = K.source_field(S, L, src.dtype, device)
    K.tb_step(src, dst, L, k, sigma, arith=arith, source=q)
    out = K.view2d(dst.cpu(), L).numpy().copy()
    T = T0.copy()
    for _ in range(k):
        T = R.ftcs_step(T, dt(sigma), arith, source=S)
    own = out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols].copy()
    assert np.array_equal(own, T[row0 + 1:row0 + 1 + nrows, 1:-1])
    # The only writes allowed outside the output rectangle (as tests/test_ops.py run_guard): the
    # device kernel's last 16-B vector of a row may cover the right frame column / pad of the
    # SAME rows, written back with src's pinned values — the source adds -0.0 there.
    out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols] = np.nan
    rr, cc = np.nonzero(~np.isnan(out))
    assert ((rr >= L.halo) & (rr < L.halo + nrows)).all(), "kernel wrote outside its output rows"
    assert (cc >= L.cpad + ncols).all() and (cc < L.cpad + ncols + 8).all(), "kernel wrote beyond one vector of right pad"
    assert np.array_equal(out[rr, cc], host[rr, cc]), "frame / pad write changed a value"
    return own


def test_memory_planner_counts_the_source(native):
    for dtype, es in (("fp32", 4), ("fp64", 8)):
        for nranks in (1, 3):
            a = heat2d.footprint(1000, nranks, dtype, source=False)
            b = heat2d.footprint(1000, nranks, dtype, source=True)
            one = a["field_bytes"] // 2
            assert a["field_bytes"] == 2 * one and b["field_bytes"] == 3 * one
            assert b["total_bytes"] - a["total_bytes"] == one and b["work_bytes"] == a["work_bytes"]
            rows = N.decompose(1000, nranks, 0)[1]
            L = N.make_layout(rows, 1000, 24, 0, 1000)
            assert one == L.elems() * es
    budget = 8 << 30
    with_src = heat2d.plan_max_grid("fp64", 1, free_bytes=budget, reserve=0, source=True)["n"]
    without = heat2d.plan_max_grid("fp64", 1, free_bytes=budget, reserve=0)["n"]
    assert with_src < without
    assert heat2d.footprint(with_src, 1, "fp64", source=True)["total_bytes"] <= budget
    assert heat2d.footprint(with_src + 1, 1, "fp64", source=True)["total_bytes"] > budget


# ------------------------------------------------------------------ CPU: checkpoints and the Python driver

def test_checkpoint_restart_other_rank_count(native, tmp_path):
    """A checkpoint with a source as 2 ranks write it (two rank files, 39 + 38 rows, and the
    meta.json save() writes), resumed on 1 rank."""
    import hashlib

    from heat2d.utils import checkpoint
    n, p = 77, problem(77, 20)
    S = rough_source(n, "fp64")
    T0 = R.initial_field(p)  # (a checkpoint holds the owned points; the frame is the problem's)
    T0[1:-1, 1:-1] = R.owned(rough_field(n, "fp64"))
    s = HeatSolver(p, backend="cpu", tb=4, arith="exact", source=S)
    s.upload(T0)
    s.step(9)
    mid = s.download()
    checkpoint.save(s, str(tmp_path / "ck1"), step=9)
    sha = s.source_sha256
    s.close()
    meta = json.loads(open(os.path.join(checkpoint.resolve(str(tmp_path / "ck1")), "meta.json")).read())
    assert meta["source_sha256"] == sha == hashlib.sha256(S.tobytes()).hexdigest()
    sd = checkpoint.step_dir(str(tmp_path / "ck"), 9)
    os.makedirs(sd)
    r1 = N.decompose(n, 2, 1)[0]
    np.save(os.path.join(sd, "rank00000.npy"), mid[:r1])
    np.save(os.path.join(sd, "rank00001.npy"), mid[r1:])
    meta["nranks"] = 2
    with open(os.path.join(sd, "meta.json"), "w") as f:
        json.dump(meta, f)
    # restart with the same source on one rank: bitwise the uninterrupted run
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", source=S)
    assert checkpoint.load(r, sd)["step"] == 9
    r.step(11)
    assert np.array_equal(r.download(), R.owned(R.ftcs(p, 20, T0=T0, source=S)))
    r.close()
    # without the source, and with another one: refused before the first step
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact")
    with pytest.raises(ValueError, match="with a heat source"):
        checkpoint.load(r, sd)
    r.close()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", source=rough_source(n, "fp64", seed=2))
    with pytest.raises(ValueError, match="differs from the checkpoint"):
        checkpoint.load(r, sd)
    r.close()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", source=S)  # a checkpoint without a source
    meta["source_sha256"] = None
    with open(os.path.join(sd, "meta.json"), "w") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError, match="without a heat source"):
        checkpoint.load(r, sd)
    r.close()


def py(cwd, *args):
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2")
    return subprocess.run([sys.executable, "-m", "heat2d", *args], cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=300)


def test_python_driver_source(native, tmp_path):
    """--source through python -m heat2d on the CPU backend: the golden's field; the checkpoint
    records the digest; a restart without the file and a wrong-shape file fail."""
    n = 50
    (tmp_path / "input.dat").write_text(f"{n} 0.25 0.05 1.0 30 1\n")
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    S = rough_source(n, "fp64")
    np.save(tmp_path / "src.npy", S)
    np.save(tmp_path / "bad.npy", S[:, 1:])
    args = ["--backend", "cpu", "--ic", "hat-cuda", "--quiet", "--output", "npy"]
    out = py(tmp_path, *args, "--source", "src.npy", "--ntime", "12", "--checkpoint", "ck")
    assert out.returncode == 0, out.stdout + out.stderr
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    import hashlib
    assert meta["source_sha256"] == hashlib.sha256(S.tobytes()).hexdigest() and meta["step"] == 12
    bad = py(tmp_path, *args, "--restart", "ck")
    assert bad.returncode != 0 and "heat source" in bad.stdout + bad.stderr
    out = py(tmp_path, *args, "--source", "src.npy", "--restart", "ck")
    assert out.returncode == 0, out.stdout + out.stderr
    # (auto with a source: fma at r = 1/4, the exact form's bits)
    got = np.load(tmp_path / "soln00000.npy")
    assert np.array_equal(got, R.owned(R.ftcs(prob, 30, source=S)))
    bad = py(tmp_path, *args, "--source", "bad.npy")
    assert bad.returncode != 0 and "shape" in bad.stdout + bad.stderr


def test_native_cli_source(native, tmp_path):
    """--source through the native CLI on the CPU backend: auto is fma (not jacobi) at r = 1/4, the
    checkpoint records the digest of the converted array, the Python driver resumes it with the
    same file, a restart without the file and a wrong-shape file fail."""
    import hashlib

    from heat2d.utils import io
    n = 64
    (tmp_path / "input.dat").write_text(f"{n} 0.25 0.05 1.0 30 1\n")
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "uniform")
    assert prob.r == 0.25 and prob.ic.sterbenz_safe()  # where auto without a source is jacobi
    S = rough_source(n, "fp64")
    np.save(tmp_path / "src.npy", S)
    np.save(tmp_path / "bad.npy", S[:, 1:])
    cli = [N.CLI_PATH, "--cpu", "--quiet", "--ic", "uniform"]

    def run_cli(*args):
        return subprocess.run([*cli, *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)

    out = run_cli("--source", "src.npy", "--ntime", "12", "--checkpoint", "ck", "--output", "none", "--json", "w.json")
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads((tmp_path / "w.json").read_text())["arith_used"] == "fma (auto)"
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    assert meta["source_sha256"] == hashlib.sha256(S.tobytes()).hexdigest() and meta["step"] == 12
    bad = run_cli("--restart", "ck")
    assert bad.returncode != 0 and "heat source" in bad.stdout + bad.stderr
    np.save(tmp_path / "other.npy", rough_source(n, "fp64", seed=2))
    bad = run_cli("--restart", "ck", "--source", "other.npy")
    assert bad.returncode != 0 and "differs from the checkpoint" in bad.stdout + bad.stderr
    gold30 = R.owned(R.ftcs(prob, 30, source=S))
    out = run_cli("--restart", "ck", "--source", "src.npy")  # 3 ranks resume the 1-rank checkpoint below too
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(io.read_xyz(str(tmp_path / "soln00000.dat"))[2], gold30)
    out = run_cli("--restart", "ck", "--source", "src.npy", "--gpus", "3", "--output", "npy")
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.concatenate([np.load(tmp_path / f"soln{r:05d}.npy") for r in range(3)], axis=0)
    assert np.array_equal(got, gold30)
    # the other driver resumes it, given the same file
    out = py(tmp_path, "--backend", "cpu", "--ic", "uniform", "--quiet", "--output", "npy", "--source", "src.npy",
             "--restart", "ck")
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.load(tmp_path / "soln00000.npy"), gold30)
    bad = run_cli("--source", "bad.npy")
    assert bad.returncode != 0 and "shape" in bad.stdout + bad.stderr
    # an f8 file in an fp32 run: converted, and the digest is the converted array's
    out = run_cli("--dtype", "fp32", "--source", "src.npy", "--ntime", "5", "--checkpoint", "ck32", "--output", "none")
    assert out.returncode == 0, out.stdout + out.stderr
    with open(tmp_path / "ck32" / "latest") as f:
        meta = json.loads((tmp_path / "ck32" / f.read().strip() / "meta.json").read_text())
    assert meta["source_sha256"] == hashlib.sha256(S.astype(np.float32).tobytes()).hexdigest()
    # without a source the CLI's auto still picks jacobi on this IC, and writes a null digest
    out = run_cli("--ntime", "3", "--checkpoint", "ck0", "--output", "none", "--json", "n.json")
    assert out.returncode == 0 and json.loads((tmp_path / "n.json").read_text())["arith_used"] == "jacobi (auto)"
    with open(tmp_path / "ck0" / "latest") as f:
        assert json.loads((tmp_path / "ck0" / f.read().strip() / "meta.json").read_text())["source_sha256"] is None


# ------------------------------------------------------------------ GPU

DEPTHS = [1, 2, 7, 8, 13, 16, "D"]


@pytest.mark.gpu
@pytest.mark.parametrize("tb", DEPTHS)
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_one_strip(native, gpu, dtype, arith, tb):
    """n = 77: one strip; 2 * tb + 3 steps: two full passes and a shallower one
    (step(tb), step(tb), step(3): one step(2 tb + 3) call runs none of depth tb)."""
    tb = depth(tb)
    steps = 2 * tb + 3
    got = run(77, dtype, "hip", tb, steps, 0.2, arith, full=2)
    assert np.array_equal(got, gold(77, dtype, steps, 0.2, arith))


@pytest.mark.gpu
@pytest.mark.parametrize("tb", [8, "D"])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_several_strips(native, gpu, dtype, sigma, tb):
    """n = 301, 37 steps: several strips, passes of different depth mix."""
    tb = depth(tb)
    for arith in ("exact", "fma"):
        got = run(301, dtype, "hip", tb, 37, sigma, arith, prepare=True)
        assert np.array_equal(got, gold(301, dtype, 37, sigma, arith)), arith


def worker(tmp_path, a, **env):
    out = subprocess.run([sys.executable, os.path.join(HERE, "source_worker.py"), str(tmp_path), json.dumps(a)],
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
    source: one-wave strips) — every launch on the source kernel."""
    tb = 16 if "HEAT2D_PIPE" in env else 8
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
    assert info["info"]["tb"] == tb and info["info"]["source"]["set"]
    assert np.array_equal(got, gold(2897, dtype, 37, 0.2, "exact", rows=301))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_graph_replay(native, gpu, dtype):
    """graph=True, step(n) twice."""
    p = problem(301, 74)
    s = HeatSolver(p, dtype=dtype, backend="hip", tb=8, arith="exact", device=0, graph=True, source=rough_source(301, dtype))
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
    g = LoopbackGroup(p, 3, dtype=dtype, backend="hip", tb=8, arith="exact", device=0, source=rough_source(301, dtype))
    assert [r for _, r in g.slabs()] == [101, 100, 100]
    g.upload(rough_field(301, dtype))
    g.step(37)
    got = g.download()
    g.close()
    assert np.array_equal(got, gold(301, dtype, 37))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_raw_op(native, gpu, dtype):
    """tb_step(source=) on a middle slab; NaN guard bands around the rows written: the new kernel
    writes nothing outside its rects."""
    for k, arith in ((8, "exact"), (depth_max(), "fma")):
        _raw_op("cuda", dtype, k, arith=arith)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_fresh_source_and_none(native, gpu, dtype):
    n, dt, p = 301, NP[dtype], problem(301, 37)
    T0, S1, S2 = rough_field(n, dtype), rough_source(n, dtype), rough_source(n, dtype, seed=2)
    s = HeatSolver(p, dtype=dtype, backend="hip", tb=8, arith="exact", device=0, source=S1)
    s.upload(T0)
    s.step(20)
    s.set_source(S2)
    s.step(17)
    got = s.download()
    mid = R.ftcs(p, 20, dtype=dt, T0=T0, source=S1)
    assert np.array_equal(got, R.owned(R.ftcs(p, 17, dtype=dt, T0=mid, source=S2)))
    s.set_source(None)
    s.upload(T0)
    s.step(37)
    assert np.array_equal(s.download(), R.owned(R.ftcs(p, 37, dtype=dt, T0=T0)))
    s.close()


@pytest.mark.gpu
def test_hip_depth_clamp_and_refusals(native, gpu):
    S = rough_source(301, "fp64")
    s = HeatSolver(problem(301, 4), backend="hip", device=0, tb=24, source=S)
    info = s.info()
    s.close()
    assert info["tb"] == depth_max() and info["source"]["max_tb"] == depth_max()
    for kw, why in ((dict(arith="jacobi"), "jacobi"), (dict(engine="jit"), "jit"), (dict(copy_swap=True), "copy-swap"),
                    (dict(bc_y="insulated"), "Dirichlet")):
        with pytest.raises(RuntimeError, match=why):
            HeatSolver(problem(301, 4, 0.25), backend="hip", device=0, source=S, **kw)
