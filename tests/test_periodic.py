"""Periodic boundary conditions on either axis (bc_x: rows, decomposed over
ranks; bc_y: columns), bitwise against the NumPy golden at every pass depth,
launch plan and rank count.

Data: rough values 10**uniform(-1, 1), frame included (the frame of a
Dirichlet axis is kept, the frame of a periodic one is ignored by upload());
r = 0.2371 with arith="exact" unless a case says otherwise. Every comparison is
np.array_equal except the "fast" arithmetic, which has its stated bound
(models.reference.fast_error_bound).

Two oracles: models.reference.ftcs(bc_x=, bc_y=) — one np.pad(mode="wrap")
layer before every single step — and the roll identity: the run from
np.roll(T0, (a, b)) is the rolled run, bitwise, which crosses every strip,
band and rank seam.

Conservation bound (fully periodic, values in [1, 2]): one step computes each
point in 6 rounded operations on values <= 8 max|T|, its sum over the grid
changes by at most 8 u sum|T| per step (the exact update conserves the sum),
so |sum T_m - sum T_0| / sum T_0 <= 8 m u, u = eps / 2; sums in fp64.
"""
import dataclasses
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import heat2d
from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver, LoopbackGroup
from heat2d.ops import _native as N
from heat2d.utils import io

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cycles as Y  # noqa: E402
from periodic_worker import problem, rough_field  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
COMBOS = [("periodic", "dirichlet"), ("dirichlet", "periodic"), ("periodic", "periodic")]
IDS = ["x", "y", "xy"]
STEPS = 57
PP = dict(bc_x="periodic", bc_y="periodic")

_GOLD = {}


def gold(n, dtype, bc_x, bc_y, steps=STEPS, sigma=0.2371, arith="exact", lo=-1.0, hi=1.0, roll=None):
    """Owned points of the golden run from rough_field (computed once, read-only)."""
    key = (n, dtype, bc_x, bc_y, steps, sigma, arith, lo, hi, roll)
    if key not in _GOLD:
        T0 = rough_field(n, dtype, lo=lo, hi=hi)
        if roll:
            T0 = rolled(T0, roll)
        g = R.owned(R.ftcs(problem(n, steps, sigma), steps, dtype=NP[dtype], T0=T0, arith=arith, bc_x=bc_x, bc_y=bc_y))
        g = np.ascontiguousarray(g)
        g.setflags(write=False)
        _GOLD[key] = g
    return _GOLD[key]


def rolled(T0, shift):
    """Frame-inclusive field whose owned points are rolled by `shift` (periodic frame: ignored)."""
    out = T0.copy()
    out[1:-1, 1:-1] = np.roll(T0[1:-1, 1:-1], shift, axis=(0, 1))
    return out


def run(n, dtype, backend, tb, bc_x, bc_y, steps=STEPS, sigma=0.2371, arith="exact", T0=None, ranks=1, prepare=False,
        lo=-1.0, hi=1.0, stats=False, calls=None, **kw):
    """One run of `steps` steps: as one step(steps) call (balanced cycles, none
    of depth tb once steps > tb), or as the step() calls of `calls`
    (tests/cycles.py calls(tb, steps, full): `full` cycles of depth tb, then
    the remainder) — then every solver's cycle_hist() must show those `full`
    cycles of depth tb. With stats the last call is step_stats() (these
    boundary conditions take the unfused statistics path: n - 1 steps, then
    one step with the statistics)."""
    p = problem(n, steps, sigma)
    T0 = rough_field(n, dtype, lo=lo, hi=hi) if T0 is None else T0
    dev = dict(device=0) if backend == "hip" else {}
    sizes = [steps] if calls is None else list(calls)
    assert sum(sizes) == steps
    full = 0 if calls is None else sum(1 for m in sizes if m == tb)
    if ranks > 1:
        s = LoopbackGroup(p, ranks, dtype=dtype, backend=backend, tb=tb, arith=arith, bc_x=bc_x, bc_y=bc_y, **dev, **kw)
        s.upload(T0)
        for m in sizes:
            s.step(m)
        out = s.download()
        hists = [s.cycle_hist(i) for i in range(ranks)]
        s.close()
        for h in hists:
            assert full == 0 or (Y.ran(h, tb, full) and max(h) == tb), (tb, sizes, hists)
        return out
    s = HeatSolver(p, dtype=dtype, backend=backend, tb=tb, arith=arith, bc_x=bc_x, bc_y=bc_y, **dev, **kw)
    s.upload(T0)
    st = None
    for i, m in enumerate(sizes):
        if prepare:
            s.prepare(m)
        if stats and i == len(sizes) - 1:
            st = s.step_stats(m)
        else:
            s.step(m)
    out, hist = s.download(), s.cycle_hist()
    s.close()
    assert full == 0 or (Y.ran(hist, tb, full) and max(hist) == tb), (tb, sizes, hist)
    return (out, st) if stats else out


# ------------------------------------------------------------------ CPU

@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_roll_identity(dtype):
    n, shift = 77, (5, 11)
    p = problem(n, STEPS)
    T0 = rough_field(n, dtype)
    a = R.owned(R.ftcs(p, STEPS, dtype=NP[dtype], T0=rolled(T0, shift), **PP))
    assert np.array_equal(a, np.roll(gold(n, dtype, "periodic", "periodic"), shift, axis=(0, 1)))


def test_golden_frame_is_wrap_image():
    T = R.ftcs(problem(31, 5), 5, T0=rough_field(31, "fp64"), bc_x="dirichlet", bc_y="periodic")
    assert np.array_equal(T[:, 0], T[:, -2]) and np.array_equal(T[:, -1], T[:, 1])  # frame rows included
    assert np.array_equal(T[0], R.wrap_frame(rough_field(31, "fp64"), "dirichlet", "periodic")[0])  # x frame kept


@pytest.mark.parametrize("tb", [1, 4, 8])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS, ids=IDS)
def test_cpu_twin_bitwise(native, bc_x, bc_y, dtype, tb):
    assert np.array_equal(run(77, dtype, "cpu", tb, bc_x, bc_y), gold(77, dtype, bc_x, bc_y))


@pytest.mark.parametrize("tb", [20, 24])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS[:2], ids=IDS[:2])
def test_cpu_twin_deep_calls(native, bc_x, bc_y, tb):
    """The GPU tests' call sequences (step(tb), step(tb), the remainder) on the
    CPU twin at depths 20 and 24 — 24: as many levels as there are ghost
    columns — against the same golden: the oracle of test_hip_bitwise is
    exercised without a GPU. run() asserts the depth from cycle_hist()."""
    assert Y.calls(tb, STEPS, 2) == [tb, tb, STEPS - 2 * tb]
    got = run(261, "fp64", "cpu", tb, bc_x, bc_y, calls=Y.calls(tb, STEPS, 2))
    assert np.array_equal(got, gold(261, "fp64", bc_x, bc_y))


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("tb", [1, 4, 8])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS, ids=IDS)
def test_cpu_twin_loopback_ranks(native, bc_x, bc_y, dtype, tb, ranks):
    if ranks == 3:
        g = LoopbackGroup(problem(80, 1), 3, backend="cpu", tb=tb, bc_x=bc_x, bc_y=bc_y)
        assert [nr for _, nr in g.slabs()] == [27, 27, 26]
        g.close()
    assert np.array_equal(run(80, dtype, "cpu", tb, bc_x, bc_y, ranks=ranks), gold(80, dtype, bc_x, bc_y))


def test_cpu_frame_roundtrip(native):
    """upload() ignores the frame entries of a periodic axis and keeps those of
    a Dirichlet one; download_field() returns wrap images / the kept frame."""
    n, T0 = 40, rough_field(40, "fp64")
    for bc_x, bc_y in COMBOS:
        s = HeatSolver(problem(n, 9), backend="cpu", tb=4, arith="exact", bc_x=bc_x, bc_y=bc_y)
        s.upload(T0)
        assert np.array_equal(s.download_field(), R.wrap_frame(T0, bc_x, bc_y))
        s.step(9)
        assert np.array_equal(s.download_field(), R.ftcs(problem(n, 9), 9, T0=T0, bc_x=bc_x, bc_y=bc_y))
        s.close()


def test_periodic_eigenmode(native):
    n, r, k, l = 64, 0.2371, 3, 5
    i = np.arange(n)
    mode = np.cos(2 * np.pi * k * i / n)[:, None] * np.cos(2 * np.pi * l * i / n)[None, :]
    g = R.periodic_eigen_factor(problem(n, 1).r, n, k, l)
    assert abs(g - (1 - 4 * r * (np.sin(np.pi * k / n) ** 2 + np.sin(np.pi * l / n) ** 2))) < 1e-12
    T = np.pad(mode, 1, mode="wrap")
    p = problem(n, 20)
    for m in range(1, 21):
        T = R.ftcs_step(T, p.r, **PP)
        exact = R.periodic_eigenmode(p.r, n, m, k, l)
        assert np.abs(R.owned(T) - exact).max() <= 1e-12 * g ** m
    s = HeatSolver(p, backend="cpu", tb=5, arith="exact", **PP)
    s.upload(np.pad(mode, 1, mode="wrap"))
    s.step(20)
    assert np.array_equal(s.download(), R.owned(T))
    s.close()


def conservation(T0, T, dtype):
    s0, s1 = T0.astype(np.float64).sum(), T.astype(np.float64).sum()
    rel = abs(s1 - s0) / s0
    bound = 8 * STEPS * float(np.finfo(NP[dtype]).eps) / 2
    print(f"conservation {dtype}: relative drift {rel:.3e}, bound {bound:.3e}")
    assert rel <= bound


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_conservation_golden_and_twin(native, dtype):
    T0 = rough_field(77, dtype, lo=0.0, hi=np.log10(2.0))
    g = gold(77, dtype, "periodic", "periodic", lo=0.0, hi=np.log10(2.0))
    conservation(R.owned(T0), g, dtype)
    got = run(77, dtype, "cpu", 8, "periodic", "periodic", lo=0.0, hi=np.log10(2.0))
    assert np.array_equal(got, g)


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_callback_transport_periodic_x(native, tmp_path, world):
    a = {"n": 80, "steps": STEPS, "tb": 4, "dtype": "fp64", "bc_x": "periodic", "bc_y": "periodic" if world == 3 else "dirichlet"}
    port = free_port()
    env = dict(os.environ, OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2", MASTER_ADDR="127.0.0.1", HEAT2D_COMM_TIMEOUT="120")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "periodic_worker.py"), "gloo", str(r), str(world),
                               str(port), str(tmp_path), json.dumps(a)], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(world)]
    try:
        outs = [p.communicate(timeout=240)[0].decode(errors="replace") for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o[-3000:]
    assert np.array_equal(np.load(tmp_path / "result.npy"), gold(80, "fp64", a["bc_x"], a["bc_y"]))


def test_refusals(native):
    """(The peer transport needs a GPU: test_refusal_peer_transport. An RCCL
    communicator of more than one rank cannot be built without GPUs.)"""
    p = problem(80, 4)
    with pytest.raises(RuntimeError, match="periodic"):
        HeatSolver(p, backend="cpu", engine="jit", bc_x="periodic")
    with pytest.raises(RuntimeError, match="periodic"):
        HeatSolver(p, backend="cpu", copy_swap=True, bc_y="periodic")
    with pytest.raises(RuntimeError, match="too small for periodic y"):
        HeatSolver(problem(20, 4), backend="cpu", bc_y="periodic")
    with pytest.raises(RuntimeError, match="too small for periodic x"):
        LoopbackGroup(problem(30, 4), 3, backend="cpu", tb=12, bc_x="periodic")
    with pytest.raises(ValueError, match="bc_x"):
        HeatSolver(p, backend="cpu", bc_x="mirror")


@pytest.mark.gpu
def test_refusal_peer_transport(native, gpu):
    """Periodic x on 2 peer-transport ranks: a clear error from every rank's solver."""
    cwd = os.path.join(HERE, "..")
    out = subprocess.run([N.CLI_PATH, os.path.join(HERE, "golden", "reference_inputs", "fortran", "hip", "input.dat"),
                          "--gpus", "2", "--transport", "peer", "--share-gpu", "--bc-x", "periodic", "--n", "128",
                          "--ntime", "4", "--output", "none", "--quiet"], cwd=cwd, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode != 0
    assert "periodic x" in out.stdout + out.stderr


def test_python_driver_rejects_unknown_bc(native, tmp_path):
    (tmp_path / "input.dat").write_text("64 0.2371 0.05 1.0 8 1\n")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), WORLD_SIZE="1")
    out = subprocess.run([sys.executable, "-m", "heat2d", "--backend", "cpu", "--bc-x", "mirror"], cwd=tmp_path,
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--bc-x" in out.stderr


def test_defaults_report_dirichlet(native):
    s = HeatSolver(problem(40, 1), backend="cpu")
    info = s.info()
    s.close()
    assert info["bc_x"] == "dirichlet" and info["bc_y"] == "dirichlet"
    s = HeatSolver(problem(40, 1), backend="cpu", bc_y="periodic")
    assert (s.info()["bc_x"], s.info()["bc_y"]) == ("dirichlet", "periodic")
    s.close()


def read_soln(path):
    return io.read_xyz(str(path))[2]


@pytest.mark.parametrize("gpus", [1, 3])
def test_cli_cpu_fully_periodic(native, tmp_path, gpus):
    (tmp_path / "input.dat").write_text("67 0.2371 0.05 1.0 23 1\n")
    out = subprocess.run([N.CLI_PATH, "--cpu", "--gpus", str(gpus), "--tb", "4", "--arith", "exact", "--bc-x", "periodic",
                          "--bc-y", "periodic", "--ic", "hat-cuda"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    ref = R.owned(R.ftcs(prob, **PP))
    got = np.concatenate([read_soln(tmp_path / f"soln{r:05d}.dat") for r in range(gpus)], axis=0)
    assert np.array_equal(got, ref)
    assert not np.array_equal(ref, R.owned(R.ftcs(prob)))  # the boundary condition matters on this IC


def py(cwd, *args):
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2")
    return subprocess.run([sys.executable, "-m", "heat2d", *args], cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=300)


@pytest.mark.parametrize("writer", ["cli", "py"])
def test_checkpoint_round_trip(native, tmp_path, writer):
    """Written by one driver, resumed by the other: meta.json carries the
    settings, the restart takes them from it, a conflicting flag fails."""
    (tmp_path / "input.dat").write_text("50 0.2371 0.05 1.0 30 1\n")
    cli = [N.CLI_PATH, "--cpu", "--quiet", "--arith", "exact", "--ic", "hat-cuda"]
    pyargs = ["--backend", "cpu", "--arith", "exact", "--ic", "hat-cuda", "--quiet"]
    bc = ["--bc-x", "periodic", "--bc-y", "periodic"]
    if writer == "cli":
        w = subprocess.run([*cli, *bc, "--ntime", "12", "--checkpoint", "ck", "--output", "none"], cwd=tmp_path,
                           capture_output=True, text=True, timeout=300)
    else:
        w = py(tmp_path, *pyargs, *bc, "--ntime", "12", "--checkpoint", "ck", "--output", "none")
    assert w.returncode == 0, w.stdout + w.stderr
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    assert meta["bc_x"] == "periodic" and meta["bc_y"] == "periodic" and meta["step"] == 12
    if writer == "cli":  # resumed by the other driver, without the flags
        bad = py(tmp_path, *pyargs, "--restart", "ck", "--bc-y", "dirichlet")
        r = py(tmp_path, *pyargs, "--restart", "ck")
    else:
        bad = subprocess.run([*cli, "--restart", "ck", "--bc-y", "dirichlet"], cwd=tmp_path, capture_output=True,
                             text=True, timeout=300)
        r = subprocess.run([*cli, "--restart", "ck"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "conflicts with the checkpoint" in bad.stdout + bad.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    assert np.array_equal(read_soln(tmp_path / "soln00000.dat"), R.owned(R.ftcs(prob, **PP)))


def test_raw_wrap_ops_cpu(native):
    import torch

    from heat2d.ops import kernels as K
    L = K.make_layout(70, 261, halo=24)
    f = torch.from_numpy(np.random.default_rng(3).random(L.elems()))
    v = K.view2d(f, L).numpy()
    own = v[24:94, 32:32 + 261].copy()
    K.wrap_cols(f, L, rows=(0, 70))
    K.wrap_rows(f, L, 24)
    want = np.pad(own, 24, mode="wrap")
    assert np.array_equal(v[0:118, 8:32 + 261 + 24], want)


# ------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("tb", [1, 4, 16, 17, 20, 21, 23, 24])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS, ids=IDS)
def test_hip_bitwise(native, gpu, bc_x, bc_y, dtype, tb):
    """Two cycles of depth tb and the remainder (tb 24: 24, 24, 9), asserted
    from cycle_hist() in run(): one step(57) call at tb 24 runs 19, 19, 19.
    21 and 23: odd depths whose strip halo rounds up to whole lanes; 24: the
    24 ghost columns of periodic y are crossed in exactly 24 levels."""
    got = run(261, dtype, "hip", tb, bc_x, bc_y, prepare=True, calls=Y.calls(tb, STEPS, 2))
    assert np.array_equal(got, gold(261, dtype, bc_x, bc_y))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS, ids=IDS)
def test_hip_single_call(native, gpu, bc_x, bc_y, dtype):
    """ONE step(57) call at tb 16: balanced cycles (15, 14, 14, 14) under the periodic views."""
    assert Y.balanced(16, STEPS) == [15, 14, 14, 14]
    got = run(261, dtype, "hip", 16, bc_x, bc_y, prepare=True)
    assert np.array_equal(got, gold(261, dtype, bc_x, bc_y))


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(graph=True), dict(autotune=1)], ids=["graph", "autotune"])
def test_hip_plan_variants(native, gpu, kw):
    got = run(261, "fp64", "hip", 8, "periodic", "periodic", prepare=True, **kw)
    assert np.array_equal(got, gold(261, "fp64", "periodic", "periodic"))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["edge-first", "concurrent", "lead"])
def test_hip_split_orders(native, gpu, tmp_path, order):
    a = {"n": 261, "steps": STEPS, "tb": 8, "dtype": "fp64", "bc_x": "periodic", "bc_y": "periodic"}
    env = dict(os.environ, HEAT2D_SPLIT_ORDER=order, HEAT2D_PLAN_CACHE="off")
    out = subprocess.run([sys.executable, os.path.join(HERE, "periodic_worker.py"), "single", str(tmp_path),
                          json.dumps(a)], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    plan = json.loads((tmp_path / "info.json").read_text())["plan"]
    assert plan["order"] == order, plan
    assert np.array_equal(np.load(tmp_path / "result.npy"), gold(261, "fp64", "periodic", "periodic"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_jacobi(native, gpu, dtype):
    got = run(261, dtype, "hip", 20, "periodic", "periodic", sigma=0.25, arith="jacobi", prepare=True, calls=Y.calls(20, STEPS, 2))
    assert np.array_equal(got, gold(261, dtype, "periodic", "periodic", sigma=0.25, arith="jacobi"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_fast_within_bound(native, gpu, dtype):
    got = run(261, dtype, "hip", 20, "periodic", "periodic", arith="fast", prepare=True, calls=Y.calls(20, STEPS, 2))
    ref = gold(261, dtype, "periodic", "periodic")
    tmax = float(np.abs(rough_field(261, dtype)).max())
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    print(f"fast vs exact {dtype}: {err:.3e}, bound {R.fast_error_bound(STEPS, NP[dtype], tmax):.3e}")
    assert err <= R.fast_error_bound(STEPS, NP[dtype], tmax)


@pytest.mark.gpu
@pytest.mark.parametrize("n,ranks", [(261, 1), (262, 3)])
def test_hip_roll_identity(native, gpu, n, ranks):
    shift = (37, 130)
    base = run(n, "fp64", "hip", 20, "periodic", "periodic", ranks=ranks, calls=Y.calls(20, STEPS, 2))
    got = run(n, "fp64", "hip", 20, "periodic", "periodic", ranks=ranks, T0=rolled(rough_field(n, "fp64"), shift),
              calls=Y.calls(20, STEPS, 2))
    assert np.array_equal(got, np.roll(base, shift, axis=(0, 1)))
    assert np.array_equal(base, gold(n, "fp64", "periodic", "periodic"))


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("ranks", [2, 3])
def test_hip_loopback(native, gpu, ranks, overlap):
    if ranks == 3:
        g = LoopbackGroup(problem(262, 1), 3, backend="hip", device=0, tb=20, **PP)
        assert [nr for _, nr in g.slabs()] == [88, 87, 87]
        g.close()
    for dtype in ("fp64", "fp32"):
        got = run(262, dtype, "hip", 20, "periodic", "periodic", ranks=ranks, overlap=overlap, calls=Y.calls(20, STEPS, 2))
        assert np.array_equal(got, gold(262, dtype, "periodic", "periodic")), dtype


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_guard_nan_beyond_ghosts(native, gpu, dtype):
    """The allocation padding (IcSpec.pad: every pad column beyond the 24 ghost
    columns and every ghost row beyond the depth in use, 20 of 24) holds NaN."""
    p = problem(261, STEPS)
    p = dataclasses.replace(p, ic=dataclasses.replace(p.ic, pad=float("nan")))
    s = HeatSolver(p, dtype=dtype, backend="hip", tb=20, arith="exact", device=0, **PP)
    s.upload(rough_field(261, dtype))
    for m in Y.calls(20, STEPS, 2):
        s.prepare(m)
        s.step(m)
    got, hist = s.download(), s.cycle_hist()
    L = s.layout
    out = np.empty((L.nrows + 2 * L.halo, L.pitch), dtype=NP[dtype])
    N.call("heat2d_solver_download_region", s._h, -L.halo, L.nrows + L.halo, -L.cpad, L.pitch - L.cpad,
           out.ctypes.data, L.pitch)
    s.close()
    Y.assert_ran(hist, 20, 2)
    assert max(hist) == 20, hist
    assert np.isnan(out[:L.halo - 20, :]).all() and np.isnan(out[:, :L.cpad - 24]).all()  # the guard was in place
    assert not np.isnan(got).any()
    assert np.array_equal(got, gold(261, dtype, "periodic", "periodic"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_fused_stats(native, gpu, dtype):
    lo, hi = 0.0, float(np.log10(2.0))
    got, st = run(261, dtype, "hip", 20, "periodic", "periodic", lo=lo, hi=hi, stats=True, prepare=True, calls=Y.calls(20, STEPS, 2))
    g = gold(261, dtype, "periodic", "periodic", lo=lo, hi=hi)
    g1 = gold(261, dtype, "periodic", "periodic", steps=STEPS - 1, lo=lo, hi=hi)
    assert np.array_equal(got, g)
    g64, d = g.astype(np.float64), g.astype(np.float64) - g1.astype(np.float64)
    assert st["min"] == g64.min() and st["max"] == g64.max() and st["residual_max"] == np.abs(d).max()
    assert np.isclose(st["sum"], g64.sum(), rtol=1e-12, atol=0) and np.isclose(st["sum_sq"], (g64 * g64).sum(), rtol=1e-12)
    assert np.isclose(st["residual_l2"], np.sqrt((d * d).sum()), rtol=1e-10)
    conservation(R.owned(rough_field(261, dtype, lo=lo, hi=hi)), got, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_raw_ops(native, gpu, dtype):
    import torch

    from heat2d.ops import kernels as K
    L = K.make_layout(70, 261, halo=24)
    host = np.random.default_rng(3).random(L.elems()).astype(NP[dtype])
    f = torch.from_numpy(host).cuda()
    own = host.reshape(L.rows_alloc(), L.pitch)[24:94, 32:32 + 261].copy()
    K.wrap_cols(f, L, rows=(0, 70))
    K.wrap_rows(f, L, 24)
    v = K.view2d(f, L).cpu().numpy()
    assert np.array_equal(v[0:118, 8:32 + 261 + 24], np.pad(own, 24, mode="wrap"))
    # nothing else written: the owned rows' pad columns beyond the 24 ghost
    # columns keep their values, and the ghost rows are whole-row copies
    h2 = host.reshape(v.shape)
    assert np.array_equal(v[24:94, :8], h2[24:94, :8]) and np.array_equal(v[24:94, 317:], h2[24:94, 317:])
    assert np.array_equal(v[0:24], v[70:94]) and np.array_equal(v[94:118], v[24:48])
    # the raw stencil op with unpinned rows and columns: 20 steps of the 70 x 261 torus
    g = torch.empty_like(f)
    K.tb_step(f, g, L, 20, 0.2371, arith="exact", bc_x="periodic", bc_y="periodic")
    T = np.pad(own, 1, mode="wrap")
    for _ in range(20):
        T = R.ftcs_step(T, 0.2371, **PP)
    assert np.array_equal(K.owned(g, L).cpu().numpy(), R.owned(T))
