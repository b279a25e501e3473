"""Insulated (zero-flux) boundaries on either axis (bc_x: rows, decomposed over
ranks; bc_y: columns), bitwise against the NumPy golden at every pass depth,
launch plan and rank count.

Convention: the n owned points are the unknowns, the wall sits half a cell
outside the first and last owned point, and the frame entry of an insulated
axis is the image of the adjacent owned point (T[0] = T[1], T[n+1] = T[n]).
The golden (models.reference.ftcs) refreshes those entries with one
np.pad(mode="edge") layer before every single step.

Data: rough values 10**uniform(-1, 1), frame included (the frame of a
Dirichlet axis is kept, the frame of an insulated one is ignored by upload());
r = 0.2371 with arith="exact", 57 steps and np.array_equal unless a case says
otherwise.

Negative control: K fused levels over K + 1 mirrored ghost layers
(np.pad(mode="symmetric")) — the route periodic boundaries take — do NOT have
the golden's bits: a mirrored point sums ((S + E) + N) + W with two operands
swapped relative to its image and drifts from it. So the engine substitutes
the operand at the wall instead (tb_impl.hpp March INS), and an implementation
by ghost layers cannot pass the bitwise tests below.

Conservation bound (fully insulated, values in [1, 2]): as in
tests/test_periodic.py — one step computes each point in 6 rounded operations
on values <= 8 max|T|, the exact update conserves the sum (the flux through an
insulated wall is zero), so |sum T_m - sum T_0| / sum T_0 <= 8 m u, u = eps / 2;
sums in fp64.

Eigenmode bound: cos(p pi (i + 1/2) / n) cos(q pi (j + 1/2) / n) decays by
g = 1 - 4r (sin^2(p pi / 2n) + sin^2(q pi / 2n)) per step; the ~6 roundings of
a step on values <= 1 add up linearly (FTCS with r <= 1/4 is non-expansive in
the max norm), ~6 m u, so the golden after m steps is within 8 m u of g^m T_0.
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
from heat2d.utils import io

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cycles as Y  # noqa: E402
from periodic_worker import problem, rough_field  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
COMBOS = [("insulated", "dirichlet"), ("dirichlet", "insulated"), ("insulated", "insulated"),
          ("insulated", "periodic"), ("periodic", "insulated")]
IDS = ["x", "y", "xy", "x-py", "px-y"]
STEPS = 57
II = dict(bc_x="insulated", bc_y="insulated")

_GOLD = {}


def gold(n, dtype, bc_x, bc_y, steps=STEPS, sigma=0.2371, arith="exact", lo=-1.0, hi=1.0, framed=False):
    """The golden run from rough_field (computed once, read-only): owned points, or with its frame."""
    key = (n, dtype, bc_x, bc_y, steps, sigma, arith, lo, hi)
    if key not in _GOLD:
        T0 = rough_field(n, dtype, lo=lo, hi=hi)
        g = R.ftcs(problem(n, steps, sigma), steps, dtype=NP[dtype], T0=T0, arith=arith, bc_x=bc_x, bc_y=bc_y)
        g = np.ascontiguousarray(g)
        g.setflags(write=False)
        _GOLD[key] = g
    return _GOLD[key] if framed else R.owned(_GOLD[key])


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


# ------------------------------------------------------------------ CPU: the golden

def test_golden_frame_is_edge_image():
    T0 = rough_field(31, "fp64")
    T = R.ftcs(problem(31, 5), 5, T0=T0, **II)
    assert np.array_equal(T, np.pad(T[1:-1, 1:-1], 1, mode="edge"))
    # one axis insulated: the Dirichlet axis keeps its frame, with edge images at its ends
    T = R.ftcs(problem(31, 5), 5, T0=T0, bc_x="dirichlet", bc_y="insulated")
    assert np.array_equal(T[:, 0], T[:, 1]) and np.array_equal(T[:, -1], T[:, -2])  # frame rows included
    assert np.array_equal(T[0, 1:-1], T0[0, 1:-1]) and np.array_equal(T[-1, 1:-1], T0[-1, 1:-1])
    T = R.ftcs(problem(31, 5), 5, T0=T0, bc_x="insulated", bc_y="dirichlet")
    assert np.array_equal(T[0], T[1]) and np.array_equal(T[-1], T[-2])
    assert np.array_equal(T[1:-1, 0], T0[1:-1, 0]) and np.array_equal(T[1:-1, -1], T0[1:-1, -1])
    with pytest.raises(ValueError, match="bc_y"):
        R.wrap_frame(T0, "insulated", "mirror")


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_differs_from_dirichlet(dtype):
    d = np.mean(gold(77, dtype, *II.values()) != gold(77, dtype, "dirichlet", "dirichlet"))
    print(f"insulated golden differs from the Dirichlet one at {100 * d:.1f} % of the points ({dtype})")
    assert d > 0


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_ghost_route_negative_control(dtype):
    """K = 8 fused levels over 9 mirrored layers differ from 8 golden steps."""
    n, K, dt = 77, 8, NP[dtype]
    T0 = rough_field(n, dtype)
    P = np.pad(T0[1:-1, 1:-1], K + 1, mode="symmetric")
    r, four = dt(0.2371), dt(4)
    for _ in range(K):
        Q = P.copy()
        c = P[1:-1, 1:-1]
        Q[1:-1, 1:-1] = c + r * ((((P[2:, 1:-1] + P[1:-1, 2:]) + P[:-2, 1:-1]) + P[1:-1, :-2]) - four * c)
        P = Q
    fused = P[K + 1:-K - 1, K + 1:-K - 1]
    share = float(np.mean(fused != gold(n, dtype, *II.values(), steps=K)))
    print(f"ghost route differs from the golden at {100 * share:.2f} % of the owned points ({dtype})")
    assert share >= 0.005


def conservation(T0, T, dtype, steps=STEPS):
    s0, s1 = T0.astype(np.float64).sum(), T.astype(np.float64).sum()
    rel = abs(s1 - s0) / s0
    bound = 8 * steps * float(np.finfo(NP[dtype]).eps) / 2
    print(f"conservation {dtype}: relative drift {rel:.3e}, bound {bound:.3e}")
    assert rel <= bound


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_conservation_golden_and_twin(native, dtype):
    lo, hi = 0.0, float(np.log10(2.0))
    g = gold(77, dtype, *II.values(), lo=lo, hi=hi)
    conservation(R.owned(rough_field(77, dtype, lo=lo, hi=hi)), g, dtype)
    assert np.array_equal(run(77, dtype, "cpu", 8, *II.values(), lo=lo, hi=hi), g)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("p,q", [(1, 1), (3, 2)])
def test_eigenmode(native, p, q, dtype):
    n, dt = 77, NP[dtype]
    prob = problem(n, STEPS)
    i = np.arange(n) + 0.5
    mode = np.cos(np.pi * p * i / n)[:, None] * np.cos(np.pi * q * i / n)[None, :]
    assert abs(R.insulated_eigen_factor(prob.r, n, p, q) -
               (1 - 4 * 0.2371 * (np.sin(np.pi * p / (2 * n)) ** 2 + np.sin(np.pi * q / (2 * n)) ** 2))) < 1e-12
    T0 = np.pad(mode, 1, mode="edge").astype(dt)
    T = R.ftcs(prob, STEPS, dtype=dt, T0=T0, **II)
    u = float(np.finfo(dt).eps) / 2
    err = float(np.abs(R.owned(T).astype(np.float64) - R.insulated_eigenmode(prob.r, n, STEPS, p, q)).max())
    print(f"eigenmode ({p}, {q}) {dtype}: max error {err:.3e} = {err / (STEPS * u):.2f} m u, bound 8 m u")
    assert err <= 8 * STEPS * u
    s = HeatSolver(prob, dtype=dtype, backend="cpu", tb=5, arith="exact", **II)
    s.upload(T0)
    s.step(STEPS)
    assert np.array_equal(s.download(), R.owned(T))
    s.close()


# ------------------------------------------------------------------ CPU: the twin

@pytest.mark.parametrize("tb", [1, 4, 8])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS, ids=IDS)
def test_cpu_twin_bitwise(native, bc_x, bc_y, dtype, tb):
    assert np.array_equal(run(77, dtype, "cpu", tb, bc_x, bc_y), gold(77, dtype, bc_x, bc_y))


@pytest.mark.parametrize("ranks", [2, 3])
@pytest.mark.parametrize("tb", [1, 4, 8])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS, ids=IDS)
def test_cpu_twin_loopback_ranks(native, bc_x, bc_y, dtype, tb, ranks):
    assert np.array_equal(run(80, dtype, "cpu", tb, bc_x, bc_y, ranks=ranks), gold(80, dtype, bc_x, bc_y))


@pytest.mark.parametrize("arith", ["fma", "jacobi", "auto"])
def test_cpu_twin_arith_forms(native, arith):
    """fma / auto at r = 0.25 (r * x exact: the contracted form has the exact form's bits) and the jacobi form."""
    got = run(77, "fp64", "cpu", 8, *II.values(), sigma=0.25, arith=arith)
    assert np.array_equal(got, gold(77, "fp64", *II.values(), sigma=0.25, arith="jacobi" if arith == "jacobi" else "exact"))


def test_cpu_frame_roundtrip(native):
    """upload() ignores the frame entries of an insulated axis and keeps those
    of a Dirichlet one; download_field() returns the images / the kept frame."""
    n, T0 = 40, rough_field(40, "fp64")
    for bc_x, bc_y in COMBOS:
        s = HeatSolver(problem(n, 9), backend="cpu", tb=4, arith="exact", bc_x=bc_x, bc_y=bc_y)
        s.upload(T0)
        assert np.array_equal(s.download_field(), R.wrap_frame(T0, bc_x, bc_y)), (bc_x, bc_y)
        s.step(9)
        assert np.array_equal(s.download_field(), R.ftcs(problem(n, 9), 9, T0=T0, bc_x=bc_x, bc_y=bc_y)), (bc_x, bc_y)
        s.close()


def test_info_reports_insulated(native):
    s = HeatSolver(problem(40, 1), backend="cpu", bc_x="insulated")
    assert (s.info()["bc_x"], s.info()["bc_y"]) == ("insulated", "dirichlet")
    s.close()
    s = HeatSolver(problem(40, 1), backend="cpu", bc_x="periodic", bc_y="insulated")
    assert (s.info()["bc_x"], s.info()["bc_y"]) == ("periodic", "insulated")
    s.close()


def test_refusals(native):
    p = problem(80, 4)
    with pytest.raises(RuntimeError, match="insulated"):
        HeatSolver(p, backend="cpu", engine="jit", bc_x="insulated")
    with pytest.raises(RuntimeError, match="insulated"):
        HeatSolver(p, backend="cpu", copy_swap=True, bc_y="insulated")
    with pytest.raises(RuntimeError, match="insulated"):
        HeatSolver(p, backend="cpu", arith="fast", bc_y="insulated")
    with pytest.raises(ValueError, match="bc_y"):
        HeatSolver(p, backend="cpu", bc_y="neumann")


def test_python_driver_rejects_unknown_bc(native, tmp_path):
    (tmp_path / "input.dat").write_text("64 0.2371 0.05 1.0 8 1\n")
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), WORLD_SIZE="1")
    out = subprocess.run([sys.executable, "-m", "heat2d", "--backend", "cpu", "--bc-y", "neumann"], cwd=tmp_path,
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode != 0 and "--bc-y" in out.stderr
    out = subprocess.run([N.CLI_PATH, "--cpu", "--bc-y", "neumann"], cwd=tmp_path, capture_output=True, text=True,
                         timeout=120)
    assert out.returncode != 0 and "insulated" in out.stdout + out.stderr


def read_soln(path):
    return io.read_xyz(str(path))[2]


@pytest.mark.parametrize("gpus", [1, 3])
def test_cli_cpu_fully_insulated(native, tmp_path, gpus):
    (tmp_path / "input.dat").write_text("67 0.2371 0.05 1.0 23 1\n")
    out = subprocess.run([N.CLI_PATH, "--cpu", "--gpus", str(gpus), "--tb", "4", "--arith", "exact", "--bc-x", "insulated",
                          "--bc-y", "insulated", "--ic", "hat-cuda"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    ref = R.owned(R.ftcs(prob, **II))
    got = np.concatenate([read_soln(tmp_path / f"soln{r:05d}.dat") for r in range(gpus)], axis=0)
    assert np.array_equal(got, ref)
    assert not np.array_equal(ref, R.owned(R.ftcs(prob)))  # the boundary condition matters on this IC


def test_cli_inclusive_output_carries_the_images(native, tmp_path):
    """soln.dat of the frame-inclusive variant: the frame entries are the edge images."""
    (tmp_path / "input.dat").write_text("41 0.2371 0.05 1.0 9 1\n")
    out = subprocess.run([N.CLI_PATH, "--cpu", "--variant", "serial", "--tb", "4", "--arith", "exact", "--bc-x", "insulated",
                          "--bc-y", "insulated"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for name in ("int.dat", "soln.dat"):
        T = read_soln(tmp_path / name)
        assert np.array_equal(T, np.pad(T[1:-1, 1:-1], 1, mode="edge")), name


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
    bc = ["--bc-x", "insulated", "--bc-y", "insulated"]
    if writer == "cli":
        w = subprocess.run([*cli, *bc, "--ntime", "12", "--checkpoint", "ck", "--output", "none"], cwd=tmp_path,
                           capture_output=True, text=True, timeout=300)
    else:
        w = py(tmp_path, *pyargs, *bc, "--ntime", "12", "--checkpoint", "ck", "--output", "none")
    assert w.returncode == 0, w.stdout + w.stderr
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    assert meta["bc_x"] == "insulated" and meta["bc_y"] == "insulated" and meta["step"] == 12
    if writer == "cli":  # resumed by the other driver, without the flags
        bad = py(tmp_path, *pyargs, "--restart", "ck", "--bc-y", "dirichlet")
        r = py(tmp_path, *pyargs, "--restart", "ck")
    else:
        bad = subprocess.run([*cli, "--restart", "ck", "--bc-y", "periodic"], cwd=tmp_path, capture_output=True,
                             text=True, timeout=300)
        r = subprocess.run([*cli, "--restart", "ck"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "conflicts with the checkpoint" in bad.stdout + bad.stderr
    assert r.returncode == 0, r.stdout + r.stderr
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    assert np.array_equal(read_soln(tmp_path / "soln00000.dat"), R.owned(R.ftcs(prob, **II)))


def test_raw_op_cpu(native):
    """The CPU raw op with bc = 4 | 8 on a 70 x 261 window: 20 fused levels = 20 golden steps."""
    import torch

    from heat2d.ops import kernels as K
    L = K.make_layout(70, 261, halo=24)
    f = torch.from_numpy(np.random.default_rng(3).random(L.elems()))
    own = K.view2d(f, L).numpy()[24:94, 32:32 + 261].copy()
    g = f.clone()
    K.tb_step(f, g, L, 20, 0.2371, arith="exact", **II)
    T = np.pad(own, 1, mode="edge")
    for _ in range(20):
        T = R.ftcs_step(T, 0.2371, **II)
    T = R.wrap_frame(T, *II.values())
    assert np.array_equal(K.view2d(g, L).numpy()[23:95, 31:32 + 262], T)  # the owned points and their images


# ------------------------------------------------------------------ GPU

@pytest.mark.gpu
@pytest.mark.parametrize("tb", [1, 4, 16, 17, 20, 24])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS, ids=IDS)
def test_hip_bitwise(native, gpu, bc_x, bc_y, dtype, tb):
    """Two cycles of depth tb and the remainder (tb 24: 24, 24, 9), asserted
    from cycle_hist() in run(): one step(57) call at tb 24 runs 19, 19, 19."""
    got = run(261, dtype, "hip", tb, bc_x, bc_y, prepare=True, calls=Y.calls(tb, STEPS, 2))
    assert np.array_equal(got, gold(261, dtype, bc_x, bc_y))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", COMBOS, ids=IDS)
def test_hip_single_call(native, gpu, bc_x, bc_y, dtype):
    """ONE step(57) call at tb 16: balanced cycles (15, 14, 14, 14) with insulated walls."""
    assert Y.balanced(16, STEPS) == [15, 14, 14, 14]
    got = run(261, dtype, "hip", 16, bc_x, bc_y, prepare=True)
    assert np.array_equal(got, gold(261, dtype, bc_x, bc_y))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_frame_images(native, gpu, dtype):
    """download_field() on the GPU: the frame holds the images after upload and after the march."""
    for bc_x, bc_y in COMBOS:
        s = HeatSolver(problem(261, STEPS), dtype=dtype, backend="hip", tb=20, arith="exact", device=0, bc_x=bc_x, bc_y=bc_y)
        T0 = rough_field(261, dtype)
        s.upload(T0)
        assert np.array_equal(s.download_field(), R.wrap_frame(T0, bc_x, bc_y)), (bc_x, bc_y)
        for m in Y.calls(20, STEPS, 2):
            s.step(m)
        assert np.array_equal(s.download_field(), gold(261, dtype, bc_x, bc_y, framed=True)), (bc_x, bc_y)
        hist = s.cycle_hist()
        s.close()
        Y.assert_ran(hist, 20, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_jacobi(native, gpu, dtype):
    """Hot-spot-like data at sigma = 0.25, against the jacobi golden."""
    got = run(261, dtype, "hip", 20, *II.values(), sigma=0.25, arith="jacobi", prepare=True, calls=Y.calls(20, STEPS, 2))
    assert np.array_equal(got, gold(261, dtype, *II.values(), sigma=0.25, arith="jacobi"))


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["fma", "auto"])
def test_hip_fma_and_auto(native, gpu, arith):
    """The contracted form against its CPU twin at r = 0.2371; auto resolves to exact there."""
    got = run(261, "fp64", "hip", 20, *II.values(), arith=arith, prepare=True, calls=Y.calls(20, STEPS, 2))
    if arith == "auto":
        assert np.array_equal(got, gold(261, "fp64", *II.values()))
    else:
        assert np.array_equal(got, run(261, "fp64", "cpu", 20, *II.values(), arith=arith))


@pytest.mark.gpu
def test_hip_refuses_fast(native, gpu):
    with pytest.raises(RuntimeError, match="insulated"):
        HeatSolver(problem(261, 4), backend="hip", device=0, arith="fast", bc_x="insulated")


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(graph=True), dict(autotune=1)], ids=["graph", "autotune"])
def test_hip_plan_variants(native, gpu, kw):
    got = run(261, "fp64", "hip", 8, *II.values(), prepare=True, **kw)
    assert np.array_equal(got, gold(261, "fp64", *II.values()))


def worker(tmp_path, a, **env):
    out = subprocess.run([sys.executable, os.path.join(HERE, "periodic_worker.py"), "single", str(tmp_path),
                          json.dumps(a)], env=dict(os.environ, HEAT2D_PLAN_CACHE="off", **env), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    return json.loads((tmp_path / "info.json").read_text())["plan"], np.load(tmp_path / "result.npy")


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["edge-first", "concurrent", "lead"])
def test_hip_split_orders(native, gpu, tmp_path, order):
    a = {"n": 261, "steps": STEPS, "tb": 8, "dtype": "fp64", **II}
    plan, got = worker(tmp_path, a, HEAT2D_SPLIT_ORDER=order)
    print(f"split order {order}: plan {plan}")
    assert np.array_equal(got, gold(261, "fp64", *II.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("nseg", [37, 200])
def test_hip_segment_plans(native, gpu, tmp_path, nseg):
    """HEAT2D_SEGMENTS: the interior launch as segment work items that cross
    strip ends — the frame-column strips carved out of it get their share."""
    a = {"n": 261, "steps": STEPS, "tb": 8, "dtype": "fp64", **II}
    plan, got = worker(tmp_path, a, HEAT2D_SEGMENTS=str(nseg))
    print(f"segments {nseg}: plan {plan}")
    assert np.array_equal(got, gold(261, "fp64", *II.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,n", [("fp64", 181), ("fp32", 213)])
def test_hip_narrow_last_strip(native, gpu, dtype, n):
    """Depth 20 with a last strip of 5 columns (fp64: 88 useful columns per
    strip, fp32: 208): narrower than the strip halo, so the strip before it
    reaches the frame column too and must not stay on the interior kernel."""
    got = run(n, dtype, "hip", 20, *II.values(), prepare=True, calls=Y.calls(20, STEPS, 2))
    assert np.array_equal(got, gold(n, dtype, *II.values()))


@pytest.mark.gpu
def test_hip_forced_pipe(native, gpu, tmp_path):
    """HEAT2D_PIPE=1 under insulated y: the wave-pair kernel's wide strips are
    not carved, so the plan falls back to the one-wave strips; the result is the golden's."""
    a = {"n": 700, "steps": STEPS, "tb": 20, "dtype": "fp64", **II}
    plan, got = worker(tmp_path, a, HEAT2D_PIPE="1")
    print(f"forced pipe, fully insulated: plan {plan}")
    assert np.array_equal(got, gold(700, "fp64", *II.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("overlap", [True, False])
@pytest.mark.parametrize("ranks", [2, 3])
def test_hip_loopback(native, gpu, ranks, overlap):
    for dtype in ("fp64", "fp32"):
        got = run(262, dtype, "hip", 20, *II.values(), ranks=ranks, overlap=overlap, calls=Y.calls(20, STEPS, 2))
        assert np.array_equal(got, gold(262, dtype, *II.values())), dtype


@pytest.mark.gpu
def test_hip_loopback_insulated_x_only(native, gpu):
    """3 ranks, x insulated and y Dirichlet: the first and last slab differ from the middle one."""
    got = run(262, "fp64", "hip", 20, "insulated", "dirichlet", ranks=3, calls=Y.calls(20, STEPS, 2))
    assert np.array_equal(got, gold(262, "fp64", "insulated", "dirichlet"))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_guard_nan_beyond_frame(native, gpu, dtype):
    """The allocation padding (IcSpec.pad: every pad column and ghost row beyond the frame) holds NaN."""
    p = problem(261, STEPS)
    p = dataclasses.replace(p, ic=dataclasses.replace(p.ic, pad=float("nan")))
    s = HeatSolver(p, dtype=dtype, backend="hip", tb=20, arith="exact", device=0, **II)
    s.upload(rough_field(261, dtype))
    for m in Y.calls(20, STEPS, 2):
        s.prepare(m)
        s.step(m)
    got, hist = s.download(), s.cycle_hist()
    Y.assert_ran(hist, 20, 2)
    L = s.layout
    out = np.empty((L.nrows + 2 * L.halo, L.pitch), dtype=NP[dtype])
    N.call("heat2d_solver_download_region", s._h, -L.halo, L.nrows + L.halo, -L.cpad, L.pitch - L.cpad,
           out.ctypes.data, L.pitch)
    s.close()
    assert np.isnan(out[:L.halo - 1, :]).all() and np.isnan(out[:, :L.cpad - 1]).all()  # the guard was in place
    assert np.isnan(out[L.halo + L.nrows + 1:, :]).all() and np.isnan(out[:, L.cpad + L.ncols + 1:]).all()
    assert not np.isnan(got).any()
    assert np.array_equal(got, gold(261, dtype, *II.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_step_stats(native, gpu, dtype):
    lo, hi = 0.0, float(np.log10(2.0))
    got, st = run(261, dtype, "hip", 20, *II.values(), lo=lo, hi=hi, stats=True, prepare=True, calls=Y.calls(20, STEPS, 2))
    g = gold(261, dtype, *II.values(), lo=lo, hi=hi)
    g1 = gold(261, dtype, *II.values(), steps=STEPS - 1, lo=lo, hi=hi)
    assert np.array_equal(got, g)
    g64, d = g.astype(np.float64), g.astype(np.float64) - g1.astype(np.float64)
    assert st["min"] == g64.min() and st["max"] == g64.max() and st["residual_max"] == np.abs(d).max()
    assert np.isclose(st["sum"], g64.sum(), rtol=1e-12, atol=0) and np.isclose(st["sum_sq"], (g64 * g64).sum(), rtol=1e-12)
    assert np.isclose(st["residual_l2"], np.sqrt((d * d).sum()), rtol=1e-10)
    conservation(R.owned(rough_field(261, dtype, lo=lo, hi=hi)), got, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_raw_op(native, gpu, dtype):
    """One tb_step launch with bc = 4 | 8 on a 70 x 261 window, against the CPU raw op."""
    import torch

    from heat2d.ops import kernels as K
    L = K.make_layout(70, 261, halo=24)
    host = (1.0 + np.random.default_rng(3).random(L.elems())).astype(NP[dtype])
    f = torch.from_numpy(host)
    want = f.clone()
    K.tb_step(f, want, L, 20, 0.2371, arith="exact", **II)
    fd = f.cuda()
    gd = fd.clone()
    K.tb_step(fd, gd, L, 20, 0.2371, arith="exact", **II)
    assert np.array_equal(gd.cpu().numpy(), want.numpy())  # owned points, frame images, and nothing else written
