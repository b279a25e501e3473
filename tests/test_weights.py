"""The constant-coefficient five-point operator, weights=(wS, wE, wN, wW, wC):
T' = wS*S + wE*E + wN*N + wW*W + wC*C (a moving medium, unequal diffusion numbers
on the two axes, a linear loss) — the golden (models.reference ftcs_step / ftcs /
probe_history weights=), the helper heat2d.weights_from, the CPU twin through
HeatSolver / LoopbackGroup / the raw ops, the refusals and the drivers'
checkpoints. No GPU needed; every comparison is bitwise.

The oracles need no tolerance: (1/4, 1/4, 1/4, 1/4, 0) is the jacobi form (products
by 1/4 are exact), a unit weight on one neighbour is a shift of the field, and the
two negative controls (wE and wW swapped: every point differs; the other arithmetic
form: more than half of the points differ) show that a bitwise match means something.
"""
import json
import math
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import heat2d
from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver, LoopbackGroup, weights_from
from heat2d.ops import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from weights_worker import BC_IDS, BCS, NP, ROUGH, bits, problem, signed_field  # noqa: E402

N77, STEPS = 77, 19
_GOLD = {}


def gold(n, dtype, arith, bc_x, bc_y, steps=STEPS, weights=ROUGH, framed=False):
    """The golden run from signed_field (computed once, read-only)."""
    key = (n, dtype, arith, bc_x, bc_y, steps, tuple(weights))
    if key not in _GOLD:
        g = np.ascontiguousarray(R.ftcs(problem(n, steps), steps, dtype=NP[dtype], T0=signed_field(n, dtype), arith=arith,
                                        bc_x=bc_x, bc_y=bc_y, weights=weights))
        g.setflags(write=False)
        _GOLD[key] = g
    return _GOLD[key] if framed else R.owned(_GOLD[key])


@pytest.fixture(scope="module", autouse=True)
def drop_goldens():
    yield
    _GOLD.clear()


def run_cpu(n, dtype, tb, arith, bc_x, bc_y, steps=STEPS, weights=ROUGH, ranks=1, T0=None, **kw):
    p = problem(n, steps)
    T0 = signed_field(n, dtype) if T0 is None else T0
    cls = (lambda *a, **k: LoopbackGroup(p, ranks, *a, **k)) if ranks > 1 else (lambda *a, **k: HeatSolver(p, *a, **k))
    s = cls(dtype=dtype, backend="cpu", tb=tb, arith=arith, bc_x=bc_x, bc_y=bc_y, weights=weights, **kw)
    s.upload(T0)
    s.step(steps)
    out = s.download()
    s.close()
    return out


# ------------------------------------------------------------------ the golden

@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", BCS, ids=BC_IDS)
def test_jacobi_identity(bc_x, bc_y, dtype, arith):
    """(1/4, 1/4, 1/4, 1/4, 0) has the bits of ftcs(arith="jacobi") at r = 1/4, in both forms."""
    T = J = signed_field(N77, dtype)
    for _ in range(8):
        T = R.ftcs_step(T, 0.0, arith, bc_x, bc_y, weights=(0.25, 0.25, 0.25, 0.25, 0.0))
        J = R.ftcs_step(J, 0.25, "jacobi", bc_x, bc_y)
    assert np.array_equal(bits(R.owned(T)), bits(R.owned(J)))


def shifted(F, steps, axis, periodic):
    """The owned points of the frame-inclusive F moved `steps` places toward increasing index along `axis`:
    a roll (periodic), or the roll with the pinned frame line fed in (Dirichlet)."""
    own = R.owned(F)
    if periodic:
        return np.roll(own, steps, axis=axis)
    out = np.empty_like(own)
    n = own.shape[axis]
    for k in range(n):
        src = k - steps  # owned index the value comes from; negative: the frame line
        sl = [slice(None), slice(None)]
        sl[axis] = k
        if axis == 0:
            out[tuple(sl)] = own[src, :] if src >= 0 else F[0, 1:-1]
        else:
            out[tuple(sl)] = own[:, src] if src >= 0 else F[1:-1, 0]
    return out


SHIFTS = {"columns": ((0, 0, 0, 1, 0), 1), "rows": ((0, 0, 1, 0, 0), 0)}  # T' = W / T' = N


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "dirichlet"])
@pytest.mark.parametrize("which", sorted(SHIFTS))
def test_shift_identity_golden(which, periodic):
    w, axis = SHIFTS[which]
    bc = ["dirichlet", "dirichlet"]
    if periodic:
        bc[axis] = "periodic"
    for dtype in ("fp64", "fp32"):
        T0 = signed_field(N77, dtype)
        for arith in ("exact", "fma"):
            got = R.owned(R.ftcs(problem(N77, 9), 9, dtype=NP[dtype], T0=T0, arith=arith, bc_x=bc[0], bc_y=bc[1], weights=w))
            assert np.array_equal(bits(got), bits(shifted(T0, 9, axis, periodic))), (dtype, arith)


@pytest.mark.parametrize("ranks", [1, 2, 3])
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "dirichlet"])
@pytest.mark.parametrize("which", sorted(SHIFTS))
def test_shift_identity_fused_passes(native, which, periodic, ranks):
    """Fused passes of depth 1, 4 and 8 on 1, 2 and 3 ranks: (0, 0, 0, 1, 0) moves every row one column per step,
    (0, 0, 1, 0, 0) the field one row per step — across the rank seams."""
    w, axis = SHIFTS[which]
    bc = ["dirichlet", "dirichlet"]
    if periodic:
        bc[axis] = "periodic"
    T0 = signed_field(N77, "fp64")
    want = shifted(T0, STEPS, axis, periodic)
    for tb in (1, 4, 8):
        for arith in ("exact", "fma"):
            got = run_cpu(N77, "fp64", tb, arith, bc[0], bc[1], weights=w, ranks=ranks)
            assert np.array_equal(bits(got), bits(want)), (tb, arith)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_negative_controls(dtype):
    """On rough weights, swapping wE and wW changes every point and the other arithmetic form more than half of
    them (measured: 100 % and 63-64 % at n = 77 over 8 steps, both axes periodic)."""
    kw = dict(steps=8, bc_x="periodic", bc_y="periodic")
    ref = gold(N77, dtype, "exact", kw["bc_x"], kw["bc_y"], steps=8)
    wS, wE, wN, wW, wC = ROUGH
    swapped = gold(N77, dtype, "exact", kw["bc_x"], kw["bc_y"], steps=8, weights=(wS, wW, wN, wE, wC))
    other = gold(N77, dtype, "fma", kw["bc_x"], kw["bc_y"], steps=8)
    f_swap, f_form = float((bits(ref) != bits(swapped)).mean()), float((bits(ref) != bits(other)).mean())
    print(f"{dtype}: wE/wW swapped differs at {100 * f_swap:.1f} %, the other form at {100 * f_form:.1f} % of the points")
    assert f_swap > 0.5 and f_form > 0.5


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_conservation_and_decay(dtype, arith):
    """Both axes periodic: with sum(w) == 1 the total heat moves per step by at most 8 u n^2 max|T|, and with a
    decay it falls by the factor sum(w) = 1 - decay*dt per step within the same bound. (The exact weighted sums
    of all points add up to sum(w) times the total; a point's rounding error is below 5 u max|T|: the products'
    errors are below u w_i max|T| and add up to u max|T| for positive weights with sum <= 1, the four sums' are
    below u max|T| each; fma: one product and four fmas.)"""
    u = float(np.finfo(NP[dtype]).eps) / 2
    n = N77
    for w in ((0.125, 0.0625, 0.25, 0.1875, 0.375), (0.125, 0.0625, 0.25, 0.1875, 0.375 - 0.015625)):
        factor = math.fsum(w)  # (dyadic: exact in both dtypes)
        assert factor in (1.0, 1.0 - 0.015625)
        T = signed_field(n, dtype)
        for _ in range(8):
            before, tmax = math.fsum(R.owned(T).ravel().tolist()), float(np.abs(R.owned(T)).max())
            T = R.ftcs_step(T, 0.0, arith, "periodic", "periodic", weights=w)
            after = math.fsum(R.owned(T).ravel().tolist())
            assert abs(after - factor * before) <= 8 * u * n * n * tmax, (w, after, before)


def test_weights_from_by_hand():
    p = problem(101, 1, sigma=0.2)  # dx = 0.01, nu = 0.05: dt = 0.2 dx^2 / nu = 4e-4, r = 0.2
    dt, dx = p.dt, p.delta
    assert weights_from(p) == pytest.approx((0.2, 0.2, 0.2, 0.2, 0.2), rel=1e-14)
    rx, ry = 0.05 * dt / dx ** 2, 0.02 * dt / dx ** 2
    cx, cy = 1.5 * dt / dx, 0.5 * dt / dx
    # upwind, positive velocities: the upstream neighbours are N (row i - 1) and W (column j - 1)
    w = weights_from(p, nu_y=0.02, vx=1.5, vy=0.5)
    assert w[:4] == (rx, ry, rx + cx, ry + cy) and w[4] == 1.0 - (rx + ry + (rx + cx) + (ry + cy))
    # negative velocities: S and E
    w = weights_from(p, nu_y=0.02, vx=-1.5, vy=-0.5)
    assert w[:4] == (rx + cx, ry + cy, rx, ry)
    # central, with a decay
    w = weights_from(p, nu_x=0.05, nu_y=0.02, vx=1.5, vy=-0.5, decay=3.0, scheme="central")
    assert w[:4] == (rx - cx / 2, ry + cy / 2, rx + cx / 2, ry - cy / 2)
    assert w[4] == 1.0 - (w[0] + w[1] + w[2] + w[3]) - 3.0 * dt
    assert all(isinstance(x, float) for x in w)
    with pytest.raises(ValueError, match="scheme"):
        weights_from(p, scheme="lax")


# ------------------------------------------------------------------ the CPU twin

@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("bc_x,bc_y", BCS, ids=BC_IDS)
def test_cpu_twin_bitwise(native, bc_x, bc_y, dtype, arith):
    """Depths 1..8 on 1, 2 and 3 ranks at n = 77 against the golden."""
    want = gold(N77, dtype, arith, bc_x, bc_y)
    for ranks in (1, 2, 3):
        for tb in range(1, 9):
            got = run_cpu(N77, dtype, tb, arith, bc_x, bc_y, ranks=ranks)
            assert np.array_equal(bits(got), bits(want)), (ranks, tb)


def test_auto_is_fma_info_and_set_weights(native):
    """arith "auto" runs fma; info()["weights"]; set_weights() between steps takes effect; None returns to the
    scalar-r run's bits; a negative weight warns."""
    p, T0 = problem(N77, STEPS), signed_field(N77, "fp32")
    s = HeatSolver(p, dtype="fp32", backend="cpu", tb=5, weights=ROUGH)
    info = s.info()
    conv = tuple(float(np.float32(x)) for x in ROUGH)
    assert info["arith"] == N.ARITH["fma"] and info["weights"] == {"set": True, "values": conv, "max_tb": N.max_tb_w5()}
    assert s.weights == conv
    s.upload(T0)
    s.step(7)
    other = (0.2, 0.05, 0.3, 0.1, 0.3)
    s.set_weights(other)
    s.step(6)
    s.set_weights(None)
    assert s.info()["weights"] == {"set": False, "values": None, "max_tb": N.max_tb_w5()} and s.weights is None
    s.step(6)
    got = s.download()
    arith_plain = s.info()["arith"]
    s.close()
    T = R.ftcs(p, 7, dtype=np.float32, T0=T0, arith="fma", weights=ROUGH)
    T = R.ftcs(p, 6, dtype=np.float32, T0=T, arith="fma", weights=other)
    plain = HeatSolver(p, dtype="fp32", backend="cpu", tb=5)
    assert plain.info()["arith"] == arith_plain  # (auto without weights: the solver's own choice again)
    plain.upload(T)
    plain.step(6)
    want = plain.download()
    plain.close()
    assert np.array_equal(bits(got), bits(want))
    with pytest.warns(RuntimeWarning, match="negative weight wE"):
        HeatSolver(p, backend="cpu", weights=(0.3, -0.05, 0.3, 0.2, 0.25)).close()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        HeatSolver(p, backend="cpu", weights=ROUGH).close()


def test_step_stats_takes_the_unfused_path(native):
    p, T0 = problem(N77, STEPS), signed_field(N77, "fp64")
    s = HeatSolver(p, backend="cpu", tb=6, arith="exact", weights=ROUGH)
    s.upload(T0)
    st = s.step_stats(STEPS)
    got = s.download()
    s.close()
    want = gold(N77, "fp64", "exact", "dirichlet", "dirichlet")
    assert np.array_equal(bits(got), bits(want))
    assert st["min"] == float(want.min()) and st["max"] == float(want.max())


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_probes(native, dtype, arith):
    """The history equals probe_history(weights=), probes on the first and last owned row and column, under
    Dirichlet and under periodic axes; the last row of the call equals download() at the probes."""
    n = N77
    pts = np.array([[1, 1], [1, 40], [77, 77], [30, 1], [52, 77], [40, 40], [77, 2]])
    for bc_x, bc_y in BCS:
        s = HeatSolver(problem(n, STEPS), dtype=dtype, backend="cpu", tb=7, arith=arith, bc_x=bc_x, bc_y=bc_y,
                       weights=ROUGH, probes=pts, probe_steps=STEPS)
        s.upload(signed_field(n, dtype))
        s.step(STEPS)
        H, out = s.probe_history(), s.download()
        s.close()
        want = R.probe_history(problem(n, STEPS), STEPS, pts, dtype=NP[dtype], T0=signed_field(n, dtype), arith=arith,
                               bc_x=bc_x, bc_y=bc_y, weights=ROUGH)
        assert np.array_equal(bits(H), bits(want)), (bc_x, bc_y)
        assert np.array_equal(H[-1], out[pts[:, 0] - 1, pts[:, 1] - 1])


def raw_window(dtype, seed=3):
    """The raw ops' shape: a window of 70 rows x 261 columns, rough signed data in the whole allocation."""
    from heat2d.ops import kernels as K
    L = K.make_layout(70, 261, halo=24)
    rng = np.random.default_rng(seed)
    host = (10.0 ** rng.uniform(-1, 1, L.elems()) * rng.choice([-1.0, 1.0], L.elems())).astype(NP[dtype])
    return K, L, host


@pytest.mark.parametrize("arith", ["exact", "fma"])
def test_raw_op_cpu(native, arith):
    """The CPU raw op on a 70 x 261 window: 20 fused levels are 20 golden steps; the raw probe cone agrees."""
    import torch
    K, L, host = raw_window("fp64")
    f = torch.from_numpy(host)
    g = f.clone()
    K.tb_step(f, g, L, 20, 0.0, arith=arith, weights=ROUGH)
    T = K.view2d(f, L).numpy()[23:95, 31:32 + 262].copy()  # the owned points with their frame
    hist = []
    pts = np.array([[1, 1], [70, 261], [35, 1], [1, 100]])
    for _ in range(20):
        T = R.ftcs_step(T, 0.0, arith, weights=ROUGH)
        hist.append(T[pts[:, 0], pts[:, 1]])
    assert np.array_equal(K.view2d(g, L).numpy()[23:95, 31:32 + 262], T)
    H = K.probe_cone(f, L, 20, 0.0, pts, arith=arith, weights=ROUGH)
    assert np.array_equal(H.numpy(), np.array(hist))


# ------------------------------------------------------------------ refusals

def test_refusals_golden():
    T = signed_field(20, "fp64")
    z = np.zeros_like(T)
    for kw in (dict(bc_x="insulated"), dict(bc_y="insulated"), dict(bc_x="robin", robin={"x_lo": (1, 0), "x_hi": (1, 0)}),
               dict(bc_y="robin"), dict(source=z), dict(rmap=z), dict(faces=(z, z)), dict(source=z, gain=1.0),
               dict(arith="jacobi"), dict(arith="fast")):
        with pytest.raises(ValueError):
            R.ftcs_step(T, 0.25, **{"arith": "exact", **kw}, weights=ROUGH)
    p = problem(20, 4)
    for kw in (dict(source=z, source_gain=np.ones(4)), dict(source=z), dict(rmap=z), dict(faces=(z, z)), dict(bc_x="insulated"),
               dict(arith="jacobi")):
        with pytest.raises(ValueError):
            R.ftcs(p, 4, T0=T, weights=ROUGH, **kw)
        with pytest.raises(ValueError):
            R.probe_history(p, 4, np.array([[1, 1]]), T0=T, weights=ROUGH, **kw)
    for bad in ((1, 2, 3, 4), (1, 2, 3, 4, 5, 6), (0.1, 0.1, float("nan"), 0.1, 0.1), (0.1, float("inf"), 0.1, 0.1, 0.1), 0.25):
        with pytest.raises(ValueError, match="weights"):
            R.ftcs_step(T, 0.25, weights=bad)
    with pytest.raises(ValueError, match="finite"):
        R.ftcs_step(T.astype(np.float32), 0.25, weights=(1e39, 0, 0, 0, 0))  # (finite in fp64, not in the run's dtype)


def test_refusals_solver(native):
    p = problem(40, 4)
    z = np.zeros((42, 42))
    cases = [dict(arith="jacobi"), dict(arith="fast"), dict(engine="jit"), dict(copy_swap=True), dict(bc_x="insulated"),
             dict(bc_y="insulated"), dict(bc_x="robin", robin={"x_lo": (1, 0), "x_hi": (1, 0)}),
             dict(bc_y="robin", robin={"y_lo": (1, 0), "y_hi": (1, 0)}), dict(source=z), dict(rmap=z), dict(faces=(z, z)),
             dict(source=z, source_gain=np.ones(4))]
    for kw in cases:
        with pytest.raises(RuntimeError, match="weights"):
            HeatSolver(p, backend="cpu", weights=ROUGH, **kw)
    for kw in cases:
        if "engine" in kw or "copy_swap" in kw:
            continue
        with pytest.raises(RuntimeError, match="weights"):
            LoopbackGroup(p, 2, backend="cpu", weights=ROUGH, **kw)
    with pytest.raises(ValueError, match="5-tuple"):
        HeatSolver(p, backend="cpu", weights=(0.1, 0.2, 0.3))
    with pytest.raises(ValueError, match="finite"):
        HeatSolver(p, backend="cpu", weights=(0.1, 0.2, float("nan"), 0.1, 0.1))
    # the native solver's own refusals (Solver::set_weights), past the Python layer's
    import ctypes as C
    arr = (C.c_double * 5)(*ROUGH)
    for kw, phrase in ((dict(bc_x="insulated"), "Dirichlet or periodic"), (dict(source=z), "heat source"),
                       (dict(arith="jacobi"), "jacobi / fast"), (dict(copy_swap=True), "copy-swap")):
        s = HeatSolver(problem(49, 4, sigma=0.25), backend="cpu", **({k: (np.zeros((51, 51)) if k == "source" else v)
                                                                      for k, v in kw.items()}))
        with pytest.raises(N.NativeError, match=phrase):
            N.call("heat2d_solver_set_weights", s._h, arr)
        s.close()
    s = HeatSolver(p, backend="cpu")
    bad = (C.c_double * 5)(0.1, 0.2, float("inf"), 0.1, 0.1)
    with pytest.raises(N.NativeError, match="finite"):
        N.call("heat2d_solver_set_weights", s._h, bad)
    s.close()


def test_refusals_raw_op(native):
    import torch
    K, L, host = raw_window("fp64")
    f = torch.from_numpy(host)
    g = f.clone()
    pts = np.array([[1, 1]])
    rob = {"x_lo": (1, 0), "x_hi": (1, 0)}
    for kw in (dict(source=f.clone()), dict(rmap=f.clone()), dict(faces=(f.clone(), f.clone())), dict(robin=rob),
               dict(source=f.clone(), gain=torch.ones(8, dtype=torch.float64)), dict(bc_x="insulated"), dict(bc_y="robin"),
               dict(arith="jacobi"), dict(arith="fast")):
        with pytest.raises((ValueError, RuntimeError), match="weights"):
            K.tb_step(f, g, L, 4, 0.25, weights=ROUGH, **kw)
        with pytest.raises((ValueError, RuntimeError), match="weights"):
            K.probe_cone(f, L, 4, 0.25, pts, weights=ROUGH, **kw)
    with pytest.raises(ValueError, match="5-tuple"):
        K.tb_step(f, g, L, 4, 0.25, weights=(1, 2))
    assert torch.equal(g, f)  # nothing ran


# ------------------------------------------------------------------ drivers and checkpoints

def py(cwd, *args):
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2")
    return subprocess.run([sys.executable, "-m", "heat2d", *args], cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=300)


def cli(cwd, *args):
    return subprocess.run([N.CLI_PATH, "--cpu", *args], cwd=cwd, capture_output=True, text=True, timeout=300)


FLAG = "--weights=" + ",".join(repr(w) for w in ROUGH)


def driver(which):
    """(run, the flags both drivers share) of the native CLI or the Python driver, on the CPU twin in fp32."""
    base = ["--ic", "hat-cuda", "--quiet", "--dtype", "fp32", "--bc-y", "periodic"]
    return (cli, base) if which == "cli" else (py, ["--backend", "cpu", *base])


@pytest.mark.parametrize("writer", ["cli", "py"])
def test_checkpoint_written_by_one_driver_resumed_by_the_other(native, tmp_path, writer):
    """meta.json records the converted five values as hex floats under "weights"; the other driver's restart
    takes them from there and reaches the golden bitwise (auto: fma). A contradicting --weights fails before the
    first step in either driver, and so does --weights on a checkpoint written without (the key is missing
    there); the same flag again does not. A solver without weights does not load a checkpoint that has them."""
    from heat2d.utils import checkpoint, io
    (tmp_path / "input.dat").write_text("50 0.2371 0.05 1.0 30 1\n")
    (wrun, wbase), (rrun, rbase) = driver(writer), driver("py" if writer == "cli" else "cli")
    w = wrun(tmp_path, *wbase, FLAG, "--ntime", "12", "--checkpoint", "ck", "--output", "none")
    assert w.returncode == 0, w.stdout + w.stderr
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    f32 = np.float32
    assert meta["step"] == 12 and checkpoint.weights_from_meta(meta) == tuple(float(f32(x)) for x in ROUGH)
    assert len(meta["weights"]) == 5 and all(v.lstrip("-").startswith("0x") for v in meta["weights"])
    plain = wrun(tmp_path, *wbase, "--ntime", "12", "--checkpoint", "ck0", "--output", "none")
    assert plain.returncode == 0, plain.stdout + plain.stderr
    with open(tmp_path / "ck0" / "latest") as f:
        assert "weights" not in json.loads((tmp_path / "ck0" / f.read().strip() / "meta.json").read_text())
    for run, base in ((rrun, rbase), (wrun, wbase)):
        bad = run(tmp_path, *base, "--restart", "ck", "--weights", "0.11,0.07,0.23,0.19,0.36", "--output", "none")
        assert bad.returncode != 0 and "conflicts with the checkpoint" in bad.stdout + bad.stderr
        assert "time_it" not in bad.stdout
        bad = run(tmp_path, *base, "--restart", "ck0", FLAG, "--output", "none")
        assert bad.returncode != 0 and "conflicts with the checkpoint" in bad.stdout + bad.stderr
    same = rrun(tmp_path, *rbase, "--restart", "ck", FLAG, "--output", "none")
    assert same.returncode == 0, same.stdout + same.stderr
    r = rrun(tmp_path, *rbase, "--restart", "ck")
    assert r.returncode == 0, r.stdout + r.stderr
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    ref = R.owned(R.ftcs(prob, dtype=f32, arith="fma", bc_y="periodic", weights=ROUGH))
    assert np.array_equal(io.read_xyz(str(tmp_path / "soln00000.dat"))[2].astype(f32), ref)
    assert not np.array_equal(ref, R.owned(R.ftcs(prob, dtype=f32, arith="exact", bc_y="periodic", weights=ROUGH)))
    s = HeatSolver(prob, dtype="fp32", backend="cpu", bc_y="periodic")
    with pytest.raises(ValueError, match="written with weights"):
        checkpoint.load(s, str(tmp_path / "ck"))
    s.close()


@pytest.mark.parametrize("which", ["cli", "py"])
def test_driver_flags(native, tmp_path, which):
    """Either driver: four numbers, jacobi, an insulated axis and --rmap beside --weights fail before the first
    step; a negative weight draws the warning; exact runs the exact golden."""
    from heat2d.utils import io
    (tmp_path / "input.dat").write_text("49 0.25 0.05 1.0 9 1\n")
    run, base = driver(which)
    short = run(tmp_path, *base, "--weights", "0.1,0.2,0.3,0.4", "--output", "none")
    assert short.returncode != 0 and "five numbers" in short.stdout + short.stderr
    jac = run(tmp_path, *base, FLAG, "--arith", "jacobi", "--output", "none")
    assert jac.returncode != 0 and "weights" in jac.stdout + jac.stderr
    ins = run(tmp_path, *base, FLAG, "--bc-x", "insulated", "--output", "none")
    assert ins.returncode != 0 and "weights" in ins.stdout + ins.stderr
    np.save(tmp_path / "m.npy", np.full((51, 51), 0.2))
    dirichlet = [f for f in base if f not in ("--bc-y", "periodic")]  # (a map needs Dirichlet axes: the weights are its one conflict)
    both = run(tmp_path, *dirichlet, FLAG, "--rmap", "m.npy", "--output", "none")
    assert both.returncode != 0 and "weights" in both.stdout + both.stderr
    noisy = [f for f in base if f != "--quiet"]
    warn = run(tmp_path, *noisy, "--weights=-0.01,0.07,0.23,0.19,0.37", "--output", "none")
    assert warn.returncode == 0 and "negative weight wS" in warn.stderr, warn.stdout + warn.stderr
    quiet = run(tmp_path, *noisy, FLAG, "--output", "none")
    assert quiet.returncode == 0 and "negative weight" not in quiet.stderr, quiet.stdout + quiet.stderr
    ex = run(tmp_path, *base, FLAG, "--arith", "exact")
    assert ex.returncode == 0, ex.stdout + ex.stderr
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    ref = R.owned(R.ftcs(prob, dtype=np.float32, arith="exact", bc_y="periodic", weights=ROUGH))
    assert np.array_equal(io.read_xyz(str(tmp_path / "soln00000.dat"))[2].astype(np.float32), ref)
