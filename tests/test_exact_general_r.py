"""Reference rounding (``arith="exact"``, SolverConfig::arith 0) at r != 1/4:
the update c + r*(((S + E) + N) + W - 4c) with every operation rounded, on the
CPU twin and on every gfx950 kernel that carries the form — what ``auto``
runs for every input whose r is not a power of two. At r = 1/4 (the rest of
the GPU suite) r*x is exact, so a kernel whose update got contracted to
fma(r, x, c), or that took r in another precision, would pass there; here it
fails.

Oracle: models.reference.ftcs(arith="exact") in the test's own dtype from the
uploaded rough field (default_rng(0).random), compared with np.array_equal.

Power condition: every bitwise test first takes the CPU twin's arith="fma"
field from the same T0 (the contracted comparator) and asserts that it differs
from the golden in more than 1 % of the owned points (POWER) — a property of
the inputs and the reference alone, so a contracted kernel cannot pass.
Measured shares (exact golden vs contracted twin, percent of owned points):


                             sigma 0.1    0.2   0.2371    0.3
  301^2, one step      fp32     8.65  14.22   16.33   20.69
                       fp64    10.98  13.72   13.94   17.60
  97^2, 51 steps       fp32     5.85   9.87   16.14   84.65
                       fp64    12.34   8.22   16.41   83.80
  301^2, depth 16      fp32     7.17  10.64   16.40   85.06   (35 steps)
  301^2, depth 12      fp64     9.53  10.43   18.25   84.61   (27 steps)
  301^2, sigma 0.2, 5 .. 51 steps: fp32 13.31 .. 9.42, fp64 14.62 .. 9.33
    (the share falls slowly as the field smooths; the lowest is the deepest)
  1100^2 .. 1500^2, sigma 0.2, 23 .. 65 steps: fp32 10.13 .. 9.12,
    fp64 10.47 .. 9.19
  n = 777, "sigma 0.25" (r = 0.25 - 2^-55), 19 steps: fp64 24.84, fp32 0
  257^2, 9 steps (jit): sigma 0.2 12.68 / 12.68, 0.2371 24.27 / 23.63 (fp32 / fp64)
  203^2, 8 steps (raw op): fp32 11.66, fp64 13.14

Two cases cannot meet the condition and are exempt, each for a stated reason:
  * sigma = 0.125 (r a power of two): contracted and rounded forms are the same
    bits, and the test asserts exactly that on the GPU;
  * n = 777 in fp32: np.float32(r) == 0.25 although r != 0.25 in double, so the
    fp32 forms are the same bits too (asserted: the comparator equals the
    golden); the case still checks that ``auto`` resolves from the double r to
    form 0 and that the fp32 form-0 kernel gives the golden.
"""
import os
import re
import sys

import numpy as np
import pytest

import heat2d
from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver, LoopbackGroup
from heat2d.ops import _native as N

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cycles as Y  # noqa: E402

POWER = 0.01
SIGMAS = [0.1, 0.2, 0.2371, 0.3]
NP = {"fp64": np.float64, "fp32": np.float32}


def prob(n, steps, conv="ghost", ic="sine", sigma=0.25, dom=1.0):
    return heat2d.make_problem(heat2d.InputDat(n=n, sigma=sigma, nu=0.05, dom_len=dom, ntime=steps), conv, ic)


def rough(p, npdt, seed=0):
    return np.random.default_rng(seed).random((p.n_owned, p.n_owned)).astype(npdt)


def golden(p, npdt, T0=None, arith="exact", steps=None):
    full = None
    if T0 is not None:
        full = R.initial_field(p, npdt)
        full[1:-1, 1:-1] = T0
    return R.owned(R.ftcs(p, steps, dtype=npdt, T0=full, arith=arith))


def run(p, backend, dtype, tb, arith="exact", upload=None, steps=None, full=0, **kw):
    """full > 0: the steps as tests/cycles.py calls(tb, steps, full) — `full`
    cycles of depth tb, asserted from cycle_hist(), then the remainder — and
    not as one step() call, whose balanced cycles are all shallower than tb."""
    s = HeatSolver(p, dtype=dtype, backend=backend, tb=tb, arith=arith, device=0 if backend == "hip" else None, **kw)
    if upload is not None:
        s.upload(upload)
    steps = p.ntime if steps is None else steps
    for m in Y.calls(tb, steps, full) if full else [steps]:
        s.step(m)
    out, hist = s.download(), s.cycle_hist()
    s.close()
    if full:
        Y.assert_ran(hist, tb, full)
    return out


def solve(c, dtype, tb, **kw):
    """c's problem on the HIP engine in form 0 from c.T0: (field, plan of depth
    tb). Two cycles of depth tb ran that plan, asserted from cycle_hist():
    step(tb), step(tb), the remainder — or, with graph=True, one call whose
    pair branch replays the captured pair of depth tb."""
    s = HeatSolver(c.p, dtype=dtype, backend="hip", tb=tb, device=0, arith="exact", **kw)
    s.upload(c.T0)
    for m in [c.p.ntime] if kw.get("graph") else Y.calls(tb, c.p.ntime, 2):
        s.step(m)
    got, hist = s.download(), s.cycle_hist()
    pl = s.plan(tb)
    s.close()
    Y.assert_ran(hist, tb, 2)
    return got, pl


class Case:
    """One (n, sigma, dtype, steps): the problem, the rough T0, the exact golden
    after ``steps`` (and after every step count in ``snaps``) and the share of
    owned points at which the contracted CPU twin differs from it."""

    def __init__(self, n, sigma, dtype, steps, snaps=()):
        self.p = prob(n, steps, sigma=sigma)
        self.npdt = NP[dtype]
        self.T0 = rough(self.p, self.npdt)
        self.T0.setflags(write=False)
        T = R.initial_field(self.p, self.npdt)
        T[1:-1, 1:-1] = self.T0
        self.at, done = {}, 0
        for k in sorted(set(snaps) | {steps}):
            T = R.ftcs(self.p, k - done, dtype=self.npdt, T0=T, arith="exact")
            done = k
            self.at[k] = R.owned(T).copy()
            self.at[k].setflags(write=False)
        self.gold = self.at[steps]
        fma = run(self.p, "cpu", dtype, 8, arith="fma", upload=self.T0, steps=steps)
        self.share = float(np.mean(fma != self.gold))

    def powered(self):
        """The power condition: a contracted kernel would differ from the golden."""
        print(f"contracted twin differs from the exact golden at {100 * self.share:.2f} % of the points")
        assert self.share > POWER, self.share
        return self


_CASES = {}


def case(n, sigma, dtype, steps, snaps=()):
    key = (n, sigma, dtype, steps, tuple(snaps))
    if key not in _CASES:
        _CASES[key] = Case(n, sigma, dtype, steps, snaps)
    return _CASES[key]


@pytest.fixture(scope="module", autouse=True)
def drop_cases():
    yield
    _CASES.clear()  # the 1100^2 .. 1500^2 fields are not kept for the rest of the session


# ------------------------------------------------------------------ CPU tier

@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("tb", [1, 5, 12, 24])
def test_cpu_exact_general_r(native, dtype, sigma, tb):
    c = case(97, sigma, dtype, 51).powered()
    assert N.arith_code("auto", c.p.r) == 0
    got = run(c.p, "cpu", dtype, tb, upload=c.T0)
    assert np.array_equal(got, c.gold)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_exact_one_step(native, dtype):
    """One step at 301^2, every sigma (the first row of the docstring's table)."""
    for sigma in SIGMAS:
        c = case(301, sigma, dtype, 1).powered()
        assert np.array_equal(run(c.p, "cpu", dtype, 1, upload=c.T0), c.gold)


def case777(dtype):
    """sigma = 0.25 at n = 777: r = 0.25 - 2^-55 in double, not a power of two
    (auto -> form 0, jacobi refused), and 0.25 exactly once rounded to fp32."""
    c = case(777, 0.25, dtype, 19)
    assert c.p.r != 0.25 and np.float32(c.p.r) == 0.25
    assert N.arith_code("auto", c.p.r) == 0
    if dtype == "fp64":
        c.powered()
    else:
        assert c.share == 0.0  # fp32: r rounds to 1/4, both forms are the same bits (exempt, see the docstring)
    return c


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_exact_777_sigma_quarter(native, dtype):
    c = case777(dtype)
    with pytest.raises(Exception, match="1/4"):
        HeatSolver(c.p, backend="cpu", arith="jacobi")
    s = HeatSolver(c.p, dtype=dtype, backend="cpu", tb=8)  # default arith
    assert s.info()["arith"] == 0
    s.upload(c.T0)
    s.step(c.p.ntime)
    got = s.download()
    s.close()
    assert np.array_equal(got, c.gold)


def test_cpu_exact_three_ranks(native):
    c = case(97, 0.2, "fp32", 51).powered()
    g = LoopbackGroup(c.p, 3, dtype="fp32", backend="cpu", tb=5, arith="exact")
    g.upload(c.T0)
    g.step(c.p.ntime)
    got = g.download()
    g.close()
    assert np.array_equal(got, c.gold)


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("sigma", SIGMAS)
def test_cpu_auto_resolves_to_exact(native, dtype, sigma):
    c = case(97, sigma, dtype, 51).powered()
    assert N.arith_code("auto", c.p.r) == 0
    s = HeatSolver(c.p, dtype=dtype, backend="cpu", tb=5)
    assert s.arith == "auto" and s.info()["arith"] == 0
    s.upload(c.T0)
    s.step(c.p.ntime)
    got = s.download()
    s.close()
    assert np.array_equal(got, c.gold)
    g = LoopbackGroup(c.p, 3, dtype=dtype, backend="cpu", tb=5)
    assert [g.arith_code(i) for i in range(3)] == [0, 0, 0]
    g.close()


def r_literal(src):
    m = re.search(r"#define R \((\S+?)(f?)\)\n", src)
    return float.fromhex(m.group(1)), m.group(2)


@pytest.mark.parametrize("n,sigma", [(257, s) for s in SIGMAS] + [(777, 0.25)])
def test_jit_r_literal_is_exact(native, n, sigma):
    """The r baked into the run-time-compiled source parses back to exactly the
    dtype's r: float(r) for fp32 (suffix f), r itself for fp64."""
    from heat2d.ops import jit
    p = prob(n, 1, sigma=sigma)
    L = N.make_layout(p.n_owned, p.n_owned, halo=16)
    v, suffix = r_literal(jit.render(N.F32, L, p.r, "exact"))
    assert suffix == "f" and v == float(np.float32(p.r))
    v, suffix = r_literal(jit.render(N.F64, L, p.r, "exact"))
    assert suffix == "" and v == p.r
    assert "#define UPDATE(c, sum) ((c) + R * ((sum) - FOUR * (c)))" in jit.render(N.F64, L, p.r, "auto")


# ------------------------------------------------------------------ GPU tier

EDGE_CASES = ([("fp64", tb, 0.2) for tb in (1, 4, 12, 16, 17, 20, 24)] +
              [("fp32", tb, 0.2) for tb in (1, 7, 16, 18, 20, 22, 24)] +
              [(dt, tb, s) for s in (0.1, 0.2371, 0.3) for dt, tb in (("fp64", 12), ("fp32", 16))])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tb,sigma", EDGE_CASES)
def test_hip_exact_every_edge_kind(gpu, native, dtype, tb, sigma):
    """Every edge kind (frame rows, frame columns, corners, interior) of the
    general kernel on a small odd grid, rough data, every depth class. (fp32
    at n = 517: its 256-column strips have none clear of both frame columns
    below n = 500, tests/instance_matrix.py.)"""
    c = case(301 if dtype == "fp64" else 517, sigma, dtype, 2 * tb + 3).powered()
    got = run(c.p, "hip", dtype, tb, upload=c.T0, full=2)  # step(tb), step(tb), step(3)
    assert np.array_equal(got, c.gold), np.abs(got.astype(np.float64) - c.gold).max()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_exact_777_sigma_quarter(gpu, native, dtype):
    """A shipped-looking input (sigma = 0.25) whose r is not 1/4: the default
    arith resolves to form 0 and gives the golden."""
    c = case777(dtype)
    s = HeatSolver(c.p, dtype=dtype, backend="hip", tb=8, device=0)  # default arith
    assert s.info()["arith"] == 0
    s.upload(c.T0)
    s.step(c.p.ntime)
    got = s.download()
    s.close()
    assert np.array_equal(got, c.gold), np.abs(got.astype(np.float64) - c.gold).max()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tb,n", [("fp64", 12, 1100), ("fp64", 20, 1500), ("fp32", 10, 1100),
                                        ("fp32", 16, 1300), ("fp32", 24, 1300)])
def test_hip_exact_split_schedule(gpu, native, monkeypatch, dtype, tb, n):
    """Split (MAIN + EDGE) schedule: the interior kernels, rings 4 and 6, the
    priming skip. The autotuner's own choice first: on one rank, with no
    exchange to hide, it may time a single general launch faster and keep it
    (valid 2), so what it chose is not asserted. Then the planned split it
    starts from (autotune=0) with either ring forced, which is a split plan
    by construction: asserted, so the interior kernels of both rings run
    whatever the tuner measured."""
    c = case(n, 0.2, dtype, 2 * tb + 3).powered()
    got, pl = solve(c, dtype, tb, autotune=1)
    assert pl["valid"] in (1, 2, 3) and pl["origin"] == "tuned", pl
    assert np.array_equal(got, c.gold), pl
    for ring in (4, 6):
        monkeypatch.setenv("HEAT2D_TB_RING", str(ring))
        got, pl = solve(c, dtype, tb, autotune=0)
        assert pl["valid"] in (1, 3) and pl["main_items"] > 0 and pl["edge_items"] > 0, pl
        assert pl["ring"] == (4 if dtype == "fp32" and tb > 16 else ring), pl  # fp32 above depth 16 has ring 4 only
        assert np.array_equal(got, c.gold), pl


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tb,n", [("fp64", 20, 1100), ("fp32", 16, 1100)])
def test_hip_exact_no_overlap(gpu, native, dtype, tb, n):
    """overlap=False: the single-launch general kernel over the whole slab."""
    c = case(n, 0.2, dtype, 2 * tb + 3).powered()
    got = run(c.p, "hip", dtype, tb, upload=c.T0, autotune=1, overlap=False)
    assert np.array_equal(got, c.gold)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,ring,tb", [("fp64", 4, 12), ("fp64", 6, 12), ("fp32", 4, 15), ("fp32", 6, 15),
                                           ("fp32", 8, 15)])
def test_hip_exact_forced_ring(gpu, native, monkeypatch, dtype, ring, tb):
    """Each load-ring instantiation of the general kernel, single launch."""
    monkeypatch.setenv("HEAT2D_SPLIT_ORDER", "single")
    monkeypatch.setenv("HEAT2D_TB_RING", str(ring))
    monkeypatch.setenv("HEAT2D_SEGMENTS", "44")
    c = case(1100, 0.2, dtype, 2 * tb + 3).powered()
    got, pl = solve(c, dtype, tb, autotune=0)
    assert pl["order"] == "single" and pl["ring"] == ring, pl
    assert np.array_equal(got, c.gold)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tb,order,nseg", [("fp64", 20, "concurrent", 500), ("fp32", 16, "single", 300)])
def test_hip_exact_dynamic_queue(gpu, native, monkeypatch, dtype, tb, order, nseg):
    """Dynamic item queue, several cycles, graph replays (test_jacobi's
    test_hip_dynamic_queue shape) in form 0."""
    monkeypatch.setenv("HEAT2D_SPLIT_ORDER", order)
    monkeypatch.setenv("HEAT2D_DYNAMIC", "1")
    monkeypatch.setenv("HEAT2D_SEGMENTS", str(nseg))
    monkeypatch.setenv("HEAT2D_MAX_WAVES", "96")
    c = case(1100, 0.2, dtype, 3 * tb + 5).powered()
    got, pl = solve(c, dtype, tb, autotune=0, graph=True)
    assert pl["dynamic"] == 1 and pl["main_items"] > pl["main_waves"], pl
    assert np.array_equal(got, c.gold)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tb,order", [("fp64", 12, "concurrent"), ("fp32", 16, "edge-first")])
def test_hip_exact_three_ranks(gpu, native, monkeypatch, dtype, tb, order):
    """Real halo exchanges: 3 loopback ranks, autotuned split plans."""
    monkeypatch.setenv("HEAT2D_SPLIT_ORDER", order)
    c = case(1100, 0.2, dtype, 2 * tb + 3).powered()
    g = LoopbackGroup(c.p, 3, dtype=dtype, backend="hip", tb=tb, device=0, arith="exact", autotune=1)
    g.upload(c.T0)
    g.step(c.p.ntime)
    got = g.download()
    g.close()
    assert np.array_equal(got, c.gold)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tb", [("fp64", 14), ("fp32", 16)])
def test_hip_exact_step_stats(gpu, native, dtype, tb):
    """Fused statistics kernels (form 0) and the one-step residual on rough data."""
    steps = 3 * tb + 2
    n1 = steps - tb
    c = case(1100, 0.2, dtype, steps, snaps=(n1 - 1, n1)).powered()
    s = HeatSolver(c.p, dtype=dtype, backend="hip", tb=tb, device=0, arith="exact")
    s.upload(c.T0)
    st = s.step_stats(n1)
    T = c.at[n1].astype(np.float64)
    d = T - c.at[n1 - 1].astype(np.float64)
    assert st["min"] == T.min() and st["max"] == T.max()
    assert np.isclose(st["sum"], T.sum(), rtol=1e-12, atol=1e-9)
    assert np.isclose(st["sum_sq"], (T * T).sum(), rtol=1e-12)
    assert np.isclose(st["residual_l2"], np.sqrt((d * d).sum()), rtol=1e-10)
    assert st["residual_max"] == np.abs(d).max()
    s.step(tb)
    got = s.download()
    s.close()
    assert np.array_equal(got, c.gold)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
@pytest.mark.parametrize("sigma", [0.2, 0.2371])
def test_hip_exact_jit_engine(gpu, native, dtype, sigma):
    """The run-time-compiled kernel: its contraction option and baked r."""
    c = case(257, sigma, dtype, 9).powered()
    got = run(c.p, "hip", dtype, 1, upload=c.T0, engine="jit")
    assert np.array_equal(got, c.gold), np.abs(got.astype(np.float64) - c.gold).max()


def slab_field(c, L, device):
    """A field of layout L (rows [L.row0, L.row0 + L.nrows) of c's grid) holding
    the frame-inclusive rough field: owned rows, every ghost row the
    allocation has, and the frame columns."""
    import torch
    from heat2d.ops import kernels as K
    m = c.p.n_owned
    full = R.initial_field(c.p, c.npdt)
    full[1:-1, 1:-1] = c.T0
    f = K.empty_field(L, torch.float64 if c.npdt == np.float64 else torch.float32, "cpu")
    K.init_field(f, L, c.p.ic, c.p.x)
    v = K.view2d(f, L)
    lo = max(-L.halo, -1 - L.row0)            # first local row inside the frame-inclusive grid
    hi = min(L.nrows + L.halo, m + 1 - L.row0)  # one past the last
    v[L.halo + lo:L.halo + hi, L.cpad - 1:L.cpad + m + 1] = torch.from_numpy(
        np.ascontiguousarray(full[L.row0 + lo + 1:L.row0 + hi + 1]))
    return f.to(device)


@pytest.mark.gpu
def test_hip_exact_jit_op_on_tensors(gpu, native):
    import torch
    from heat2d.ops import jit
    from heat2d.ops import kernels as K
    c = case(257, 0.2, "fp32", 1).powered()
    m = c.p.n_owned
    L = K.make_layout(m, m, halo=16)
    a = slab_field(c, L, "cuda")
    b = a.clone()
    st = jit.JitStencil(torch.float32, L, c.p.r, arith="exact")
    st.step(a, b)
    torch.cuda.synchronize()
    st.close()
    assert np.array_equal(K.owned(b, L).cpu().numpy(), c.gold)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_exact_raw_op(gpu, native, dtype):
    """ops.kernels.tb_step in form 0 on a middle slab: rows (17, 61) of the slab
    [40, 140) of a 203-wide problem, depth 8; rows outside stay untouched."""
    import torch
    from heat2d.ops import kernels as K
    k, row0, nrows, (rb, re_) = 8, 40, 100, (17, 61)
    c = case(203, 0.2, dtype, k).powered()
    m = c.p.n_owned
    L = K.make_layout(nrows, m, halo=16, row0=row0, nrows_global=m)
    src = slab_field(c, L, "cuda")
    dst = torch.full_like(src, float("nan"))
    K.tb_step(src, dst, L, k, c.p.r, rows=(rb, re_), arith="exact")
    torch.cuda.synchronize()
    got = K.owned(dst, L).cpu().numpy()
    assert np.array_equal(got[rb:re_], c.gold[row0 + rb:row0 + re_])
    assert np.isnan(got[:rb]).all() and np.isnan(got[re_:]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,tb", [("fp64", 12), ("fp32", 16)])
def test_hip_pow2_other_than_quarter(gpu, native, dtype, tb):
    """sigma = 0.125: r is a power of two other than 1/4, auto picks fma, and
    fma, exact and the golden agree bitwise on rough data (no power condition:
    the forms are the same bits by construction)."""
    c = case(301, 0.125, dtype, 2 * tb + 3)
    assert c.p.r == 0.125 and N.arith_code("auto", c.p.r) == 1
    a = run(c.p, "hip", dtype, tb, arith="fma", upload=c.T0)
    b = run(c.p, "hip", dtype, tb, arith="exact", upload=c.T0)
    s = HeatSolver(c.p, dtype=dtype, backend="hip", tb=tb, device=0)
    assert s.info()["arith"] == 1
    s.close()
    assert np.array_equal(a, b)
    assert np.array_equal(a, c.gold)
