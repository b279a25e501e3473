"""Time-dependent heat source g(t) * f(x, y): a 1-D schedule G of per-step gains
beside source=S. The step at position q adds G[q] * S at every fused level,

    exact: T' = upd + (G[q] * S[i,j])      (the product rounded, then the add)
    fma:   T' = fma(G[q], S[i,j], upd)     (one rounding)

bitwise against the NumPy golden (models.reference.ftcs(source_gain=)) at every
pass depth, launch plan and rank count, on the CPU twin and on the HIP engine
(tb_kernel_gain, csrc/kernels/tb_impl.hpp), with the position kept in device
memory so that replayed graphs take the gains of their replay.

Data (fixed seeds): tests/source_worker.py's rough field and source; gains
10**uniform(-1, 0.5) with exact zeros at [2::5] and exact ones at [4::7], so
every cycle sees a 0, a 1 and rough values.

Two identities are the oracles of the golden itself: G == 1 gives the bits of
source= alone in both forms (1 * S is exact, fma(1, S, x) = x + S), and in
"exact" the run equals a loop of ftcs_step(source=(G[q] * S rounded)).
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
import instance_matrix as M  # noqa: E402
from source_worker import problem, rough_field, rough_source  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
SHAPES = [(77, 8), (301, 11)]
KNOBS = ("HEAT2D_PIPE", "HEAT2D_TB_RING", "HEAT2D_SPLIT_ORDER", "HEAT2D_BANDS", "HEAT2D_SEGMENTS", "HEAT2D_EDGE_BANDS",
         "HEAT2D_MAX_WAVES", "HEAT2D_DYNAMIC")


def gains(count, seed=7):
    g = 10.0 ** np.random.default_rng(seed).uniform(-1.0, 0.5, count)
    g[2::5] = 0.0
    g[4::7] = 1.0
    return g


_GOLD = {}


def traj(n, dtype, steps, arith="exact", rows=None, start=0):
    """The golden's owned points after every step 0..steps of the run from
    position `start` of gains(start + steps) (computed once, read-only)."""
    key = (n, dtype, steps, arith, rows, start)
    if key not in _GOLD:
        T, S = rough_field(n, dtype, rows=rows), rough_source(n, dtype, rows=rows)
        G = gains(start + steps).astype(NP[dtype])
        out = [R.owned(T).copy()]
        for q in range(steps):
            T = R.ftcs_step(T, problem(n, 1).r, arith, source=S, gain=G[start + q])
            out.append(R.owned(T).copy())
        for a in out:
            a.setflags(write=False)
        _GOLD[key] = out
    return _GOLD[key]


def differ(a, b):
    """Share of points with other bits."""
    return float((a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,))).any(-1).mean())


def solver(n, dtype, steps, backend="cpu", tb=4, arith="exact", G="rough", rows=None, **kw):
    dev = dict(device=0) if backend == "hip" else {}
    s = HeatSolver(problem(n, steps), dtype=dtype, backend=backend, tb=tb, arith=arith, rows=rows,
                   source=rough_source(n, dtype, rows=rows), source_gain=gains(steps) if isinstance(G, str) else G,
                   **dev, **kw)
    s.upload(rough_field(n, dtype, rows=rows))
    return s


# ------------------------------------------------------------------ CPU: the golden

@pytest.mark.parametrize("n,steps", SHAPES)
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_golden_identities(dtype, n, steps):
    dt = NP[dtype]
    p, T0, S = problem(n, steps), rough_field(n, dtype), rough_source(n, dtype)
    for arith in ("exact", "fma"):
        ones = R.ftcs(p, steps, dtype=dt, T0=T0, arith=arith, source=S, source_gain=np.ones(steps))
        assert np.array_equal(ones, R.ftcs(p, steps, dtype=dt, T0=T0, arith=arith, source=S)), arith
    G = gains(steps).astype(dt)
    T = T0.copy()
    for q in range(steps):
        T = R.ftcs_step(T, p.r, "exact", source=(G[q] * S).astype(dt))
    assert np.array_equal(R.owned(T), traj(n, dtype, steps)[steps])
    assert np.array_equal(R.owned(R.ftcs(p, steps, dtype=dt, T0=T0, source=S, source_gain=gains(steps))),
                          traj(n, dtype, steps)[steps])
    # gain_start and probe_history take the same entries
    H = R.probe_history(p, steps - 3, [(1, 1), (n, n)], dtype=dt, T0=T0, source=S, source_gain=gains(steps), gain_start=0)
    assert np.array_equal(H[-1], traj(n, dtype, steps)[steps - 3][[0, -1], [0, -1]])
    part = R.ftcs(p, 3, dtype=dt, T0=T0, source=S, source_gain=gains(steps), gain_start=0)
    rest = R.ftcs(p, steps - 3, dtype=dt, T0=part, source=S, source_gain=gains(steps), gain_start=3)
    assert np.array_equal(R.owned(rest), traj(n, dtype, steps)[steps])


@pytest.mark.parametrize("n,steps", SHAPES)
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_negative_controls(dtype, n, steps):
    """Shares of owned points with other bits, measured on this data (fp64, fp32):
    fma with the gain against fma with a pre-multiplied rounded source: n = 77 / 8 steps 4.03 %,
    4.23 %; n = 301 / 11 steps 6.48 %, 6.68 %. exact against fma: 20.81 %, 17.07 %; 19.60 %, 18.02 %.
    The near-miss schedules (shifted by one step, the mean, held over each 4-step pass, reversed)
    give other bits at >= 99.99 % of the points at both shapes in both dtypes."""
    dt = NP[dtype]
    p, T0, S = problem(n, steps), rough_field(n, dtype), rough_source(n, dtype)
    G = gains(steps + 1).astype(dt)
    ex, fm = traj(n, dtype, steps)[steps], traj(n, dtype, steps, "fma")[steps]
    T = T0.copy()
    for q in range(steps):
        T = R.ftcs_step(T, p.r, "fma", source=(G[q] * S).astype(dt))
    share = differ(fm, R.owned(T))
    print(f"{dtype} n={n}: fma gain vs pre-multiplied {100 * share:.2f} %, exact vs fma {100 * differ(ex, fm):.2f} %")
    assert share > 0 and differ(ex, fm) > 0

    def run(Gx):
        return R.owned(R.ftcs(p, steps, dtype=dt, T0=T0, source=S, source_gain=Gx))

    g = G[:steps]
    for name, Gx in (("shifted", G[1:]), ("mean", np.full(steps, g.mean(), dtype=dt)),
                     ("held", g[(np.arange(steps) // 4) * 4]), ("reversed", g[::-1].copy())):
        share = differ(ex, run(Gx))
        print(f"{dtype} n={n}: {name} {100 * share:.3f} %")
        assert share >= 0.9999, (name, share)


def test_golden_refusals():
    p, T0, S = problem(20, 4), rough_field(20, "fp64"), rough_source(20, "fp64")
    for G, why in (([1.0, -1.0, 1, 1], ">= 0"), ([1.0, np.nan, 1, 1], "finite"), ([1.0, np.inf, 1, 1], "finite"),
                   (np.ones((2, 2)), "1-D"), ([], "1-D"), ([1.0, 1.0], "past its end")):
        with pytest.raises(ValueError, match=why):
            R.ftcs(p, 4, T0=T0, source=S, source_gain=G)
    with pytest.raises(ValueError, match="source"):
        R.ftcs(p, 4, T0=T0, source_gain=np.ones(4))
    with pytest.raises(ValueError, match="source"):
        R.ftcs_step(T0, p.r, gain=1.0)


# ------------------------------------------------------------------ CPU twin

@pytest.mark.parametrize("tb", [1, 2, 7, 8])
@pytest.mark.parametrize("n,steps", SHAPES)
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_twin_bitwise(native, dtype, arith, n, steps, tb):
    s = solver(n, dtype, steps, tb=tb, arith=arith)
    s.step(steps)
    got, info = s.download(), s.info()["source_gain"]
    s.close()
    assert info == {"set": True, "length": steps, "position": steps}
    assert np.array_equal(got, traj(n, dtype, steps, arith)[steps])


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_loopback_uneven_slabs(native, dtype, arith):
    """77 rows on 3 ranks (26 / 26 / 25): every rank takes the whole schedule."""
    g = LoopbackGroup(problem(77, 8), 3, dtype=dtype, backend="cpu", tb=3, arith=arith, source=rough_source(77, dtype),
                      source_gain=gains(8))
    assert [r for _, r in g.slabs()] == [26, 26, 25]
    g.upload(rough_field(77, dtype))
    g.step(3)
    g.step(5)
    got, infos = g.download(), [g.gain_info(i) for i in range(3)]
    g.close()
    assert all(i == {"set": True, "length": 8, "position": 8} for i in infos)
    assert np.array_equal(got, traj(77, dtype, 8, arith)[8])


# ------------------------------------------------------------------ position

@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_position(native, dtype):
    n, steps = 77, 8
    s = solver(n, dtype, steps, tb=4)
    s.prepare(3)
    s.prepare(8)
    assert s.info()["source_gain"]["position"] == 0  # prepare() consumes nothing
    s.step(3)
    assert s.info()["source_gain"]["position"] == 3
    assert np.array_equal(s.download(), traj(n, dtype, steps)[3])
    s.step(5)  # step(3); step(5) == step(8)
    assert np.array_equal(s.download(), traj(n, dtype, steps)[8])
    before = s.download_field()
    with pytest.raises(RuntimeError, match="exhausted"):  # past the end: nothing moves
        s.step(1)
    assert s.info()["source_gain"]["position"] == 8 and s.info()["steps"] == 8
    assert np.array_equal(s.download_field(), before)
    # set_source_gain(G, start=s) == the golden with gain_start=s
    s.upload(rough_field(n, dtype))
    s.set_source_gain(gains(3 + steps), start=3)
    assert s.info()["source_gain"] == {"set": True, "length": 11, "position": 3}
    s.step(steps)
    assert np.array_equal(s.download(), traj(n, dtype, steps, start=3)[steps])
    with pytest.raises(RuntimeError, match="exhausted"):
        s.step_stats(2)
    # None: the bits of source= alone
    s.upload(rough_field(n, dtype))
    s.set_source_gain(None)
    assert s.info()["source_gain"] == {"set": False, "length": 0, "position": 0}
    s.step(steps)
    got = s.download()
    s.close()
    assert np.array_equal(got, R.owned(R.ftcs(problem(n, steps), steps, dtype=NP[dtype], T0=rough_field(n, dtype),
                                              source=rough_source(n, dtype))))


def test_step_stats_consumes_and_matches(native):
    s = solver(77, "fp64", 8, tb=4)
    st = s.step_stats(8)
    got, pos = s.download(), s.info()["source_gain"]["position"]
    s.close()
    assert pos == 8 and np.array_equal(got, traj(77, "fp64", 8)[8])
    assert st["sum"] == pytest.approx(float(got.sum()), rel=1e-12)


def _init_between_steps(backend, dtype, n, **kw):
    """step / init() / step with an odd cycle count before init(): init() resets the buffer parity,
    the schedule keeps its position, and the entries used, info() and the exhaustion check agree."""
    s = solver(n, dtype, 12, backend=backend, tb=4, **kw)
    s.step(4)  # one cycle: the other buffer is current now
    assert s.cycle_hist().get(4) == 1
    s.init()
    assert s.info()["source_gain"]["position"] == 4 and s.info()["steps"] == 0
    s.upload(rough_field(n, dtype))
    s.step(4)
    assert s.info()["source_gain"]["position"] == 8
    assert np.array_equal(s.download(), traj(n, dtype, 4, start=4)[4])  # G[4..7], not G[0..3] again
    s.init()  # after an even count too
    s.upload(rough_field(n, dtype))
    s.step(4)
    assert np.array_equal(s.download(), traj(n, dtype, 4, start=8)[4])
    with pytest.raises(RuntimeError, match="exhausted"):
        s.step(1)
    assert s.info()["source_gain"]["position"] == 12
    s.close()


@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_init_between_steps(native, dtype):
    _init_between_steps("cpu", dtype, 77)


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_pinned_negative_zero_survives(native, dtype, arith):
    """A frame of -0.0 and rough values keeps its bits under gains that include 0 and non-unit
    values, although the source array has nonzero frame entries."""
    n, dt = 40, NP[dtype]
    T0, S = rough_field(n, dtype), rough_source(n, dtype)
    T0[0, :] = dt(-0.0)
    T0[-1, 5:9] = dt(-0.0)
    T0[3:7, 0] = dt(-0.0)
    G = gains(9)
    assert (S[0] != 0).all() and (S[:, 0] != 0).all() and (G == 0).any() and ((G != 0) & (G != 1)).any()
    s = HeatSolver(problem(n, 9), dtype=dtype, backend="cpu", tb=4, arith=arith, source=S, source_gain=G)
    s.upload(T0)
    s.step(9)
    F = s.download_field()
    s.close()
    frame = np.ones_like(T0, dtype=bool)
    frame[1:-1, 1:-1] = False
    assert np.array_equal(F[frame].view(np.uint8), T0[frame].view(np.uint8))
    assert np.signbit(F[0]).all() and np.signbit(F[-1, 5:9]).all() and np.signbit(F[3:7, 0]).all()
    assert np.array_equal(F, R.ftcs(problem(n, 9), 9, dtype=dt, T0=T0, arith=arith, source=S, source_gain=G))


def test_refusals(native):
    p, S = problem(40, 4, 0.25), rough_source(40, "fp64")
    for G, why in (([1.0, -1.0], ">= 0"), ([1.0, np.nan], "finite"), ([np.inf], "finite"), (np.ones((2, 2)), "1-D"),
                   ([], "1-D"), (3.0, "1-D")):
        with pytest.raises(ValueError, match=why):
            HeatSolver(p, backend="cpu", source=S, source_gain=G)
    with pytest.raises(RuntimeError, match="heat source"):  # G needs source=
        HeatSolver(p, backend="cpu", source_gain=np.ones(4))
    with pytest.raises(RuntimeError, match="heat source"):
        LoopbackGroup(p, 2, backend="cpu", source_gain=np.ones(4))
    # everything a source refuses stays refused
    for kw, why in ((dict(arith="jacobi"), "jacobi"), (dict(arith="fast"), "fast"), (dict(bc_x="periodic"), "Dirichlet"),
                    (dict(bc_y="insulated"), "Dirichlet"), (dict(copy_swap=True), "copy-swap")):
        with pytest.raises(RuntimeError, match=why):
            HeatSolver(p, backend="cpu", source=S, source_gain=np.ones(4), **kw)
    with pytest.raises(RuntimeError, match="jit|HIP"):
        HeatSolver(p, backend="cpu", engine="jit", source=S, source_gain=np.ones(4))
    for kw in (dict(rmap=np.full((42, 42), 0.1)), dict(faces=(np.full((42, 42), 0.1), np.full((42, 42), 0.1)))):
        with pytest.raises((RuntimeError, ValueError)):
            HeatSolver(p, backend="cpu", source=S, source_gain=np.ones(4), **kw)
    s = HeatSolver(p, backend="cpu", source=S)
    with pytest.raises(ValueError, match="start"):
        s.set_source_gain(np.ones(4), start=5)
    s.set_source_gain(np.ones(4))
    s.set_source(None)  # a schedule scales a source: cleared with it
    assert s.info()["source_gain"]["set"] is False and s.source_gain_sha256 is None
    with pytest.raises(RuntimeError, match="heat source"):
        s.set_source_gain(np.ones(4))
    s.close()


def test_auto_and_clamp(native):
    """arith "auto" resolves as with a source; the depth is clamped to the source kernels'."""
    inp = heat2d.parse_input_text("64 0.25 0.05 1.0 6 0")
    p = heat2d.make_problem(inp, "ghost", "uniform")
    S = rough_source(p.n_owned, "fp64")
    s = HeatSolver(p, backend="cpu", arith="auto", tb=24, source=S, source_gain=gains(6))
    info = s.info()
    s.step(6)
    got = s.download()
    s.close()
    assert info["arith"] == N.ARITH["fma"] and info["tb"] <= info["source"]["max_tb"] == 16
    assert info["source"] == {"enabled": True, "set": True, "max_tb": 16}  # info()["source"] as it was
    assert np.array_equal(got, R.owned(R.ftcs(p, 6, arith="fma", source=S, source_gain=gains(6))))


# ------------------------------------------------------------------ probes

@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_cpu_probes(native, dtype, arith):
    n, steps = 77, 8
    pts = [(1, 1), (1, n), (n, 1), (n, n), (26, 30), (27, 30), (40, 41)]
    p, T0, S = problem(n, steps), rough_field(n, dtype), rough_source(n, dtype)
    H = R.probe_history(p, steps, pts, dtype=NP[dtype], T0=T0, arith=arith, source=S, source_gain=gains(steps))
    s = solver(n, dtype, steps, tb=7, arith=arith, probes=pts, probe_steps=steps)
    s.step(3)
    s.step(5)
    got, last = s.probe_history(), s.download()
    s.close()
    assert np.array_equal(got, H)
    assert np.array_equal(got[-1], last[[i - 1 for i, _ in pts], [j - 1 for _, j in pts]])
    g = LoopbackGroup(p, 3, dtype=dtype, backend="cpu", tb=4, arith=arith, source=S, source_gain=gains(steps), probes=pts,
                      probe_steps=steps)
    g.upload(T0)
    g.step(steps)
    got = g.probe_history()
    g.close()
    assert np.array_equal(got, H)


def _raw_cone(device, dtype, arith, k=9, n=90):
    import torch

    from heat2d.ops import kernels as K
    dt = NP[dtype]
    T0, S = rough_field(n, dtype, seed=3), rough_source(n, dtype, seed=3)
    L = K.make_layout(n, n, halo=24, row0=0, nrows_global=n)
    host = np.full((L.rows_alloc(), L.pitch), 3.25, dtype=dt)
    host[L.halo - 1:L.halo + n + 1, L.cpad - 1:L.cpad + n + 1] = T0
    src = torch.from_numpy(host.reshape(-1).copy()).to(device)
    q = K.source_field(S, L, src.dtype, device)
    pts = [(1, 1), (n, n), (1, n), (45, 46), (5, 80)]
    G = gains(k).astype(dt)
    out = K.probe_cone(src, L, k, 0.2, pts, arith=arith, source=q, gain=torch.from_numpy(G).to(device))
    H = R.probe_history(problem(n, k), k, pts, dtype=dt, T0=T0, arith=arith, source=S, source_gain=G)
    return out.cpu().numpy(), H


@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_raw_cone_cpu(native, dtype, arith):
    got, H = _raw_cone("cpu", dtype, arith)
    assert np.array_equal(got, H)


def _raw_op(device, dtype, k, arith, n=150, ncols=261, row0=40, nrows=70, pos=2):
    """tb_step(gain=, gain_pos=) on a middle slab (rows 40..110 of 150) with NaN guard bands
    around the rows written; as tests/test_source.py _raw_op."""
    import torch

    from heat2d.ops import kernels as K
    dt = NP[dtype]
    rng = np.random.default_rng(7)
    T0 = (10.0 ** rng.uniform(-1, 1, (n + 2, ncols + 2))).astype(dt)
    S = (T0 * 10.0 ** rng.uniform(-3, -1, T0.shape) * rng.choice([-1.0, 1.0], T0.shape)).astype(dt)
    G = gains(pos + k).astype(dt)
    L = K.make_layout(nrows, ncols, halo=24, row0=row0, nrows_global=n)
    host = np.full((L.rows_alloc(), L.pitch), 3.25, dtype=dt)
    g0 = row0 - L.halo
    host[:, L.cpad - 1:L.cpad + ncols + 1] = T0[g0 + 1:g0 + 1 + L.rows_alloc()]
    src = torch.from_numpy(host.reshape(-1).copy()).to(device)
    dst = torch.full_like(src, float("nan"))
    q = K.source_field(S, L, src.dtype, device)
    K.tb_step(src, dst, L, k, 0.2, arith=arith, source=q, gain=torch.from_numpy(G).to(device), gain_pos=pos)
    out = K.view2d(dst.cpu(), L).numpy().copy()
    T = T0.copy()
    for s in range(k):
        T = R.ftcs_step(T, dt(0.2), arith, source=S, gain=G[pos + s])
    own = out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols].copy()
    assert np.array_equal(own, T[row0 + 1:row0 + 1 + nrows, 1:-1])
    out[L.halo:L.halo + nrows, L.cpad:L.cpad + ncols] = np.nan
    rr, cc = np.nonzero(~np.isnan(out))
    assert ((rr >= L.halo) & (rr < L.halo + nrows)).all(), "kernel wrote outside its output rows"
    assert (cc >= L.cpad + ncols).all() and (cc < L.cpad + ncols + 8).all(), "kernel wrote beyond one vector of right pad"
    assert np.array_equal(out[rr, cc].view(np.uint8), host[rr, cc].view(np.uint8)), "frame / pad write changed a value"


@pytest.mark.parametrize("arith", ["exact", "fma"])
def test_raw_op_cpu(native, arith):
    _raw_op("cpu", "fp64", 8, arith)
    import torch

    from heat2d.ops import kernels as K
    L = K.make_layout(8, 8, halo=24, row0=0, nrows_global=8)
    f = torch.zeros(L.rows_alloc() * L.pitch, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="source"):
        K.tb_step(f, f.clone(), L, 2, 0.2, gain=torch.ones(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="past its end"):
        K.tb_step(f, f.clone(), L, 2, 0.2, source=f.clone(), gain=torch.ones(2, dtype=torch.float64), gain_pos=1)
    with pytest.raises(ValueError, match=">= 0"):
        K.tb_step(f, f.clone(), L, 2, 0.2, source=f.clone(), gain=-torch.ones(2, dtype=torch.float64))


def test_memory_planner_counts_the_schedule(native):
    from heat2d.utils import memplan
    a = memplan.footprint(1024, 1, "fp64", source=True)
    b = memplan.footprint(1024, 1, "fp64", source=True, source_gain=1000)
    assert b["total_bytes"] - a["total_bytes"] == (1000 + 16) * 8 + 16 == memplan.gain_bytes(1000, "fp64")
    assert b["field_bytes"] == a["field_bytes"]
    free = 8 << 30
    assert memplan.plan_max_grid("fp32", 1, free_bytes=free, reserve=0, source=True, source_gain=10 ** 6)["n"] <= \
        memplan.plan_max_grid("fp32", 1, free_bytes=free, reserve=0, source=True)["n"]


# ------------------------------------------------------------------ checkpoints and drivers

def test_checkpoint_restart_other_rank_count(native, tmp_path):
    """A checkpoint with a schedule as 2 ranks write it, resumed on 1 rank at G[step]: bitwise the
    uninterrupted run; without the schedule or with another one: refused before the first step."""
    from heat2d.utils import checkpoint
    n, p = 77, problem(77, 20)
    S, G = rough_source(n, "fp64"), gains(20)
    T0 = R.initial_field(p)
    T0[1:-1, 1:-1] = R.owned(rough_field(n, "fp64"))
    s = HeatSolver(p, backend="cpu", tb=4, arith="exact", source=S, source_gain=G)
    s.upload(T0)
    s.step(9)
    mid = s.download()
    checkpoint.save(s, str(tmp_path / "ck1"), step=9)
    s.close()
    meta = json.loads(open(os.path.join(checkpoint.resolve(str(tmp_path / "ck1")), "meta.json")).read())
    assert meta["source_gain_sha256"] == hashlib.sha256(G.tobytes()).hexdigest()
    sd = checkpoint.step_dir(str(tmp_path / "ck"), 9)
    os.makedirs(sd)
    r1 = N.decompose(n, 2, 1)[0]
    np.save(os.path.join(sd, "rank00000.npy"), mid[:r1])
    np.save(os.path.join(sd, "rank00001.npy"), mid[r1:])
    meta["nranks"] = 2
    with open(os.path.join(sd, "meta.json"), "w") as f:
        json.dump(meta, f)
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", source=S, source_gain=G)
    assert checkpoint.load(r, sd)["step"] == 9
    r.set_source_gain(G, start=9)
    r.step(11)
    assert np.array_equal(r.download(), R.owned(R.ftcs(p, 20, T0=T0, source=S, source_gain=G)))
    r.close()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", source=S)
    with pytest.raises(ValueError, match="with a source gain"):
        checkpoint.load(r, sd)
    r.close()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", source=S, source_gain=gains(20, seed=8))
    with pytest.raises(ValueError, match="differs from the checkpoint"):
        checkpoint.load(r, sd)
    r.close()
    r = HeatSolver(p, backend="cpu", tb=7, arith="exact", source=S, source_gain=G)
    del meta["source_gain_sha256"]  # a checkpoint without a schedule: the key is absent
    with open(os.path.join(sd, "meta.json"), "w") as f:
        json.dump(meta, f)
    with pytest.raises(ValueError, match="without a source gain"):
        checkpoint.load(r, sd)
    r.close()
    s = HeatSolver(p, backend="cpu", tb=4, source=S)  # ... and save() writes the key only with one
    checkpoint.save(s, str(tmp_path / "ck0"), step=0)
    s.close()
    assert "source_gain_sha256" not in json.loads(
        open(os.path.join(checkpoint.resolve(str(tmp_path / "ck0")), "meta.json")).read())


def py(cwd, *args):
    env = dict(os.environ, PYTHONPATH=os.path.dirname(HERE), OMP_NUM_THREADS="1", HEAT2D_CPU_THREADS="2")
    return subprocess.run([sys.executable, "-m", "heat2d", *args], cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=300)


def _driver_files(tmp_path, n, steps):
    (tmp_path / "input.dat").write_text(f"{n} 0.25 0.05 1.0 {steps} 1\n")
    S, G = rough_source(n, "fp64"), gains(steps)
    np.save(tmp_path / "src.npy", S)
    np.save(tmp_path / "g.npy", G)
    (tmp_path / "g.txt").write_text("# gains, one per step\n" + "".join(f"{v!r}  # step {q}\n" for q, v in enumerate(G.tolist())))
    np.save(tmp_path / "short.npy", G[:steps - 1])
    np.save(tmp_path / "other.npy", gains(steps, seed=8))
    np.save(tmp_path / "neg.npy", -G)
    return S, G


def test_python_driver(native, tmp_path):
    n, steps = 50, 30
    S, G = _driver_files(tmp_path, n, steps)
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "hat-cuda")
    gold = R.owned(R.ftcs(prob, steps, arith="fma", source=S, source_gain=G))
    args = ["--backend", "cpu", "--ic", "hat-cuda", "--quiet", "--output", "npy", "--source", "src.npy", "--arith", "fma"]
    for f in ("g.npy", "g.txt"):  # both file formats
        out = py(tmp_path, *args, "--source-gain", f)
        assert out.returncode == 0, out.stdout + out.stderr
        assert np.array_equal(np.load(tmp_path / "soln00000.npy"), gold), f
    out = py(tmp_path, *args, "--source-gain", "g.txt", "--ntime", "12", "--checkpoint", "ck")
    assert out.returncode == 0, out.stdout + out.stderr
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    assert meta["source_gain_sha256"] == hashlib.sha256(G.tobytes()).hexdigest() and meta["step"] == 12
    bad = py(tmp_path, *args, "--restart", "ck")
    assert bad.returncode != 0 and "source gain" in bad.stdout + bad.stderr
    bad = py(tmp_path, *args, "--restart", "ck", "--source-gain", "other.npy")
    assert bad.returncode != 0 and "differs from the checkpoint" in bad.stdout + bad.stderr
    out = py(tmp_path, *args, "--restart", "ck", "--source-gain", "g.npy")  # continues at G[12]
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.load(tmp_path / "soln00000.npy"), gold)
    bad = py(tmp_path, *args, "--source-gain", "short.npy")
    assert bad.returncode != 0 and "29 entries" in bad.stdout + bad.stderr
    bad = py(tmp_path, *args, "--source-gain", "neg.npy")
    assert bad.returncode != 0 and ">= 0" in bad.stdout + bad.stderr
    bad = py(tmp_path, "--backend", "cpu", "--ic", "hat-cuda", "--quiet", "--output", "none", "--source-gain", "g.npy")
    assert bad.returncode != 0 and "--source" in bad.stdout + bad.stderr


def test_native_cli(native, tmp_path):
    n, steps = 64, 30
    S, G = _driver_files(tmp_path, n, steps)
    prob = heat2d.make_problem(heat2d.read_input(str(tmp_path / "input.dat")), "ghost", "uniform")
    gold = R.owned(R.ftcs(prob, steps, arith="fma", source=S, source_gain=G))
    cli = [N.CLI_PATH, "--cpu", "--quiet", "--ic", "uniform", "--source", "src.npy"]

    def run_cli(*args):
        return subprocess.run([*cli, *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)

    for f in ("g.npy", "g.txt"):
        out = run_cli("--source-gain", f, "--output", "npy")
        assert out.returncode == 0, out.stdout + out.stderr
        assert np.array_equal(np.load(tmp_path / "soln00000.npy"), gold), f
    out = run_cli("--source-gain", "g.txt", "--ntime", "12", "--checkpoint", "ck", "--output", "none")
    assert out.returncode == 0, out.stdout + out.stderr
    with open(tmp_path / "ck" / "latest") as f:
        meta = json.loads((tmp_path / "ck" / f.read().strip() / "meta.json").read_text())
    assert meta["source_gain_sha256"] == hashlib.sha256(G.tobytes()).hexdigest() and meta["step"] == 12
    bad = run_cli("--restart", "ck")
    assert bad.returncode != 0 and "source gain" in bad.stdout + bad.stderr
    bad = run_cli("--restart", "ck", "--source-gain", "other.npy")
    assert bad.returncode != 0 and "differs from the checkpoint" in bad.stdout + bad.stderr
    out = run_cli("--restart", "ck", "--source-gain", "g.npy", "--gpus", "3", "--output", "npy")  # another rank count
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.concatenate([np.load(tmp_path / f"soln{r:05d}.npy") for r in range(3)], axis=0)
    assert np.array_equal(got, gold)
    # the other driver resumes it, given the same schedule (in the other format)
    out = py(tmp_path, "--backend", "cpu", "--ic", "uniform", "--quiet", "--output", "npy", "--source", "src.npy",
             "--source-gain", "g.txt", "--restart", "ck")
    assert out.returncode == 0, out.stdout + out.stderr
    assert np.array_equal(np.load(tmp_path / "soln00000.npy"), gold)
    bad = run_cli("--source-gain", "short.npy")
    assert bad.returncode != 0 and "29 entries" in bad.stdout + bad.stderr
    bad = run_cli("--source-gain", "neg.npy")
    assert bad.returncode != 0 and ">= 0" in bad.stdout + bad.stderr
    # an f8 schedule in an fp32 run: converted, and the digest is the converted array's
    out = run_cli("--dtype", "fp32", "--source-gain", "g.npy", "--ntime", "5", "--checkpoint", "ck32", "--output", "none")
    assert out.returncode == 0, out.stdout + out.stderr
    with open(tmp_path / "ck32" / "latest") as f:
        meta = json.loads((tmp_path / "ck32" / f.read().strip() / "meta.json").read_text())
    assert meta["source_gain_sha256"] == hashlib.sha256(G.astype(np.float32).tobytes()).hexdigest()


# ------------------------------------------------------------------ GPU

def setenv(monkeypatch, env):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split", "single"])
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_every_instance(native, gpu, monkeypatch, dtype, arith, mode):
    """tb_kernel_gain, depths 1..kMaxTBSrc: 2 K + 3 steps as step(K), step(K), step(3) at
    instance_matrix's shapes, once with a split plan and once as a single launch of three bands;
    the plan and the cycle histogram say that depth K ran on all four edge kinds."""
    setenv(monkeypatch, M.MODES[mode])
    n = M.N_OF[dtype]
    gold = traj(n, dtype, 2 * 16 + 3, arith)
    fails = []
    for k in range(1, 17):
        steps = 2 * k + 3
        s = solver(n, dtype, steps, backend="hip", tb=k, arith=arith, autotune=0, overlap=True, graph=False)
        for m in (k, k, 3):
            s.step(m)
        got, plan, info, hist = s.download(), s.plan(k), s.info(), s.cycle_hist()
        s.close()
        assert info["tb"] == k and info["source_gain"] == {"set": True, "length": steps, "position": steps}, (k, info)
        assert plan["k"] == k and (plan["valid"] in (1, 3) if mode == "split" else plan["valid"] == 2), (k, plan)
        assert M.kinds_run(dtype, k, n, plan, "src") >= {("src", e) for e in range(4)}, (k, plan)
        assert hist.get(k, 0) >= 2 and max(hist) == k, (k, hist)
        if not np.array_equal(got, gold[steps]):
            fails.append((k, differ(got, gold[steps])))
    assert not fails, f"(depth, share of points with other bits) {fails}"


STALE = {"graph": (dict(graph=True), {}),
         "concurrent": (dict(graph=False), {"HEAT2D_SPLIT_ORDER": "concurrent"}),
         "edge-first": (dict(graph=False), {"HEAT2D_SPLIT_ORDER": "edge-first"})}


@pytest.mark.gpu
@pytest.mark.parametrize("how", list(STALE))
@pytest.mark.parametrize("dtype,arith", [("fp64", "exact"), ("fp32", "fma")])
def test_hip_stale_position(native, gpu, monkeypatch, dtype, arith, how):
    """301 rows x 2897 columns, tb = 8, several items per wave from the dynamic queue. graph:
    two replays of the pair graph, then a shallower cycle — a replay that reused a captured
    position fails here, the gains differ from cycle to cycle. Eager: the concurrent
    (two-stream) and the edge-first order of the split plan. (HEAT2D_SPLIT_ORDER=lead is taken
    only by a rank that exchanges: test_hip_loopback_lead_order.)"""
    kw, env = STALE[how]
    setenv(monkeypatch, dict(env, HEAT2D_DYNAMIC="1", HEAT2D_MAX_WAVES="40"))
    n, rows, calls = 2897, 301, [16, 16, 5]
    gold = traj(n, dtype, sum(calls), arith, rows=rows)
    s = solver(n, dtype, sum(calls), backend="hip", tb=8, arith=arith, rows=rows, autotune=0, **kw)
    done = 0
    for m in calls:
        s.prepare(m)
        s.step(m)
        done += m
        assert s.info()["source_gain"]["position"] == done
        assert np.array_equal(s.download(), gold[done]), (how, done)
    plan, hist = s.plan(8), s.cycle_hist()
    s.close()
    assert hist.get(8, 0) == 4 and hist.get(5, 0) == 1, hist
    assert plan["valid"] == (3 if how == "edge-first" else 1) or how == "graph", plan


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_loopback_three_ranks(native, gpu, dtype, arith):
    """n = 302 on 3 loopback ranks (101 / 101 / 100): step(D), then step(D + 5)."""
    n, D = 302, 16
    g = LoopbackGroup(problem(n, 2 * D + 5), 3, dtype=dtype, backend="hip", tb=D, device=0, arith=arith,
                      source=rough_source(n, dtype), source_gain=gains(2 * D + 5))
    g.upload(rough_field(n, dtype))
    g.step(D)
    mid = g.download()
    g.step(D + 5)
    got, infos = g.download(), [g.gain_info(i) for i in range(3)]
    g.close()
    gold = traj(n, dtype, 2 * D + 5, arith)
    assert all(i["position"] == 2 * D + 5 for i in infos)
    assert np.array_equal(mid, gold[D]) and np.array_equal(got, gold[2 * D + 5])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,arith", [("fp64", "exact"), ("fp32", "fma")])
def test_hip_loopback_lead_order(native, gpu, monkeypatch, dtype, arith):
    """The lead order (band launch first on the comm stream, the interior beside it), which only an
    exchanging rank takes: n = 302 on 3 loopback ranks, tb = 8, every plan forced to it and said
    so by plan(); gains that differ from cycle to cycle."""
    setenv(monkeypatch, {"HEAT2D_SPLIT_ORDER": "lead"})
    n, calls = 302, [16, 13]
    g = LoopbackGroup(problem(n, sum(calls)), 3, dtype=dtype, backend="hip", tb=8, device=0, arith=arith,
                      source=rough_source(n, dtype), source_gain=gains(sum(calls)))
    g.upload(rough_field(n, dtype))
    gold, done = traj(n, dtype, sum(calls), arith), 0
    for m in calls:
        g.step(m)
        done += m
        assert np.array_equal(g.download(), gold[done]), done
    plans, hists, infos = [g.plan(i, 8) for i in range(3)], [g.cycle_hist(i) for i in range(3)], [g.gain_info(i) for i in range(3)]
    g.close()
    assert all(p["order"] == "lead" and p["valid"] == 1 for p in plans), plans
    assert all(h.get(8, 0) == 2 and sum(k * c for k, c in h.items()) == sum(calls) for h in hists), hists
    assert all(i["position"] == sum(calls) for i in infos)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_init_between_steps(native, gpu, dtype):
    _init_between_steps("hip", dtype, 301, autotune=0, graph=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,arith", [("fp64", "fma"), ("fp32", "exact")])
def test_hip_trials_near_the_end(native, gpu, dtype, arith):
    """autotune on: prepare() runs the autotuner's trial cycles and the schedule trials with the
    schedule set, positioned so that a trial's K gains reach into the padding past the end of G
    (and, at the very end, lie in it entirely). They consume nothing and leave the field alone."""
    n, steps, start = 301, 6, 5
    s = solver(n, dtype, steps, backend="hip", tb=4, arith=arith, autotune=1, G=gains(start + steps))
    s.set_source_gain(gains(start + steps), start=start)
    s.prepare(steps)
    tuned = s.tune_stats
    assert tuned["depths"] > 0 and tuned["candidates"] > 0, tuned  # trial cycles ran
    assert s.info()["source_gain"] == {"set": True, "length": start + steps, "position": start}
    assert np.array_equal(s.download(), R.owned(rough_field(n, dtype)))
    s.step(steps)
    assert np.array_equal(s.download(), traj(n, dtype, steps, arith, start=start)[steps])
    s.prepare(4)  # at the end: every gain a trial reads is padding
    s.prepare(3)
    assert s.info()["source_gain"]["position"] == start + steps
    assert np.array_equal(s.download(), traj(n, dtype, steps, arith, start=start)[steps])
    with pytest.raises(RuntimeError, match="exhausted"):
        s.step(1)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_changing_the_schedule(native, gpu, dtype):
    """set_source_gain between steps with graph=True (captured graphs are dropped), then None."""
    n, dt = 301, NP[dtype]
    T0, S = rough_field(n, dtype), rough_source(n, dtype)
    p = problem(n, 40)
    s = solver(n, dtype, 16, backend="hip", tb=4, arith="fma", graph=True, autotune=0)
    s.step(16)  # pair graphs of depth 4
    assert np.array_equal(s.download(), traj(n, dtype, 16, "fma")[16])
    G2 = gains(30, seed=9)
    s.set_source_gain(G2, start=5)
    s.step(16)
    frame = T0.copy()
    frame[1:-1, 1:-1] = traj(n, dtype, 16, "fma")[16]
    want = R.ftcs(p, 16, dtype=dt, T0=frame, arith="fma", source=S, source_gain=G2, gain_start=5)
    assert s.info()["source_gain"] == {"set": True, "length": 30, "position": 21}
    assert np.array_equal(s.download(), R.owned(want))
    s.set_source_gain(None)
    s.step(16)
    got = s.download()
    s.close()
    assert np.array_equal(got, R.owned(R.ftcs(p, 16, dtype=dt, T0=want, arith="fma", source=S)))


@pytest.mark.gpu
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_hip_raw_ops(native, gpu, dtype, arith):
    _raw_op("cuda", dtype, 8, arith)
    _raw_op("cuda", dtype, 16, arith, pos=0)
    got, H = _raw_cone("cuda", dtype, arith)
    assert np.array_equal(got, H) and np.array_equal(got, _raw_cone("cpu", dtype, arith)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,arith", [("fp64", "exact"), ("fp64", "fma"), ("fp32", "exact"), ("fp32", "fma")])
def test_hip_probes(native, gpu, dtype, arith):
    """n = 301: the four corner owned points and a slab seam of 3 ranks (rows 101 | 102); one rank
    with graph=True, then 3 loopback ranks. The last row equals download() at the probes."""
    n, steps = 301, 37
    pts = [(1, 1), (1, n), (n, 1), (n, n), (101, 150), (102, 150), (201, 7), (202, 7), (150, 151)]
    p, T0, S = problem(n, steps), rough_field(n, dtype), rough_source(n, dtype)
    H = R.probe_history(p, steps, pts, dtype=NP[dtype], T0=T0, arith=arith, source=S, source_gain=gains(steps))
    s = solver(n, dtype, steps, backend="hip", tb=8, arith=arith, graph=True, autotune=0, probes=pts, probe_steps=steps)
    for m in (16, 16, 5):
        s.step(m)
    got, last = s.probe_history(), s.download()
    s.close()
    assert np.array_equal(got, H)
    assert np.array_equal(got[-1], last[[i - 1 for i, _ in pts], [j - 1 for _, j in pts]])
    g = LoopbackGroup(p, 3, dtype=dtype, backend="hip", tb=8, device=0, arith=arith, source=S, source_gain=gains(steps),
                      probes=pts, probe_steps=steps)
    g.upload(T0)
    g.step(20)
    g.step(17)
    got, last = g.probe_history(), g.download()
    g.close()
    assert np.array_equal(got, H)
    assert np.array_equal(got[-1], last[[i - 1 for i, _ in pts], [j - 1 for _, j in pts]])


@pytest.mark.gpu
def test_hip_clamp_and_refusals(native, gpu):
    p, S = problem(64, 4, 0.25), rough_source(64, "fp64")
    s = HeatSolver(p, backend="hip", device=0, tb=24, source=S, source_gain=np.ones(4))
    info = s.info()
    with pytest.raises(RuntimeError, match="exhausted"):
        s.step(5)
    assert s.info()["source_gain"]["position"] == 0 and s.info()["steps"] == 0
    s.step(4)
    got = s.download()
    s.close()
    assert info["tb"] == 16 == info["source"]["max_tb"]
    assert np.array_equal(got, R.owned(R.ftcs(p, 4, arith="fma", source=S)))  # G == 1: the bits of source= alone
    for kw, why in ((dict(arith="jacobi"), "jacobi"), (dict(arith="fast"), "fast"), (dict(bc_x="periodic"), "Dirichlet"),
                    (dict(bc_y="insulated"), "Dirichlet"), (dict(copy_swap=True), "copy-swap"), (dict(engine="jit"), "jit")):
        with pytest.raises(RuntimeError, match=why):
            HeatSolver(p, backend="hip", device=0, source=S, source_gain=np.ones(4), **kw)
    with pytest.raises(RuntimeError, match="heat source"):
        HeatSolver(p, backend="hip", device=0, source_gain=np.ones(4))
    with pytest.raises(ValueError, match=">= 0"):
        HeatSolver(p, backend="hip", device=0, source=S, source_gain=[-1.0])
