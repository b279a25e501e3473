"""The wave-pair interior kernel (tb_kernel_pipe: the deep fp64 r = 1/4 march
split over a producer and a consumer wave with 32-byte lanes, csrc/kernels/
tb_pipe_impl.hpp) on a real MI355X. Every case runs twice in fresh processes
(tests/pipe_worker.py; HEAT2D_PIPE is read once per process): forced on
(HEAT2D_PIPE=1) and off (=0). The two runs must agree bitwise with each other
AND with the NumPy golden of the same arithmetic — the pair kernel keeps the
one-wave march's operations and their order per point, so no tolerance — on
rough non-dyadic data. The shapes are the smallest at which the hand-over can
go wrong (tests/pipe_worker.py cases()). A FIFO wait that gives up raises in
the worker (the kernel's waits are bounded): a bug is a failed test, not a
hung GPU; each worker also runs under a time limit.

All four arithmetic forms have pair instances. jacobi, exact and fma are
bitwise against the golden of their form at any r (fma at sigma 0.2: against
its CPU twin, the golden model having no contracted form). fast is bitwise at r = 1/4
(there it is the jacobi form) and within its stated bound of the reference
rounding at sigma 0.2 (models.reference.fast_error_bound), where its bits
depend on which strips are interior ones, so the two runs are not compared.
The cases marked kind0 assert from the geometry that a strip clear of both
frame columns exists: only such strips carry scaled levels through the FIFO
and unscale once at the store.

The inst_<form>_<K> cases run every pair instance once (depths 16..24 x 4
forms; tests/test_instance_matrix.py holds the table against the built code
objects).

Every case makes its steps with tests/cycles.py calls() — step(K), step(K),
the remainder — and test_pipe_bitwise asserts from cycle_hist() that cycles
of depth K ran (every member's, for the loopback cases): one step(n) call runs
balanced cycles, ceil(n / K) of them, so step(2 K + 3) alone never reaches
depth K, and below depth 16 there is no pair kernel at all. Plan assertions
are made on the plan of every depth the history shows, not on plan(K) alone.
tests/test_cycles.py audits the table without a GPU.

The loopback cases run the pair kernel beside a halo exchange: two edge slabs,
three slabs (a middle one), and a depth-16 cycle followed by the exchange for
a depth-17 one (the plan re-made over wider boundary bands). The
test_pipe_boundary_conditions cases force it under periodic x, periodic y,
both, and insulated x."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cycles as Y  # noqa: E402
import pipe_worker as W  # noqa: E402
from test_cycles import RELAUNCH  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = W.cases()
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pipe_worker.py")


@pytest.fixture(scope="module")
def runs(gpu, native, tmp_path_factory):
    """{knob value: (outdir, info)} of the two worker runs."""
    out = {}
    for knob in ("1", "0"):
        d = str(tmp_path_factory.mktemp("pipe" + knob))
        env = dict(os.environ, HEAT2D_PIPE=knob, HEAT2D_PLAN_CACHE="off")
        r = subprocess.run([sys.executable, WORKER, d], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (knob, r.stdout[-2000:], r.stderr[-4000:])
        out[knob] = (d, json.load(open(os.path.join(d, "info.json"))))
    return out


_golden = {}


def golden(a):
    key = (a["n"], a["steps"], a["ic"], a.get("arith", "jacobi"), a.get("sigma", 0.25))
    if key not in _golden:
        p = W.problem(a["n"], a["steps"], a.get("sigma", 0.25))
        full = R.initial_field(p, np.float64)
        if a["ic"] == "rough":
            full[1:-1, 1:-1] = W.rough(a["n"])
        arith = a.get("arith", "jacobi")
        if arith == "fma" and a.get("sigma", 0.25) != 0.25:
            # the NumPy golden has no contracted form (it equals the reference
            # rounding only at a power-of-two r): the oracle is the CPU twin
            s = HeatSolver(p, dtype="fp64", backend="cpu", tb=4, arith="fma")
            s.upload(full[1:-1, 1:-1])
            s.step(p.ntime)
            _golden[key] = s.download()
            s.close()
        else:
            _golden[key] = R.owned(R.ftcs(p, dtype=np.float64, T0=full, arith="exact" if arith == "fast" else arith))
    return _golden[key]


def ran_plans(a, info, relaunch):
    """The plans of the cycles that ran, [(member, depth, plan)], after asserting
    from every member's cycle_hist() that the case made its cycles: exactly
    those of its calls, tb among them (twice where it names a relaunch)."""
    want = Y.hist_of(Y.depths(a["tb"], a["calls"], graph=a.get("kind") == "graph"))
    out = []
    for i, m in enumerate(info["members"]):
        hist = {int(k): v for k, v in m["hist"].items()}
        Y.assert_ran(hist, a["tb"], 2 if relaunch else 1)
        for k in a.get("also", []):
            Y.assert_ran(hist, k)
        assert hist == want, (i, hist, want)
        assert sorted(int(k) for k in m["plans"]) == sorted(hist)
        out += [(i, int(k), pl) for k, pl in m["plans"].items()]
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_pipe_bitwise(runs, name):
    a = CASES[name]
    on = np.load(os.path.join(runs["1"][0], name + ".npy"))
    off = np.load(os.path.join(runs["0"][0], name + ".npy"))
    pl_on, pl_off = runs["1"][1][name], runs["0"][1][name]
    print(name, "tb", a["tb"], "cycle_hist on", [m["hist"] for m in pl_on["members"]], "off",
          [m["hist"] for m in pl_off["members"]])
    assert len(pl_on["members"]) == len(pl_off["members"]) == a.get("ranks", 1)
    # the plans that ran (every member's, of every depth in its history): the pair kernel on
    # wide strips at every depth it exists at where forced, never with the knob off
    for i, k, pl in ran_plans(a, pl_off, name in RELAUNCH):
        assert pl["pipe"] == 0 and pl["main_strip_w"] == 128, (i, k, pl)
    for i, k, pl in ran_plans(a, pl_on, name in RELAUNCH):
        if k >= 16:
            assert pl["pipe"] == 1 and pl["valid"] in (1, 3), (i, k, pl)
            # (the library's strip shape against this file's own formula)
            assert pl["main_strip_w"] == 256 and pl["main_useful_w"] == W.useful(k), (i, k, pl)
            assert pl["main_rect"][3] == -(-a["n"] // W.useful(k)), (i, k, pl)  # wide strips cover the columns
        else:  # (no pair instance below depth 16: the one-wave kernel)
            assert pl["pipe"] == 0 and pl["main_strip_w"] == 128, (i, k, pl)
    assert pl_off["pipe"] == 0 and pl_off["main_strip_w"] == 128
    assert pl_on["pipe"] == 1 and pl_on["valid"] in (1, 3), pl_on
    assert pl_on["main_strip_w"] == 256 and pl_on["main_useful_w"] == W.useful(a["tb"])
    assert pl_on["main_rect"][3] == -(-a["n"] // W.useful(a["tb"]))
    assert sum(a["calls"]) == a["steps"]
    if name.startswith("inst_"):  # the every-instance cases: two cycles of depth tb and a 3-step one
        for pl in (pl_on, pl_off):
            assert pl["members"][0]["hist"] == {"3": 1, str(a["tb"]): 2}, pl["members"]
    if a.get("kind") == "loopback":
        # the slabs: every member's interior between its two boundary bands ran the pair kernel
        # (asserted above from its own plans); three ranks have a middle slab
        rows = [m["rows"] for m in pl_on["members"]]
        assert sum(rows) == a["n"] and min(rows) - 2 * a["tb"] >= 4 * a["tb"], rows
    if a.get("kind0"):
        assert W.kind0_strips(a["n"], a["tb"]), "no strip clear of the frame columns: the scaled path would not run"
    ref = golden(a)
    if a.get("arith") == "fast" and a.get("sigma", 0.25) != 0.25:
        full_max = max(float(W.rough(a["n"]).max()), float(R.initial_field(W.problem(a["n"], 1, a["sigma"])).max()))
        bound = R.fast_error_bound(a["steps"], np.float64, full_max)
        for got in (on, off):
            assert np.abs(got - ref).max() <= bound, (np.abs(got - ref).max(), bound)
        return
    assert np.array_equal(on, off), np.abs(on - off).max()
    if a.get("arith") == "fast":  # r = 1/4: the jacobi form's bits
        ref = golden(dict(a, arith="jacobi"))
    assert np.array_equal(on, ref), np.abs(on - ref).max()


def test_pipe_items_exceed_pairs(runs):
    """The several-items-per-pair cases really had more items than pairs, and
    the dynamic ones really ran the queue: read from the plan of the depth
    that ran (twice: cycle_hist)."""
    info = {}
    for name in RELAUNCH:
        m = runs["1"][1][name]["members"][0]
        Y.assert_ran(m["hist"], CASES[name]["tb"], 2)
        info[name] = m["plans"][str(CASES[name]["tb"])]
        assert info[name]["pipe"] == 1, (name, info[name])
    for name in ("items_static", "items_dynamic", "segments_dynamic", "depth_24_items", "depth_21_segments",
                 "depth_19_items"):
        assert info[name]["main_items"] > info[name]["main_waves"], info[name]
    assert info["items_dynamic"]["dynamic"] == 1 and info["segments_dynamic"]["dynamic"] == 1
    assert info["depth_24_items"]["dynamic"] == 1
    assert info["items_static"]["dynamic"] == 0 and info["depth_19_items"]["dynamic"] == 0
    assert info["segments"]["main_bands"] < 0 and info["depth_21_segments"]["main_bands"] < 0  # segments


# ---- the pair kernel under the other boundary conditions pipe_ok allows: periodic x (one rank: the
# self-wrap exchange), periodic y (the march over the view widened by 24 ghost columns a side; tight
# at depth 24) and both, at depths 24 and 16; insulated x with Dirichlet y at depth 20 (insulated y
# is refused: tests/test_insulated.py test_hip_forced_pipe). No kernel family of their own, so no row
# of the instance matrix. n = 2 U(K) + 37 (periodic x: rows per rank >= tb; periodic y: n >= 24),
# 2 K + 3 steps as step(K), step(K), step(3); rough data, arith "exact" at r = 0.2371, bitwise
# against models.reference.ftcs(bc_x=, bc_y=) and against the knob-off run.
BC_WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "periodic_worker.py")
BC_CASES = {f"{idx}_{k}": dict(n=2 * W.useful(k) + 37, steps=2 * k + 3, calls=Y.calls(k, 2 * k + 3, 2), tb=k, dtype="fp64",
                               bc_x=bx, bc_y=by)
            for idx, bx, by in (("px", "periodic", "dirichlet"), ("py", "dirichlet", "periodic"),
                                ("pxy", "periodic", "periodic")) for k in (24, 16)}
BC_CASES["ix_20"] = dict(n=2 * W.useful(20) + 37, steps=43, calls=Y.calls(20, 43, 2), tb=20, dtype="fp64", bc_x="insulated",
                         bc_y="dirichlet")


@pytest.fixture(scope="module")
def bc_runs(gpu, native, tmp_path_factory):
    """{knob value: (outdir, [info per BC_CASES entry])}: one worker per knob value."""
    out = {}
    for knob in ("1", "0"):
        d = str(tmp_path_factory.mktemp("pipebc" + knob))
        env = dict(os.environ, HEAT2D_PIPE=knob, HEAT2D_PLAN_CACHE="off")
        r = subprocess.run([sys.executable, BC_WORKER, "single", d, json.dumps(list(BC_CASES.values()))], env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (knob, r.stdout[-2000:], r.stderr[-4000:])
        out[knob] = (d, json.load(open(os.path.join(d, "info.json"))))
    return out


@pytest.mark.parametrize("name", list(BC_CASES))
def test_pipe_boundary_conditions(bc_runs, name):
    from periodic_worker import problem, rough_field
    a, i = BC_CASES[name], list(BC_CASES).index(name)
    on, off = (np.load(os.path.join(bc_runs[knob][0], f"result_{i}.npy")) for knob in ("1", "0"))
    inf_on, inf_off = bc_runs["1"][1][i], bc_runs["0"][1][i]
    print(name, "tb", a["tb"], "cycle_hist on", inf_on["cycle_hist"], "off", inf_off["cycle_hist"])
    for inf in (inf_on, inf_off):
        assert {int(k): v for k, v in inf["cycle_hist"].items()} == Y.hist_of(Y.depths(a["tb"], a["calls"]))
        Y.assert_ran(inf["cycle_hist"], a["tb"], 2)
    # the plan of the depth that ran: the pair kernel on wide strips where forced
    pl_on, pl_off = inf_on["plans"][str(a["tb"])], inf_off["plans"][str(a["tb"])]
    assert pl_off["pipe"] == 0 and pl_off["main_strip_w"] == 128, pl_off
    assert pl_on["pipe"] == 1 and pl_on["valid"] in (1, 3), pl_on
    assert pl_on["main_strip_w"] == 256 and pl_on["main_useful_w"] == W.useful(a["tb"]), pl_on
    ref = R.owned(R.ftcs(problem(a["n"], a["steps"]), a["steps"], dtype=np.float64, T0=rough_field(a["n"], "fp64"),
                         arith="exact", bc_x=a["bc_x"], bc_y=a["bc_y"]))
    assert np.array_equal(on, off), np.abs(on - off).max()
    assert np.array_equal(on, ref), np.abs(on - ref).max()


def test_kind0_cases_cover_the_scaled_path():
    """Every depth class has a case with a strip clear of both frame columns
    (K1 == K2: 16, 20, 24; K1 != K2: 19, 21), and the narrow cases have none."""
    k0 = {a["tb"] for a in CASES.values() if a.get("kind0") and W.kind0_strips(a["n"], a["tb"])}
    assert {16, 19, 20, 21, 24} <= k0
    assert not W.kind0_strips(CASES["cols_u_plus_1"]["n"], 20)
