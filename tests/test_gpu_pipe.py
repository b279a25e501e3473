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
objects). They make their 2 K + 3 steps as step(K), step(K), step(3) and
assert from cycle_hist() that cycles of depth K ran: one step(n) call runs
balanced cycles, ceil(n / K) of them, so step(2 K + 3) alone never reaches
depth K."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pipe_worker as W  # noqa: E402

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


@pytest.mark.parametrize("name", sorted(CASES))
def test_pipe_bitwise(runs, name):
    a = CASES[name]
    on = np.load(os.path.join(runs["1"][0], name + ".npy"))
    off = np.load(os.path.join(runs["0"][0], name + ".npy"))
    pl_on, pl_off = runs["1"][1][name], runs["0"][1][name]
    # the plans that ran: the pair kernel on wide strips where forced, never with the knob off
    assert pl_off["pipe"] == 0 and pl_off["main_strip_w"] == 128
    assert pl_on["pipe"] == 1 and pl_on["valid"] in (1, 3), pl_on
    # (the library's strip shape against this file's own formula)
    assert pl_on["main_strip_w"] == 256 and pl_on["main_useful_w"] == W.useful(a["tb"])
    assert pl_on["main_rect"][3] == -(-a["n"] // W.useful(a["tb"]))  # wide strips cover the columns
    if "calls" in a:  # the every-instance cases: cycles of depth tb really ran (two, and a 3-step one)
        assert sum(a["calls"]) == a["steps"]
        assert pl_on["depths"] == [3, a["tb"]] and pl_off["depths"] == [3, a["tb"]], (pl_on, pl_off)
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
    the dynamic ones really ran the queue."""
    info = runs["1"][1]
    for name in ("items_static", "items_dynamic", "segments_dynamic", "depth_24_items", "depth_21_segments",
                 "depth_19_items"):
        assert info[name]["main_items"] > info[name]["main_waves"], info[name]
    assert info["items_dynamic"]["dynamic"] == 1 and info["segments_dynamic"]["dynamic"] == 1
    assert info["depth_24_items"]["dynamic"] == 1
    assert info["items_static"]["dynamic"] == 0 and info["depth_19_items"]["dynamic"] == 0
    assert info["segments"]["main_bands"] < 0 and info["depth_21_segments"]["main_bands"] < 0  # segments


def test_kind0_cases_cover_the_scaled_path():
    """Every depth class has a case with a strip clear of both frame columns
    (K1 == K2: 16, 20, 24; K1 != K2: 19, 21), and the narrow cases have none."""
    k0 = {a["tb"] for a in CASES.values() if a.get("kind0") and W.kind0_strips(a["n"], a["tb"])}
    assert {16, 19, 20, 21, 24} <= k0
    assert not W.kind0_strips(CASES["cols_u_plus_1"]["n"], 20)
