"""Every compiled tb_kernel_div instance once against the golden: each depth
1..kMaxTBDiv, both dtypes, exact and fma, each in a split plan (boundary bands
and interior) and in a single three-band launch, at the instance matrix's
shapes (fp64 n = 301, fp32 n = 517: a strip clear of the frame columns, one
that is not, a partial last lane). From the plan the solver reports: edge kinds
0..3 ran; from cycle_hist(): cycles of that depth ran. Bitwise, on rough data
with two materials at 100 : 1, zero faces and a zero-faced block
(tests/faces_worker.py).

The geometry is tests/instance_matrix.py's (imported, not copied): with faces
every launch runs the one kernel, which picks the kind per piece — the "src"
family's rule, with the row test applied to interior pieces too.
"""
import os
import sys

import numpy as np
import pytest

from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver
from heat2d.ops import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import cycles  # noqa: E402
import instance_matrix as M  # noqa: E402
from faces_worker import problem, rough_faces, rough_field  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
KNOBS = ("HEAT2D_PIPE", "HEAT2D_TB_RING", "HEAT2D_SPLIT_ORDER", "HEAT2D_BANDS", "HEAT2D_SEGMENTS", "HEAT2D_EDGE_BANDS",
         "HEAT2D_MAX_WAVES", "HEAT2D_DYNAMIC")
_TRAJ = {}


def depth_max():
    s = HeatSolver(problem(8, 1), backend="cpu", faces=(np.full((10, 10), 0.1), np.full((10, 10), 0.1)))
    d = s.info()["faces"]["max_tb"]
    s.close()
    return d


def trajectory(dtype, arith):
    """Owned points of the golden after 5, 7, ..., 2 D + 3 steps (computed once, read-only)."""
    key = (dtype, arith)
    if key not in _TRAJ:
        n = M.N_OF[dtype]
        T, F = rough_field(n, dtype), rough_faces(n, dtype)
        out = []
        for m in range(2 * depth_max() + 4):
            keep = m >= 5 and m % 2 == 1
            o = np.ascontiguousarray(R.owned(T)) if keep else None
            if keep:
                o.setflags(write=False)
            out.append(o)
            T = R.ftcs_step(T, 0.0, arith, faces=F)
        _TRAJ[key] = out
    return _TRAJ[key]


@pytest.fixture(scope="module", autouse=True)
def drop_trajectories():
    yield
    _TRAJ.clear()


def kinds_run(dtype, k, n, plan):
    """The edge kinds the launches of `plan` execute on tb_kernel_div: every rect of every launch,
    interior rects too, picks kind = (row test) | (column test) per piece (tb_impl.hpp tb_kernel_div)."""
    rects = list(plan["main_rects"] or [plan["main_rect"]])
    if plan["valid"] != 2:
        rects += list(plan["edge_rects"])
    return {M.strip_kind_cols(dtype, k, s, n) | M.item_kind_rows(t0, t1, k, n)
            for rect in rects for s, t0, t1 in M.rect_pieces(rect)}


def test_kinds_from_the_matrix_geometry():
    """The rule above agrees with instance_matrix.kinds_run's "src" family on a single-launch plan
    (where that function applies both tests to every piece)."""
    plan = {"valid": 2, "main_rects": [[0, 301, 0, 3, 3]], "main_rect": [0, 301, 0, 3, 3], "edge_rects": []}
    assert kinds_run("fp64", 8, 301, plan) == {e for _, e in M.kinds_run("fp64", 8, 301, plan, "src")} == {0, 1, 2, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split", "single"])
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_div_instances(gpu, native, monkeypatch, dtype, arith, mode):
    """Every depth of one (dtype, arith, mode) row: 2 K + 3 steps as step(K), step(K) and the
    3-step remainder (two cycles of depth K each)."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in M.MODES[mode].items():
        monkeypatch.setenv(name, v)
    n = M.N_OF[dtype]
    T0, F, traj = rough_field(n, dtype), rough_faces(n, dtype), trajectory(dtype, arith)
    fails = []
    for k in range(1, depth_max() + 1):
        steps = 2 * k + 3
        s = HeatSolver(problem(n, steps), dtype=dtype, backend="hip", tb=k, device=0, arith=arith, autotune=0, overlap=True,
                       graph=False, faces=F)
        s.upload(T0)
        sizes = cycles.calls(k, steps, 2)
        for m in sizes[:2] + cycles.balanced(k, sizes[2]):  # one cycle per call
            s.step(m)
        got, plan, info, hist = s.download(), s.plan(k), s.info(), s.cycle_hist()
        s.close()
        tag = (dtype, arith, mode, k)
        assert plan["k"] == k and plan["pipe"] == 0, (tag, plan)
        assert plan["main_strip_w"] == M.strip_width(dtype) and plan["main_useful_w"] == M.useful(dtype, k), (tag, plan)
        if mode == "split":
            assert plan["valid"] in (1, 3) and plan["edge_items"] > 0, (tag, plan)
        else:
            assert plan["valid"] == 2 and plan["order"] == "single", (tag, plan)
        assert kinds_run(dtype, k, n, plan) == {0, 1, 2, 3}, (tag, plan)
        assert info["tb"] == k and info["arith"] == N.ARITH[arith] and info["faces"]["set"], (tag, info)
        cycles.assert_ran(hist, k, 2)
        assert max(int(d) for d, v in hist.items() if v) == k, (tag, hist)
        bad = got != traj[steps]
        if bad.any():
            fails.append((k, int(bad.sum()), tuple(int(x) for x in np.argwhere(bad)[0])))
    assert not fails, f"{dtype} {arith} {mode}: (depth, differing points, first index) {fails}"
