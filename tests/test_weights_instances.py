"""Every compiled tb_kernel_w5 instance once against the golden: each depth
1..kMaxTBW5, both dtypes, exact and fma, each in a split plan (boundary bands
and interior, both on the five-weight kernel) and in a single three-band launch,
at the instance matrix's shapes (fp64 n = 301, fp32 n = 517: a strip clear of
the frame columns, one that is not, a partial last lane). From cycle_hist(): two
cycles of that depth ran. Bitwise, on rough signed data with rough weights
(tests/weights_worker.py ROUGH), Dirichlet on both axes: all four edge kinds.
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
from weights_worker import ROUGH, problem, signed_field  # noqa: E402

KNOBS = ("HEAT2D_PIPE", "HEAT2D_TB_RING", "HEAT2D_SPLIT_ORDER", "HEAT2D_BANDS", "HEAT2D_SEGMENTS", "HEAT2D_EDGE_BANDS",
         "HEAT2D_MAX_WAVES", "HEAT2D_DYNAMIC")
_TRAJ = {}


def trajectory(dtype, arith):
    """Owned points of the golden after 5, 7, ..., 2 D + 3 steps (computed once, read-only)."""
    key = (dtype, arith)
    if key not in _TRAJ:
        T = signed_field(M.N_OF[dtype], dtype)
        out = []
        for m in range(2 * N.max_tb_w5() + 4):
            keep = m >= 5 and m % 2 == 1
            o = np.ascontiguousarray(R.owned(T)) if keep else None
            if keep:
                o.setflags(write=False)
            out.append(o)
            T = R.ftcs_step(T, 0.0, arith, weights=ROUGH)
        _TRAJ[key] = out
    return _TRAJ[key]


@pytest.fixture(scope="module", autouse=True)
def drop_trajectories():
    yield
    _TRAJ.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["split", "single"])
@pytest.mark.parametrize("arith", ["exact", "fma"])
@pytest.mark.parametrize("dtype", M.DTYPES)
def test_w5_instances(gpu, native, monkeypatch, dtype, arith, mode):
    """Every depth of one (dtype, arith, mode) row: 2 K + 3 steps as step(K), step(K) and the
    3-step remainder (two cycles of depth K each)."""
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in M.MODES[mode].items():
        monkeypatch.setenv(name, v)
    n = M.N_OF[dtype]
    T0, traj = signed_field(n, dtype), trajectory(dtype, arith)
    fails = []
    for k in range(1, N.max_tb_w5() + 1):
        steps = 2 * k + 3
        s = HeatSolver(problem(n, steps), dtype=dtype, backend="hip", tb=k, device=0, arith=arith, autotune=0,
                       overlap=True, graph=False, weights=ROUGH)
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
        assert info["tb"] == k and info["arith"] == N.ARITH[arith], (tag, info)
        assert info["weights"]["set"] and info["weights"]["max_tb"] == N.max_tb_w5(), (tag, info)
        cycles.assert_ran(hist, k, 2)
        assert max(int(d) for d, v in hist.items() if v) == k, (tag, hist)
        bad = got != traj[steps]
        if bad.any():
            fails.append((k, int(bad.sum()), tuple(int(x) for x in np.argwhere(bad)[0])))
    assert not fails, f"{dtype} {arith} {mode}: (depth, differing points, first index) {fails}"
