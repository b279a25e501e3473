"""tests/cycles.py: the cycle depths one step(n) call runs, and the audit that
every depth-named pair-kernel case runs a cycle of the depth it names.

balanced() mirrors Solver::step_runs; it is held against the CPU twin's
HeatSolver.step_cycles (the same scheduler) where the native library is built,
and against three patterns frozen as literals where it is not. The audit runs
without a library and without a GPU: it reads tests/pipe_worker.py cases()."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cycles as Y  # noqa: E402
import pipe_worker  # noqa: E402

# one step(n) call with tb = K, as the depth-named tests made their steps
# before calls(): (tb, n) -> the balanced cycles, none of depth tb
SINGLE_CALL = {(20, 43): [15, 14, 14], (16, 35): [12, 12, 11], (24, 57): [19, 19, 19]}
# the pipe_worker cases that name a relaunch (several items per pair, the dynamic queue, segments): tb twice
RELAUNCH = ("items_static", "items_dynamic", "segments", "segments_dynamic", "depth_24_items", "depth_21_segments",
            "depth_19_items")


@pytest.mark.parametrize("tb", [1, 2, 7, 12, 16, 17, 20, 24])
def test_balanced_mirrors_the_twin(tb):
    from heat2d.ops import _native as N
    if not N.available():
        pytest.skip("native library missing")
    import heat2d
    from heat2d.models.heat2d import HeatSolver
    p = heat2d.make_problem(heat2d.InputDat(n=301, sigma=0.2, nu=0.05, dom_len=1.0, ntime=1), "ghost", "uniform")
    s = HeatSolver(p, dtype="fp64", backend="cpu", tb=tb, autotune=0)
    try:
        assert s.info()["tb"] == tb
        for n in range(1, 3 * tb + 6):
            assert Y.balanced(tb, n) == s.step_cycles(n), (tb, n)
    finally:
        s.close()


def test_single_call_never_reaches_tb():
    """Negative control, no library: the old pattern's depths, and the audit
    predicate is False for each of them."""
    for (tb, n), seq in SINGLE_CALL.items():
        assert Y.balanced(tb, n) == seq
        assert sum(seq) == n
        assert not Y.ran(seq, tb) and not Y.ran(Y.hist_of(seq), tb)
        with pytest.raises(AssertionError):
            Y.assert_ran(Y.hist_of(seq), tb)


def test_balanced_shapes():
    for tb in range(1, 25):
        assert Y.balanced(tb, 0) == [] and Y.balanced(tb, tb) == [tb]
        for n in range(1, 3 * tb + 6):
            seq = Y.balanced(tb, n)
            assert sum(seq) == n and len(seq) == -(-n // tb) and max(seq) - min(seq) <= 1 and max(seq) <= tb
            assert seq == sorted(seq, reverse=True)
    # the graph-pair branch: pairs of depth tb while left >= 2 tb, from parity 0 only
    assert Y.balanced(16, 48, graph=True) == [16, 16, 16]
    assert Y.balanced(16, 70, graph=True) == [16] * 4 + [6]
    assert Y.balanced(16, 48, graph=True, parity=1) == Y.balanced(16, 48) == [16, 16, 16]
    assert Y.balanced(16, 49, graph=True, parity=1) == [13, 16, 16, 4]  # (one balanced cycle, then parity 0)
    assert Y.balanced(20, 43, graph=True) == [20, 20, 3]


def test_calls():
    assert Y.calls(20, 43, 2) == [20, 20, 3] and Y.calls(12, 27) == [12, 15]
    assert Y.calls(20, 20) == [20] and Y.calls(20, 40, 2) == [20, 20] and Y.calls(24, 57, 2) == [24, 24, 9]
    for tb in (1, 7, 16, 24):
        for full in (1, 2):
            for steps in range(full * tb, 3 * tb + 6):
                c = Y.calls(tb, steps, full)
                assert sum(c) == steps and c[:full] == [tb] * full and len(c) <= full + 1 and min(c) > 0
                seq = Y.depths(tb, c)
                assert seq[:full] == [tb] * full and seq[full:] == Y.balanced(tb, steps - full * tb)
    with pytest.raises(ValueError):
        Y.calls(20, 39, 2)
    with pytest.raises(ValueError):
        Y.calls(20, 19)


def test_assert_ran():
    Y.assert_ran({20: 2, 3: 1}, 20, 2)
    Y.assert_ran({"20": 2, "3": 1}, 20, 2)  # (after a trip through JSON)
    Y.assert_ran([20, 20, 3], 20, 2)
    for hist, count in (({20: 1, 3: 1}, 2), ({19: 3}, 1), ({}, 1)):
        with pytest.raises(AssertionError):
            Y.assert_ran(hist, 20, count)


def case_depths(a):
    return Y.depths(a["tb"], a["calls"], graph=a.get("kind") == "graph")


def test_pipe_cases_run_their_depth():
    """The audit: every entry of pipe_worker.cases() makes its steps with
    `calls`, those add up to its step count, tb is among the cycle depths they
    run, and a case that names a relaunch runs tb twice."""
    cases = pipe_worker.cases()
    assert set(RELAUNCH) <= set(cases)
    bad = []
    for name, a in sorted(cases.items()):
        sizes = a.get("calls", [a["steps"]])  # (no calls: the one step(steps) the worker then makes)
        seq = Y.depths(a["tb"], sizes, graph=a.get("kind") == "graph")
        if sum(sizes) != a["steps"] or not Y.ran(seq, a["tb"], 2 if name in RELAUNCH else 1):
            bad.append((name, a["tb"], seq))
    assert not bad, f"cases that do not run the depth they name (name, tb, cycles): {bad}"
    assert all("calls" in a for a in cases.values())
    # each case's extra depths (`also`) run too
    for name, a in cases.items():
        for k in a.get("also", []):
            assert Y.ran(case_depths(a), k), (name, k)
