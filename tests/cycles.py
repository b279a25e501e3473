"""The cycle depths a step(n) call runs, and the step() calls that reach depth tb.

Plain Python (no torch, no native library): the tests and their workers share
it. One step(n) call on a solver with no measured schedule runs BALANCED
cycles — ceil(n / tb) of them, of depth about n / ceil(n / tb) — so
step(2 tb + 3) runs three cycles of depth about 2 tb / 3 and never one of depth
tb. A test that names a depth makes its steps with calls() and asserts the
depth from cycle_hist() with assert_ran()."""


def balanced(tb, n, graph=False, parity=0):
    """The cycle depths of one step(n) call: Solver::step_runs (csrc/runtime/
    solver.cpp) line by line, without a measured schedule. graph=True is the
    graph-pair branch: pairs of depth tb while left >= 2 tb, from buffer
    parity 0 only (the parity the pair graph was captured for)."""
    seq = []
    if n <= 0:
        return seq
    K = tb
    left = n
    par = parity
    while left > 0:
        if graph and left >= 2 * K and par == 0:
            pairs = left // (2 * K)
            seq += [K] * (2 * pairs)
            left -= pairs * 2 * K
            continue
        ncyc = (left + K - 1) // K
        k = left // ncyc + (1 if left % ncyc else 0)
        seq.append(k)
        left -= k
        par ^= 1
    return seq


def calls(tb, steps, full=1):
    """The step() sizes that make `steps` steps with `full` cycles of depth tb:
    the first `full` calls are of tb steps each (one cycle each), the last takes
    the remainder and still runs balanced cycles. calls(20, 43, 2) == [20, 20, 3],
    calls(12, 27) == [12, 15]."""
    if full < 1 or steps < full * tb:
        raise ValueError(f"{steps} steps do not hold {full} cycles of depth {tb}")
    rest = steps - full * tb
    return [tb] * full + ([rest] if rest > 0 else [])


def depths(tb, sizes, graph=False):
    """The cycle depths of a sequence of step() calls, in order (the buffer
    parity carried from call to call)."""
    seq = []
    for m in sizes:
        seq += balanced(tb, m, graph=graph, parity=len(seq) % 2)
    return seq


def hist_of(seq):
    """{depth: count} of a list of cycle depths: what cycle_hist() returns."""
    h = {}
    for k in seq:
        h[k] = h.get(k, 0) + 1
    return h


def ran(hist, tb, count=1):
    """The audit predicate: at least `count` cycles of depth tb in a cycle_hist()
    dict (keys may be strings after a trip through JSON) or a list of depths."""
    if not isinstance(hist, dict):
        hist = hist_of(hist)
    return sum(int(v) for k, v in hist.items() if int(k) == tb) >= count


def assert_ran(hist, tb, count=1):
    assert ran(hist, tb, count), f"no {count} cycle(s) of depth {tb} ran: cycle_hist {hist}"
