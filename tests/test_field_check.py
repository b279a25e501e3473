"""Negative controls for the timed-field check (parallel/select.py).

``check_timed_field`` certifies a timed run's field against an independent
reference run; ``field_windows`` picks the rows it samples when a second copy of
the slab does not fit. Every other test only sees them report zero differences
on fields that agree. Here the field is damaged on purpose — one ulp, one NaN —
and the check must say so, in every window and in both the bitwise and the
bounded verdicts; where the sampling cannot see a difference, that is asserted
too, so the limit of ``windows`` is written down."""
import math
import types

import numpy as np
import pytest

import heat2d
from heat2d.models.heat2d import HeatSolver
from heat2d.parallel import select

NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------ fakes
class FakeRef:
    def __init__(self, log, **kw):
        self.log, self.kw, self.closed = log, kw, False

    def step(self, n):
        self.log.append(("step", n))

    def synchronize(self):
        pass

    def close(self):
        self.closed = True


class FakeTimed:
    """Duck-typed timed solver: .compare returns the scripted results in order."""

    def __init__(self, script, nrows=150, row0=0, n_owned=150):
        self.script = list(script)
        self.nrows, self.row0 = nrows, row0
        self.problem = types.SimpleNamespace(n_owned=n_owned)
        self.calls = []

    def compare(self, ref, r0=0, nrows=None, other_r0=None):
        self.calls.append((r0, nrows, other_r0))
        return self.script.pop(0)


def run_fake(script, arith, full=False):
    log, refs, amax_calls, asum_calls = [], [], [], []

    def make_ref(full_run, rows=None, slab_row0=None, arith="exact"):
        refs.append(FakeRef(log, full=full_run, rows=rows, slab_row0=slab_row0, arith=arith))
        return refs[-1]

    def amax(v):
        amax_calls.append(v)
        return v

    def asum(v):
        asum_calls.append(v)
        return v

    timed = FakeTimed(script)
    out = select.check_timed_field(timed, make_ref, 7, arith=arith, r=0.25, dtype="fp64", t0_absmax=2.0, full=full,
                                   amax=amax, asum=asum, window=16)
    return out, timed, refs, amax_calls, asum_calls


def res(d, m=None):
    return {"max_abs_diff": d, "mismatches": (0 if d == 0 else 1) if m is None else m}


@pytest.mark.parametrize("arith", ["exact", "fast"])  # a bitwise and a bounded verdict
@pytest.mark.parametrize("seq", [[NAN, 0.0, 0.0], [0.0, NAN, 0.0], [0.0, 0.0, NAN]])
def test_nan_in_any_window_fails(arith, seq):
    """A NaN reported for any one window — first, middle or last — is folded to
    inf and fails the check, whether the verdict is bitwise or a bound."""
    out, timed, refs, amax_calls, asum_calls = run_fake([res(d) for d in seq], arith)
    assert out["max_abs_diff"] == INF and out["ok"] is False
    assert out["mismatches"] == 1 and out["rows_checked"] == 48 and out["mode"] == "windows"
    # the reductions over ranks see the folded values, once each
    assert amax_calls == [INF]
    assert asum_calls == [1.0, 48.0]
    assert timed.script == [] and len(refs) == 3 and all(r.closed for r in refs)


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_fold_is_max_and_sum(arith):
    """Finite windows fold to their maximum and the sum of their mismatches;
    larger values before and after the maximum do not replace it."""
    out, timed, refs, amax_calls, asum_calls = run_fake([res(1e-3, 2), res(0.5, 5), res(1e-9, 1)], arith)
    assert out["max_abs_diff"] == 0.5 and out["mismatches"] == 8 and out["ok"] is False
    assert amax_calls == [0.5] and asum_calls == [8.0, 48.0]
    # the windows asked of compare are field_windows's, shifted into the reference slab
    wins = select.field_windows(150, 7, 0, 150, 16)
    assert timed.calls == [(a, m, a - g0) for a, m, g0, _ in wins]
    assert [(r.kw["rows"], r.kw["slab_row0"]) for r in refs] == [(nr, g0) for _, _, g0, nr in wins]
    assert all(r.kw["arith"] == "exact" and r.kw["full"] is False for r in refs)


def test_fake_verdicts():
    """Clean windows pass; a bounded verdict passes below its bound and fails
    above it; the bitwise verdict fails on a mismatch count alone (+0 / -0) and
    on a difference alone."""
    from heat2d.models import reference as R
    bound = R.fast_error_bound(7, np.float64, 2.0)
    assert run_fake([res(0.0)] * 3, "exact")[0]["ok"] is True
    out = run_fake([res(0.0)] * 3, "fast")[0]
    assert out["ok"] is True and out["bound"] == bound
    assert run_fake([res(0.0), res(bound), res(0.0)], "fast")[0]["ok"] is True
    assert run_fake([res(0.0), res(math.nextafter(bound, INF)), res(0.0)], "fast")[0]["ok"] is False
    assert run_fake([res(0.0), res(0.0, 1), res(0.0)], "exact")[0]["ok"] is False
    assert run_fake([res(0.0), res(1e-300, 0), res(0.0)], "exact")[0]["ok"] is False
    # full mode: one compare of the whole slab; NaN -> inf there too
    for arith in ("exact", "fast"):
        out, timed, refs, amax_calls, asum_calls = run_fake([res(NAN)], arith, full=True)
        assert out["max_abs_diff"] == INF and out["ok"] is False and out["rows_checked"] == 150
        assert timed.calls == [(0, None, None)] and amax_calls == [INF] and asum_calls == [1.0, 150.0]


# ------------------------------------------------------------------ field_windows
@pytest.mark.parametrize("window", [1, 16, 64])
@pytest.mark.parametrize("steps", [0, 7, 300])
def test_field_windows_properties(steps, window):
    for nrows in range(1, 201):
        for row0, extra in ((0, 0), (0, 55), (13, 0), (1000, 77)):
            n_global = row0 + nrows + extra
            wins = select.field_windows(nrows, steps, row0, n_global, window)
            assert 1 <= len(wins) <= 3
            m = min(window, nrows)
            covered = set()
            for a, mm, g0, ref_rows in wins:
                assert mm == m and 0 <= a and a + mm <= nrows  # inside the slab
                covered.update(range(a, a + mm))
                # the reference covers the window + steps + 1 rows each side, clipped to the grid
                lo = max(0, row0 + a - steps - 1)
                hi = min(n_global, row0 + a + mm + steps + 1)
                assert (g0, ref_rows) == (lo, hi - lo)
                other_r0 = row0 + a - g0
                assert 0 <= other_r0 and other_r0 + mm <= ref_rows
            assert 0 in covered and nrows - 1 in covered
            assert len({w[0] for w in wins}) == len(wins)  # no window twice


# ------------------------------------------------------------------ real solvers
def _problem(n, steps):
    return heat2d.make_problem(heat2d.InputDat(n=n, sigma=0.25, nu=0.05, dom_len=2.0, ntime=steps), "ghost", "hat")


class Rig:
    """A timed solver (IC + steps) and bench.py's reference factory for it."""

    def __init__(self, backend, n, steps, dtype="fp64"):
        self.backend, self.steps, self.dtype = backend, steps, dtype
        self.prob = _problem(n, steps)
        self.timed = HeatSolver(self.prob, dtype=dtype, backend=backend, arith="exact", autotune=0, graph=False)
        self.timed.step(steps)
        self.timed.synchronize()
        self.clean = self.timed.download()

    def make_ref(self, full_run, rows=None, slab_row0=None, arith="exact"):
        return HeatSolver(self.prob, dtype=self.dtype, backend=self.backend, rows=None if full_run else rows,
                          slab_row0=None if full_run else slab_row0, arith=arith,
                          engine="jit" if self.backend == "hip" else "tb", tb=1, overlap=False, graph=False,
                          autotune=0)

    def check(self, full, arith="exact", window=16):
        return select.check_timed_field(self.timed, self.make_ref, self.steps, arith=arith, r=self.prob.r,
                                        dtype=self.dtype, t0_absmax=self.prob.ic.absmax(), full=full,
                                        amax=lambda v: v, asum=lambda v: v, window=window,
                                        sterbenz=self.prob.ic.sterbenz_safe())

    def plant(self, i, j, value=None):
        """The clean field with element (i, j) moved one ulp up (or set to
        ``value``); returns |new - old| in float64."""
        f = self.clean.copy()
        f[i, j] = np.nextafter(f[i, j], f.dtype.type(np.inf)) if value is None else value
        self.timed.upload(f)
        return abs(float(f[i, j]) - float(self.clean[i, j]))

    def close(self):
        self.timed.close()


@pytest.fixture(scope="module")
def cpu_rig(native):
    rig = Rig("cpu", 150, 7)
    yield rig
    rig.close()


def test_clean_field_passes_cpu(cpu_rig):
    cpu_rig.timed.upload(cpu_rig.clean)
    assert np.ptp(cpu_rig.clean) > 0.5  # the hat has diffused: not a constant field
    out = cpu_rig.check(True)
    assert out["ok"] is True and out["mode"] == "full" and out["rows_checked"] == 150
    assert out["max_abs_diff"] == 0.0 and out["mismatches"] == 0
    out = cpu_rig.check(False)
    assert out["ok"] is True and out["mode"] == "windows" and out["rows_checked"] == 48
    assert out["max_abs_diff"] == 0.0 and out["mismatches"] == 0
    assert [w[0] for w in select.field_windows(150, 7, 0, 150, 16)] == [0, 67, 134]


@pytest.mark.parametrize("i,j", [(0, 0), (40, 75), (149, 149), (75, 0)])
def test_one_ulp_fails_full_cpu(cpu_rig, i, j):
    ulp = cpu_rig.plant(i, j)
    out = cpu_rig.check(True)
    assert ulp > 0 and out["ok"] is False and out["mismatches"] == 1 and out["max_abs_diff"] == ulp


# rows of the three windows of a 150-row slab at window=16: [0, 16), [67, 83), [134, 150)
@pytest.mark.parametrize("i,j", [(0, 3), (15, 149), (67, 0), (82, 75), (134, 149), (149, 0)])
def test_one_ulp_fails_windows_cpu(cpu_rig, i, j):
    ulp = cpu_rig.plant(i, j)
    out = cpu_rig.check(False)
    assert ulp > 0 and out["ok"] is False and out["mismatches"] == 1 and out["max_abs_diff"] == ulp
    assert out["rows_checked"] == 48


@pytest.mark.parametrize("i", [16, 40, 66, 83, 133])
def test_windows_do_not_see_other_rows_cpu(cpu_rig, i):
    """The sampling limit of ``windows``: a difference in a row outside all
    three windows is NOT seen — the mode checks 48 of 150 rows here, and only
    ``full`` certifies the whole slab."""
    ulp = cpu_rig.plant(i, 75)
    out = cpu_rig.check(False)
    assert ulp > 0 and out["ok"] is True and out["mismatches"] == 0 and out["max_abs_diff"] == 0.0
    assert cpu_rig.check(True)["ok"] is False


@pytest.mark.parametrize("arith", ["fast", "exact"])
@pytest.mark.parametrize("i", [3, 70, 149])  # a row of the first, the middle and the last window
def test_nan_fails_windows_cpu(cpu_rig, arith, i):
    """A NaN in any window fails the bounded verdict ("fast": ok is diff <=
    bound, the mismatch count is not consulted) as well as the bitwise one."""
    cpu_rig.plant(i, 20, value=np.nan)
    out = cpu_rig.check(False, arith=arith)
    assert out["max_abs_diff"] == INF and out["mismatches"] == 1 and out["ok"] is False
    out = cpu_rig.check(True, arith=arith)
    assert out["max_abs_diff"] == INF and out["mismatches"] == 1 and out["ok"] is False


def test_bounded_verdict_cpu(cpu_rig):
    """The bounded verdict ("fast") passes a clean field and a one-ulp
    difference (below the stated bound) and fails one above the bound."""
    cpu_rig.timed.upload(cpu_rig.clean)
    out = cpu_rig.check(False, arith="fast")
    assert out["ok"] is True and out["max_abs_diff"] == 0.0
    ulp = cpu_rig.plant(70, 70)
    out = cpu_rig.check(False, arith="fast")
    assert out["ok"] is True and out["max_abs_diff"] == ulp <= out["bound"] and out["mismatches"] == 1
    d = cpu_rig.plant(70, 70, value=cpu_rig.clean[70, 70] + 1e-6)
    out = cpu_rig.check(False, arith="fast")
    assert out["ok"] is False and out["max_abs_diff"] == d > out["bound"]


@pytest.mark.gpu
def test_flips_fail_gpu(native, gpu):
    """The device comparator behind run-time compiled (jit) references: a
    one-ulp flip fails ``full`` and, in a first-window and a last-window row,
    ``windows``; exactly one mismatch and exactly the ulp are reported, so
    every other element matched bitwise."""
    rig = Rig("hip", 301, 7)
    try:
        assert [w[0] for w in select.field_windows(301, 7, 0, 301, 16)] == [0, 142, 285]
        ulp = rig.plant(150, 300)
        out = rig.check(True)
        assert out["engine"] == "jit-exact" and out["rows_checked"] == 301
        assert ulp > 0 and out["ok"] is False and out["mismatches"] == 1 and out["max_abs_diff"] == ulp
        out = rig.check(False)  # row 150 is in the middle window [142, 158)
        assert out["ok"] is False and out["mismatches"] == 1 and out["max_abs_diff"] == ulp
        for i, j in ((0, 0), (300, 300)):
            ulp = rig.plant(i, j)
            out = rig.check(False)
            assert out["rows_checked"] == 48
            assert ulp > 0 and out["ok"] is False and out["mismatches"] == 1 and out["max_abs_diff"] == ulp
        rig.plant(40, 7)  # outside the windows: not seen (the sampling limit)
        assert rig.check(False)["ok"] is True
        rig.plant(3, 7, value=np.nan)
        out = rig.check(False, arith="fast")
        assert out["max_abs_diff"] == INF and out["mismatches"] == 1 and out["ok"] is False
    finally:
        rig.close()
