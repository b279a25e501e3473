"""Every compiled stencil instance, once, against the golden.

The library ships one template instance per (dtype, ring, interior / general,
arithmetic form, depth) — 768 plain tb_kernel instances, 192 with fused
statistics, 144 insulated, 64 heat-source and 64 diffusivity-map ones — each
with its own register allocation, ring, dependency chains and occupancy floor.
The other GPU tests run hand-picked depths; this file runs all of them from
one table (tests/instance_matrix.py cases()), and test_matrix_names_every_instance
holds that table against the instances in the built code objects.

Which instance is covered by which mode (one rank, Dirichlet, autotune off, no
graph, HEAT2D_PIPE unset, ring forced with HEAT2D_TB_RING):

  split   (overlap=True)                  tb_kernel<MAIN> rings 4 / 6, kinds 0 and 2
                                          (the interior), and tb_kernel<general>
                                          rings 4 / 6, kinds 1 and 3 (the two bands)
  single  (HEAT2D_SPLIT_ORDER=single,     tb_kernel<general> rings 4 / 6 and, fp32
           HEAT2D_BANDS=3)                K <= 16, ring 8: kinds 0..3 in one launch
  stats   (step_stats, tb = K)            tb_kernel<general, stats> ring 4, kinds 0..3
  ins / src / var, split and single       tb_kernel_ins (split: kinds 1, 2, 3 — the
                                          interior strips stay on tb_kernel<MAIN>;
                                          single: kinds 0..3), tb_kernel_src and
                                          tb_kernel_var (kinds 0..3 in both modes)

Every id asserts from the plan that ran (HeatSolver.plan(K)) the ring and, with
instance_matrix.kinds_run, the full set of (kernel, kind) paths above, and from
cycle_hist() that a cycle of depth K ran. One thing rests on reading the code
and not on a reported plan: the band count of the statistics launch (plan()
does not report it) — see test_stats_instances.

Shapes: fp64 n = 301, fp32 n = 517, the smallest at which a strip clear of both
frame columns exists at every depth (test_shapes_reach_every_kind). Data: rough
non-dyadic values 10**uniform(-1, 1) (tests/pipe_worker.rough), 2 K + 3 steps
per depth: two full passes and a shallower one, made as step(K), step(K),
step(3) — ONE step(2 K + 3) call runs balanced cycles of depth about 2 K / 3
and never one of depth K (test_step_counts_reach_depth). Every oracle is a NumPy golden
of models.reference, computed once per (family, dtype, variant) as one 51-step
trajectory; all comparisons are bitwise except the scaled form ("fast") at
r != 1/4, held to models.reference.fast_error_bound.
"""
import dataclasses
import os
import sys

import numpy as np
import pytest

import heat2d
from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver
from heat2d.ops import _native as N

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import cycles  # noqa: E402
import instance_matrix as M  # noqa: E402
import isa_report  # noqa: E402
import pipe_worker  # noqa: E402
from rmap_worker import rough_map  # noqa: E402
from source_worker import rough_field, rough_source  # noqa: E402

NP = {"fp64": np.float64, "fp32": np.float32}
NSTEPS = 2 * M.MAX_TB + 3  # 51: the longest run of the matrix
KNOBS = ("HEAT2D_PIPE", "HEAT2D_TB_RING", "HEAT2D_SPLIT_ORDER", "HEAT2D_BANDS", "HEAT2D_SEGMENTS", "HEAT2D_EDGE_BANDS",
         "HEAT2D_MAX_WAVES", "HEAT2D_DYNAMIC")
RUNS = []  # solver runs made by the GPU tests of this file (printed by each id)


def problem(n, steps, sigma):
    p = heat2d.make_problem(heat2d.InputDat(n=n, sigma=sigma, nu=0.05, dom_len=1.0, ntime=steps), "ghost", "uniform")
    if sigma == 0.25:  # r = nu dt / delta^2 is 1/4 only up to rounding (n = 517: one ulp off)
        assert abs(p.r - 0.25) <= 2.0 ** -52
        p = dataclasses.replace(p, r=0.25)
    return p


# ------------------------------------------------------------------ data and goldens

def start_field(family, dtype):
    """The frame-inclusive initial field of a family's runs, in the run's dtype.
    plain / stats: the reference IC's frame around tests/pipe_worker.rough;
    ins / src / var: tests/source_worker.rough_field (rough frame too)."""
    n = M.N_OF[dtype]
    if family in ("plain", "stats"):
        full = R.initial_field(problem(n, 1, 0.2), NP[dtype])
        full[1:-1, 1:-1] = pipe_worker.rough(n).astype(NP[dtype])
        return full
    return rough_field(n, dtype)


def extra_array(family, dtype):
    """The source (src) / map (var) of a family's runs: rough signed values /
    values in (0, 0.25] with some exact zeros (tests/source_worker, tests/rmap_worker)."""
    n = M.N_OF[dtype]
    return {"src": rough_source, "var": rough_map}[family](n, dtype)


_TRAJ = {}


def trajectory(family, dtype, arith, sigma):
    """Owned points of the golden after 0, 1, ..., 51 steps (computed once, read-only).
    arith: "exact", "jacobi", or "fma" — the TRUE contracted form (one rounding,
    models.reference.fma): without a source ftcs_step's "fma" keeps the exact
    expression, so the plain runs pass a source of -0.0 everywhere, which takes
    the contracted branch and adds nothing (x + -0.0 == x bitwise)."""
    key = (family, dtype, arith, sigma)
    if key not in _TRAJ:
        n = M.N_OF[dtype]
        r = problem(n, 1, sigma).r
        T = start_field(family, dtype)
        kw = {}
        if family == "ins":
            kw = dict(bc_x="insulated", bc_y="insulated")
            if arith == "fma":  # r = 1/4: the reference expression has the contracted form's bits
                assert r == 0.25
                arith = "exact"
        elif family == "src":
            kw = dict(source=extra_array(family, dtype))
        elif family == "var":
            kw = dict(rmap=extra_array(family, dtype))
        elif arith == "fma":
            kw = dict(source=np.full(T.shape, -0.0, dtype=T.dtype))
        out = []
        for m in range(NSTEPS + 1):
            # (the variant families compare at 2 K + 3 steps only: 5, 7, ..., 51)
            keep = family == "plain" or (m >= 5 and m % 2 == 1)
            o = np.ascontiguousarray(R.owned(T)) if keep else None
            if keep:
                o.setflags(write=False)
            out.append(o)
            T = R.ftcs_step(T, r, arith, **kw)
        _TRAJ[key] = out
    return _TRAJ[key]


@pytest.fixture(scope="module", autouse=True)
def drop_trajectories():
    yield
    _TRAJ.clear()  # not kept for the rest of the session


def oracle(case):
    """(trajectory, bitwise?) of a case: the table of the module docstring."""
    fam = "plain" if case["family"] == "stats" else case["family"]
    arith, sigma = case["arith"], case["sigma"]
    if arith == "fast":  # r = 1/4: the jacobi form's bits; else the reference rounding within the stated bound
        return trajectory(fam, case["dtype"], "jacobi" if sigma == 0.25 else "exact", sigma), sigma == 0.25
    return trajectory(fam, case["dtype"], arith, sigma), True


def fast_bound(case, steps):
    full = start_field("plain", case["dtype"])  # the frame value included
    return R.fast_error_bound(steps, NP[case["dtype"]], float(np.abs(full).max()))


def mismatch(got, ref):
    """None, or (max |got - ref|, first differing index) of a bitwise comparison."""
    if np.array_equal(got, ref):
        return None
    bad = np.argwhere(got.view(f"u{got.itemsize}") != ref.view(f"u{ref.itemsize}"))
    return float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max()), tuple(int(i) for i in bad[0])


# ------------------------------------------------------------------ CPU: the table, the shapes, the oracles

def built(pattern):
    return {p for p in (pattern(k["name"]) for k in isa_report.kernels(N.LIB_PATH)) if p}


def family_depth(family):
    """The deepest pass of the source / map kernels, as a solver reports it
    (tests/test_source_isa.py / test_rmap_isa.py hold it against the code objects)."""
    arr = np.zeros((10, 10))
    s = HeatSolver(problem(8, 1, 0.2), backend="cpu", tb=M.MAX_TB, **{"src": dict(source=arr), "var": dict(rmap=arr)}[family])
    d = s.info()[{"src": "source", "var": "rmap"}[family]]["max_tb"]
    s.close()
    return d


def all_cases():
    return M.cases(family_depth("src"), family_depth("var")) if N.available() else M.cases()


CASES = all_cases()


def of(family):
    return [c for c in CASES if c["family"] == family]


def ids(cs):
    return [c["id"] for c in cs]


@pytest.mark.skipif(not (N.available() and os.path.exists(isa_report.READELF)),
                    reason="native library or llvm-readelf missing")
def test_matrix_names_every_instance():
    """The instances the table claims to run are exactly the instances in the
    built library, family by family, with no exclusion list: an instance added
    to the build without a matrix row fails here, and so does a row that names
    an instance the library does not have."""
    import test_insulated_isa
    import test_rmap_isa
    import test_source_isa
    tb = built(isa_report.tb_params)
    have = {"plain": {p for p in tb if len(p) == 6}, "stats": {p for p in tb if len(p) == 7},
            "ins": built(test_insulated_isa.ins_params), "src": built(test_source_isa.src_params),
            "var": built(test_rmap_isa.var_params)}
    assert len(have["plain"]) + len(have["stats"]) == len(tb)
    for fam, inst in have.items():
        claimed = set().union(*(M.claimed_instances(c) for c in of(fam)))
        assert inst, fam
        assert claimed == inst, (fam, sorted(inst - claimed, key=str)[:8], sorted(claimed - inst, key=str)[:8])
    # every id is unique, and every plain / variant instance is run in each mode its kernel has
    assert len(set(ids(CASES))) == len(CASES)


@pytest.mark.skipif(not (N.available() and os.path.exists(isa_report.READELF)),
                    reason="native library or llvm-readelf missing")
def test_pipe_cases_name_every_pair_instance():
    """tests/pipe_worker.py cases() reaches every wave-pair instance (fp64,
    depths 16..24 x 4 forms), each with a strip clear of both frame columns."""
    have = built(isa_report.pipe_params)
    assert len(have) == 36
    claimed = {(a["tb"], M.ARITH.index(a.get("arith", "jacobi"))) for a in pipe_worker.cases().values()
               if a.get("kind0") and pipe_worker.kind0_strips(a["n"], a["tb"])}
    assert claimed == have, (sorted(have - claimed), sorted(claimed - have))


def test_shapes_reach_every_kind():
    """By the kernels' own formulas, at every depth of either dtype the matrix's
    n has a strip clear of both frame columns (kind 0) and one that is not (kind
    2), splits (n - 2K >= 4K), and leaves the middle of three bands clear of the
    frame rows. The hole this file was written for: fp32 at n = 301 has NO
    kind-0 strip at any depth, which is why the two dtypes' shapes differ."""
    for dtype in M.DTYPES:
        n = M.N_OF[dtype]
        assert n % 2 == 1
        for k in range(1, M.MAX_TB + 1):
            kinds = [M.strip_kind_cols(dtype, k, s, n) for s in range(M.nstrips(dtype, k, n))]
            assert 0 in kinds and 2 in kinds, (dtype, k, kinds)
            assert n % M.useful(dtype, k) != 0 and n % M.vec_elems(dtype) != 0  # partial last strip and lane
            assert n - 2 * k >= 4 * k
            assert M.item_kind_rows(n // 3, 2 * n // 3, k, n) == 0
            assert M.item_kind_rows(0, n // 3, k, n) == 1 and M.item_kind_rows(2 * n // 3, n, k, n) == 1
            assert n >= M.useful(dtype, k) + M.strip_width(dtype) - M.halo_cols(dtype, k)
            # one smaller than the bound of the module's N_OF comment has no kind-0 strip
            m = M.useful(dtype, k) + M.strip_width(dtype) - M.halo_cols(dtype, k) - 1
            assert all(M.strip_kind_cols(dtype, k, s, m) for s in range(M.nstrips(dtype, k, m)))
    assert max(M.useful("fp64", k) + 128 - M.halo_cols("fp64", k) for k in range(1, 25)) == 250
    assert max(M.useful("fp32", k) + 256 - M.halo_cols("fp32", k) for k in range(1, 25)) == 500
    for k in range(1, M.MAX_TB + 1):
        assert all(M.strip_kind_cols("fp32", k, s, 301) for s in range(M.nstrips("fp32", k, 301))), k
    # this file's geometry against tests/pipe_worker.py's own (the wide strip: fp64, 4 doubles per lane)
    assert [M.useful("fp32", k) for k in range(1, 25)] == [pipe_worker.useful(k) for k in range(1, 25)]


def test_kinds_run_on_hand_made_plans():
    """kinds_run on plans written out by hand (fp64 K = 4: U = 120, 3 strips of n = 301)."""
    split = dict(valid=1, main_rect=[4, 297, 0, 3, 2], main_rects=[], edge_rects=[[0, 4, 0, 3, 1], [297, 301, 0, 3, 1]])
    assert M.kinds_run("fp64", 4, 301, split) == {("main", 0), ("main", 2), ("gen", 1), ("gen", 3)}
    single = dict(valid=2, main_rect=[0, 301, 0, 3, 3], main_rects=[], edge_rects=[])
    assert M.kinds_run("fp64", 4, 301, single) == {("gen", e) for e in range(4)}
    assert M.kinds_run("fp64", 4, 301, dict(single, main_rect=[0, 301, 0, 3, 1])) == {("gen", 1), ("gen", 3)}
    # main_rects replace main_rect; a segment crossing a strip end is cut there
    assert M.kinds_run("fp64", 4, 301, dict(single, main_rects=[[0, 301, 1, 2, 1]])) == {("gen", 1)}
    assert list(M.rect_pieces([10, 20, 0, 2, -3])) == [(0, 10, 16), (0, 16, 20), (1, 10, 13), (1, 13, 20)]
    assert M.kinds_run("fp64", 4, 301, split, "ins") == {("main", 0), ("ins", 2), ("ins", 1), ("ins", 3)}
    assert M.kinds_run("fp64", 4, 301, split, "src") == {("src", e) for e in range(4)}
    with pytest.raises(ValueError):
        M.kinds_run("fp64", 4, 301, dict(split, valid=0))


def test_mismatch_reports_one_ulp():
    """The comparator of the depth loops: equal arrays pass, one ulp at one
    point is reported with its size and index."""
    for dtype in M.DTYPES:
        ref = trajectory("plain", dtype, "exact", 0.2)[5]
        got = ref.copy()
        assert mismatch(got, ref) is None
        got[7, 11] = np.nextafter(got[7, 11], np.inf)
        assert mismatch(got, ref) == (float(abs(np.float64(got[7, 11]) - np.float64(ref[7, 11]))), (7, 11))


@pytest.mark.parametrize("dtype", M.DTYPES)
def test_oracles_tell_the_forms_apart(dtype):
    """Negative control: on the matrix's own data and step counts (2 K + 3, K =
    1..24) the goldens differ at a nonzero share of the owned points, so a kernel
    that ran another form, or a step too few, cannot pass a bitwise comparison.
    Smallest share over the 24 step counts, measured:
        exact vs true fma, sigma 0.2:    fp64 0.109, fp32 0.100
        jacobi vs exact, sigma 0.25:     fp64 0.060, fp32 0.061
        exact / fma / jacobi vs itself one step short: 1.000 (fp32 exact and fma: 0.99996)
    Any share above zero is the condition."""
    ex, fm = trajectory("plain", dtype, "exact", 0.2), trajectory("plain", dtype, "fma", 0.2)
    ja, eq = trajectory("plain", dtype, "jacobi", 0.25), trajectory("plain", dtype, "exact", 0.25)

    def share(a, b):
        return float((a.view(f"u{a.itemsize}") != b.view(f"u{b.itemsize}")).mean())

    steps = [2 * k + 3 for k in range(1, M.MAX_TB + 1)]
    shares = {"exact-fma": min(share(ex[m], fm[m]) for m in steps),
              "jacobi-exact": min(share(ja[m], eq[m]) for m in steps)}
    for name, t in (("exact", ex), ("fma", fm), ("jacobi", ja)):
        shares[name + "-short"] = min(share(t[m], t[m - 1]) for m in steps)
    print(dtype, {k: round(v, 5) for k, v in shares.items()})
    assert all(v > 0 for v in shares.values()), shares


@pytest.mark.skipif(not N.available(), reason="native library missing")
@pytest.mark.parametrize("k", [1, 2, 7, 16, 17, 24])
def test_step_counts_reach_depth(k):
    """The cycle depths the matrix relies on, from the solver's own schedule
    (CPU twin, the same scheduler, Solver::step_runs): a step(n) call runs
    BALANCED cycles, ceil(n / K) of depth about n / ceil(n / K), so one call
    step(2 K + 3) with tb = K never runs a cycle of depth K once K > 3 (K = 24:
    17, 17, 17). The matrix therefore makes its 2 K + 3 steps as step(K),
    step(K), step(min(3, K)) ... — two full passes and a shallower one, each
    call one cycle — and its K + 1 statistics steps as step(1), step_stats(K)."""
    s = HeatSolver(problem(301, 2 * k + 3, 0.2), dtype="fp64", backend="cpu", tb=k, autotune=0)
    assert s.step_cycles(k) == [k]
    assert sum(chunks(k)) == 2 * k + 3 and chunks(k)[:2] == [k, k]
    assert all(len(s.step_cycles(m)) == 1 for m in chunks(k))
    if k > 3:
        assert k not in s.step_cycles(2 * k + 3) and k not in s.step_cycles(k + 1)
    s.close()


def chunks(k):
    """The step() calls that make 2 K + 3 steps with two cycles of depth K
    (tests/cycles.py calls()), the 3-step remainder as one-cycle calls too."""
    out = cycles.calls(k, 2 * k + 3, 2)
    return out[:2] + cycles.balanced(k, out[2])


# ------------------------------------------------------------------ GPU

def setenv(monkeypatch, case):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in case["env"].items():
        monkeypatch.setenv(name, v)


def solver_kw(case):
    fam = case["family"]
    if fam == "ins":
        return dict(bc_x="insulated", bc_y="insulated")
    if fam == "src":
        return dict(source=extra_array(fam, case["dtype"]))
    if fam == "var":
        return dict(rmap=extra_array(fam, case["dtype"]))
    return {}


def check_ran(case, k, plan, info, hist):
    """What the run of depth k says about itself: the plan, the ring, the
    (kernel, kind) paths of its launches, the family's kernel, the depth."""
    fam, dtype, n, tag = case["family"], case["dtype"], case["n"], (case["id"], k)
    assert plan["k"] == k and plan["pipe"] == 0, (tag, plan)
    assert plan["main_strip_w"] == M.strip_width(dtype) and plan["main_useful_w"] == M.useful(dtype, k), (tag, plan)
    if case["mode"] == "split":
        assert plan["valid"] in (1, 3) and plan["edge_items"] > 0, (tag, plan)
    else:
        assert plan["valid"] == 2 and plan["order"] == "single", (tag, plan)
    if fam == "plain":
        assert plan["ring"] == case["ring"], (tag, plan)
    ran = M.kinds_run(dtype, k, n, plan, fam)
    assert ran >= M.need(case), (tag, sorted(M.need(case) - ran), plan)
    assert info["tb"] == k and info["arith"] == M.ARITH.index(case["arith"]), (tag, info["tb"], info["arith"])
    if fam == "ins":
        assert (info["bc_x"], info["bc_y"]) == ("insulated", "insulated"), tag
    if fam == "src":
        assert info["source"]["set"] and info["source"]["max_tb"] >= k, (tag, info["source"])
    if fam == "var":
        assert info["rmap"]["set"] and info["rmap"]["max_tb"] >= k, (tag, info["rmap"])
    assert hist.get(k, 0) >= 2 and max(hist) == k, (tag, hist)


def run_case(case, monkeypatch):
    """Every depth of one table row. A mismatch is recorded and the loop goes
    on; an exception from the solver is not caught (nothing else is started on
    the GPU by this test after a HIP error, not even a close())."""
    setenv(monkeypatch, case)
    dtype, n, fam = case["dtype"], case["n"], case["family"]
    traj, bitwise = oracle(case)
    T0 = start_field(fam, dtype)
    kw = solver_kw(case)
    fails = []
    for k in case["depths"]:
        steps = 2 * k + 3
        p = problem(n, steps, case["sigma"])
        if case["arith"] in ("jacobi", "fast") and case["sigma"] == 0.25 or (fam == "ins" and case["arith"] == "fma"):
            assert p.r == 0.25
        s = HeatSolver(p, dtype=dtype, backend="hip", tb=k, device=0, arith=case["arith"], autotune=0, overlap=True,
                       graph=False, **kw)
        s.upload(T0 if fam != "plain" else T0[1:-1, 1:-1])
        for m in chunks(k):  # one cycle per call: two of depth k (test_step_counts_reach_depth)
            s.step(m)
        got, plan, info, hist = s.download(), s.plan(k), s.info(), s.cycle_hist()
        s.close()
        RUNS.append((case["id"], k))
        check_ran(case, k, plan, info, hist)
        if bitwise:
            bad = mismatch(got, traj[steps])
            if bad:
                fails.append((k,) + bad)
        else:
            d = float(np.abs(got.astype(np.float64) - traj[steps].astype(np.float64)).max())
            bound = fast_bound(case, steps)
            print(f"{case['id']} K={k}: max |fast - exact| = {d:.3e}, bound {bound:.3e}")
            if d > bound or (d == 0.0 and k > 1):  # (not the reference rounding on rough data)
                fails.append((k, d, ("bound", bound)))
    print(f"{case['id']}: {len(case['depths'])} solver runs ({len(RUNS)} so far in this process)")
    assert not fails, f"{case['id']}: (depth, max |diff|, first differing index) {fails}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", of("plain"), ids=ids(of("plain")))
def test_plain_instances(gpu, native, monkeypatch, case):
    """tb_kernel: every (dtype, ring, interior / general, form, depth) instance,
    in the split plan (interior kernel kinds 0 and 2, general kernel kinds 1
    and 3) and in a single general launch of three bands (kinds 0..3)."""
    run_case(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", of("ins"), ids=ids(of("ins")))
def test_insulated_instances(gpu, native, monkeypatch, case):
    """tb_kernel_ins, both axes insulated, depths 1..24, against
    models.reference.ftcs_step(bc_x=, bc_y=); fma at r = 1/4, where the
    reference expression has the contracted form's bits."""
    run_case(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", of("src"), ids=ids(of("src")))
def test_source_instances(gpu, native, monkeypatch, case):
    """tb_kernel_src, every depth the source kernels have, rough signed source,
    against models.reference.ftcs_step(source=) (fma: the true contracted form)."""
    run_case(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", of("var"), ids=ids(of("var")))
def test_map_instances(gpu, native, monkeypatch, case):
    """tb_kernel_var, every depth the map kernels have, rough map in (0, 0.25]
    with exact zeros, against models.reference.ftcs_step(rmap=)."""
    run_case(case, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("case", of("stats"), ids=ids(of("stats")))
def test_stats_instances(gpu, native, monkeypatch, case):
    """tb_kernel<general, ring 4, stats>: 4 forms x 48 depths. K + 1 steps as
    step(1), step_stats(K) with tb = K: the second call is one statistics cycle
    of depth K (asserted from step_cycles and cycle_hist); the statistics are held
    to the golden with the tolerances of tests/test_gpu_solver.py
    test_step_stats_fused (the scaled form at r != 1/4: those of
    tests/test_arith_fast.py test_hip_fast_step_stats), then step(K) and the
    field after 2 K + 1 steps bitwise (scaled form: within its bound).

    plan() does not report the statistics launch's band count. That its items
    reach kinds 0 and 2 as well as 1 and 3 rests on reading
    stencil_tb.hip launch_tb_stats / choose_bands: one round of items, so the
    cost falls strictly with the band count and the chooser returns
    rows // max(4 K, 16) (instance_matrix.stats_bands) — asserted >= 3 below, so
    a middle band clear of the frame rows exists (test_shapes_reach_every_kind)."""
    setenv(monkeypatch, case)
    dtype, n = case["dtype"], case["n"]
    traj, bitwise = oracle(case)
    T0 = start_field("plain", dtype)
    fails = []
    for k in case["depths"]:
        assert M.stats_bands(k, n) >= 3, (k, n)
        p = problem(n, 2 * k + 1, case["sigma"])
        s = HeatSolver(p, dtype=dtype, backend="hip", tb=k, device=0, arith=case["arith"], autotune=0, graph=False)
        s.upload(T0[1:-1, 1:-1])
        s.step(1)
        cycles = s.step_cycles(k)
        st = s.step_stats(k)
        mid = s.download()
        s.step(k)
        got, info, hist = s.download(), s.info(), s.cycle_hist()
        s.close()
        RUNS.append((case["id"], k))
        assert cycles == [k] and hist.get(k, 0) >= (2 if k > 1 else 3), (case["id"], k, cycles, hist)
        assert info["tb"] == k and info["arith"] == M.ARITH.index(case["arith"])
        T = traj[k + 1].astype(np.float64)
        d = T - traj[k].astype(np.float64)
        if bitwise:
            ok = (np.isclose(st["sum"], T.sum(), rtol=1e-12, atol=1e-9) and np.isclose(st["sum_sq"], (T * T).sum(), rtol=1e-12)
                  and st["min"] == T.min() and st["max"] == T.max()
                  and np.isclose(st["residual_l2"], np.sqrt((d * d).sum()), rtol=1e-10)
                  and st["residual_max"] == np.abs(d).max())
            bad = mismatch(mid, traj[k + 1]) or mismatch(got, traj[2 * k + 1])
        else:
            # statistics of the field the kernel stored; the residual against the reference rounding's
            # (fp64: the existing test's rtol; fp32: each of the two levels is within the form's stated
            # bound of the reference rounding, so their difference's maximum is within twice that)
            m64 = mid.astype(np.float64)
            tol = (dict(rtol=1e-6) if dtype == "fp64" else dict(rtol=0.0, atol=2 * fast_bound(case, k + 1)))
            ok = (np.isclose(st["sum"], m64.sum(), rtol=1e-12) and st["min"] == mid.min() and st["max"] == mid.max()
                  and np.isclose(st["residual_max"], np.abs(d).max(), **tol))
            worst = max(float(np.abs(m64 - T).max()) / fast_bound(case, k + 1),
                        float(np.abs(got.astype(np.float64) - traj[2 * k + 1].astype(np.float64)).max())
                        / fast_bound(case, 2 * k + 1))
            bad = (worst, ("of the bound",)) if worst > 1.0 else None
        if not ok:
            fails.append((k, "statistics", {key: float(v) for key, v in st.items()}))
        if bad:
            fails.append((k,) + bad)
    print(f"{case['id']}: {len(case['depths'])} solver runs ({len(RUNS)} so far in this process)")
    assert not fails, f"{case['id']}: (depth, max |diff|, first differing index) {fails}"
