"""Negative controls for the oracle kernels of csrc/kernels/field_ops.hip.

The project's bitwise claims rest on ``HeatSolver.compare`` (compare_pass1 /
compare_pass2 on the device, the loop in Solver::compare on the host); every
other test only sees it report zero on fields that agree. Here it is given
fields that differ in known places — one ulp in a corner, the last column, the
first row a block reaches only by grid-striding, a NaN ahead of larger finite
differences in the same lane — and must return exactly what a NumPy reference
of the same contract returns. The statistics, row pack / unpack, streaming copy
and initial-condition kernels are checked the same way: against plain
high-precision references, on poisoned allocations, at the sizes where their
loops change shape. Device tests have a CPU-backend twin where the API has one:
different code, the same contract."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import heat2d
from heat2d.models import reference as R
from heat2d.models.heat2d import HeatSolver
from heat2d.ops import _native as N
from heat2d.ops import kernels as K
from heat2d.utils.config import IC_CONST, IcSpec

NPDT = {"fp64": np.float64, "fp32": np.float32}
UINT = {np.float64: np.uint64, np.float32: np.uint32}
TDT = {"fp64": torch.float64, "fp32": torch.float32}
TINT = {torch.float64: torch.int64, torch.float32: torch.int32}

DEV = [pytest.param("cpu", id="cpu"), pytest.param("cuda", marks=pytest.mark.gpu, id="gpu")]
DTYPES = ["fp64", "fp32"]


@pytest.fixture
def dev(request, native):
    if request.param == "cuda":
        request.getfixturevalue("gpu")
    return request.param


def problem(n, ic="uniform", steps=0):
    return heat2d.make_problem(heat2d.InputDat(n=n, sigma=0.25, nu=0.05, dom_len=2.0, ntime=steps), "ghost", ic)


# =============================================================== compare
def ref_compare(a, b):
    """The contract of HeatSolver.compare in NumPy: (max |a - b| in float64, NaN
    if any difference is NaN; number of elements whose bit patterns differ)."""
    U = UINT[a.dtype.type]
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    mx = 0.0 if d.size == 0 else (float("nan") if np.isnan(d).any() else float(d.max()))
    return mx, int(np.count_nonzero(a.view(U) != b.view(U)))


def same(got, want):
    """Exact agreement of a compare() result with the reference pair."""
    g, w = got["max_abs_diff"], want[0]
    return (g == w or (g != g and w != w)) and got["mismatches"] == want[1]


class Pair:
    """Two solvers on one problem with different layouts, holding the same
    rough data (values over three decades, as verify_decomposition uploads)."""

    def __init__(self, backend, n, dtype):
        self.backend, self.n, self.dtype = backend, n, dtype
        self.prob = problem(n)
        kw = dict(dtype=dtype, backend=backend, autotune=0, graph=False)
        self.a = HeatSolver(self.prob, halo=24, **kw)
        self.b = HeatSolver(self.prob, tb=4, halo=12, **kw)
        self.subs = {}
        self.base = (np.random.default_rng(n).random((n, n)) * 10.0 + 0.01).astype(NPDT[dtype])
        self.a.upload(self.base)
        self.b.upload(self.base)

    def sub(self, g0, rows):
        """A solver owning global rows [g0, g0 + rows) of the same grid."""
        if (g0, rows) not in self.subs:
            self.subs[g0, rows] = HeatSolver(self.prob, dtype=self.dtype, backend=self.backend, autotune=0,
                                             graph=False, rows=rows, slab_row0=g0, tb=1, overlap=False)
        return self.subs[g0, rows]

    def check(self, b, a=None):
        """Upload b (and a, default the base) and hold compare() to the reference."""
        try:
            if a is not None:
                self.a.upload(a)
            self.b.upload(b)
            want = ref_compare(self.base if a is None else a, b)
            got = self.a.compare(self.b)
            assert same(got, want), f"compare -> {got}, reference {want}"
            back = self.b.compare(self.a)  # symmetric
            assert same(back, want), f"reversed compare -> {back}, reference {want}"
            return got
        finally:
            if a is not None:
                self.a.upload(self.base)

    def close(self):
        for s in [self.a, self.b, *self.subs.values()]:
            s.close()


@pytest.fixture(scope="module")
def pairs(native):
    cache = {}

    def get(backend, n, dtype):
        if (backend, n, dtype) not in cache:
            cache[backend, n, dtype] = Pair(backend, n, dtype)
        return cache[backend, n, dtype]
    yield get
    for p in cache.values():
        p.close()


# n = 129: fewer columns than the 256 lanes of a block; 301: a column tail
# beyond one 256-lane pass; 2100: more rows than kCmpBlocks = 2048, so pass 1
# grid-strides and pass 2 reduces all 2048 partials. The CPU loop has no such
# thresholds: 150 and 301.
GRIDS = [pytest.param(("cpu", 150), id="cpu-150"), pytest.param(("cpu", 301), id="cpu-301")] + \
        [pytest.param(("hip", n), marks=pytest.mark.gpu, id=f"gpu-{n}") for n in (129, 301, 2100)]


@pytest.fixture
def pair(request, pairs):
    (backend, n), dtype = request.param
    if backend == "hip":
        request.getfixturevalue("gpu")
    return pairs(backend, n, dtype)


def on_grids(fn):
    params = [pytest.param((g.values[0], dt), marks=g.marks, id=f"{g.id}-{dt}") for g in GRIDS for dt in DTYPES]
    return pytest.mark.parametrize("pair", params, indirect=True)(fn)


def ulp_up(x):
    return np.nextafter(x, x.dtype.type(np.inf))


@on_grids
def test_upload_download_are_bit_exact(pair):
    """The precondition of everything below: download() returns the uploaded
    bytes — a NaN with a payload and -0.0 included — from either layout."""
    assert pair.a.layout.as_dict() != pair.b.layout.as_dict()
    U = UINT[pair.base.dtype.type]
    f = pair.base.copy()
    f[0, 0] = -0.0
    f.view(U)[pair.n - 1, pair.n - 1] = np.array(np.nan, f.dtype).view(U) | U(0x1234)  # NaN, payload bits set
    f[pair.n // 2, 1] = np.inf
    assert np.isnan(f[-1, -1]) and np.signbit(f[0, 0])
    for s in (pair.a, pair.b):
        try:
            s.upload(f)
            assert np.array_equal(s.download().view(U), f.view(U))
        finally:
            s.upload(pair.base)
        assert np.array_equal(s.download().view(U), pair.base.view(U))


@on_grids
def test_compare_identical(pair):
    assert pair.check(pair.base) == {"max_abs_diff": 0.0, "mismatches": 0}


@on_grids
def test_compare_one_ulp(pair):
    """One element one ulp off, anywhere: exactly one mismatch, exactly that ulp."""
    n = pair.n
    spots = [(0, 0), (0, n - 1), (n - 1, 0), (n - 1, n - 1), (n // 2, n // 2)]
    spots += [(1, c) for c in (255, 256) if c < n] + [(r, 7) for r in (2047, 2048, 2099) if r < n]
    for i, j in spots:
        b = pair.base.copy()
        b[i, j] = ulp_up(b[i, j])
        ulp = float(b[i, j]) - float(pair.base[i, j])
        got = pair.check(b)
        assert ulp > 0 and got == {"max_abs_diff": ulp, "mismatches": 1}, (i, j, got)


@on_grids
def test_compare_random_1000(pair):
    """1000 distinct elements moved by random amounts: exact count, exact maximum."""
    rng = np.random.default_rng(7)
    n = pair.n
    pos = rng.choice(n * n, 1000, replace=False)
    b = pair.base.copy()
    b.flat[pos] += (rng.uniform(1e-3, 1.0, 1000) * rng.choice([-1.0, 1.0], 1000)).astype(b.dtype)
    got = pair.check(b)
    assert got["mismatches"] == 1000 and 0.0 < got["max_abs_diff"] <= 1.0 + 1e-6


@on_grids
def test_compare_signed_zero(pair):
    """+0.0 against -0.0: no difference in value, one in bits."""
    n = pair.n
    for i, j in ((0, 0), (n - 1, n - 1)):
        a, b = pair.base.copy(), pair.base.copy()
        a[i, j], b[i, j] = 0.0, -0.0
        assert pair.check(b, a) == {"max_abs_diff": 0.0, "mismatches": 1}


@on_grids
def test_compare_nan_in_one_field(pair):
    """A NaN in one field is (NaN, 1) wherever it is, and stays NaN through the
    lane's running maximum, the LDS tree and pass 2 when larger finite
    differences come before and after it."""
    n = pair.n
    # (0, 5): the first element lane 5 of block 0 visits; the same lane goes on
    # to columns 261, 517, ... and (n > 2048) to row 2048
    later = [(0, c) for c in (261, 517) if c < n] + [(r, 5) for r in (2048,) if r < n] + [(0, 6), (1, 5)]
    cases = [((0, 5), later), ((n - 1, n - 1), [(0, 0), (n - 1, n - 2)])]
    if n > 2048:  # a row reached only by grid-striding, finite differences earlier (row 22) and later in its lane
        cases.append(((2070, 1000), [(22, 1000), (22, 232), (2070, 1256), (2099, 2099)]))
    for (i, j), finite in cases:
        b = pair.base.copy()
        b[i, j] = np.nan
        got = pair.check(b)
        assert math.isnan(got["max_abs_diff"]) and got["mismatches"] == 1, (i, j, got)
        for k, (fi, fj) in enumerate(finite):
            b[fi, fj] += 3.0 + k
        got = pair.check(b)
        assert math.isnan(got["max_abs_diff"]) and got["mismatches"] == 1 + len(finite), (i, j, got)
        b[i, j] = pair.base[i, j]  # without the NaN: the largest finite difference
        got = pair.check(b)
        assert got["mismatches"] == len(finite) and abs(got["max_abs_diff"] - (2.0 + len(finite))) < 1e-5


@on_grids
def test_compare_nan_and_inf_in_both_fields(pair):
    """The same NaN bits at the same place in both fields: (NaN, 0) — the bits
    agree, the value difference is NaN. +inf at the same place in both fields
    is (NaN, 0) as well: inf - inf is NaN in the reference arithmetic too, so a
    field holding an inf never compares clean. +inf in one field only: (inf, 1)."""
    n = pair.n
    for i, j in ((0, 0), (n // 2, n - 1), (n - 1, n - 1)):
        for v in (np.nan, np.inf, -np.inf):
            a = pair.base.copy()
            a[i, j] = v
            got = pair.check(a.copy(), a)
            assert math.isnan(got["max_abs_diff"]) and got["mismatches"] == 0, (i, j, v, got)
        b = pair.base.copy()
        b[i, j] = np.inf
        assert pair.check(b) == {"max_abs_diff": float("inf"), "mismatches": 1}
        a = pair.base.copy()
        a[i, j] = -np.inf  # +inf against -inf: inf, not NaN
        assert pair.check(b, a) == {"max_abs_diff": float("inf"), "mismatches": 1}


@on_grids
def test_compare_row_windows(pair):
    """compare(other, r0, nrows, other_r0) against a solver owning a sub-slab:
    differences in the rows just outside the window are not counted, those in
    its first and last row are."""
    n = pair.n
    g0, rows = n // 3, n // 2
    sub = pair.sub(g0, rows)
    assert (sub.row0, sub.nrows, sub.ncols) == (g0, rows, n)
    r0, nr = g0 + 10, rows - 25
    o0 = r0 - g0
    slab = pair.base[g0:g0 + rows]

    def check(b, want_mism):
        sub.upload(b)
        want = ref_compare(pair.base[r0:r0 + nr], b[o0:o0 + nr])
        got = pair.a.compare(sub, r0, nr, o0)
        assert same(got, want) and got["mismatches"] == want_mism, (got, want)
        assert same(sub.compare(pair.a, o0, nr, r0), want)
        return got

    assert check(slab, 0) == {"max_abs_diff": 0.0, "mismatches": 0}
    outside = [(o0 - 1, 0), (o0 - 1, n - 1), (o0 + nr, 0), (o0 + nr, n - 1)]
    inside = [(o0, 0), (o0, n - 1), (o0 + nr - 1, 0), (o0 + nr - 1, n - 1)]
    for i, j in outside:
        b = slab.copy()
        b[i, j] = np.nan
        assert check(b, 0) == {"max_abs_diff": 0.0, "mismatches": 0}, (i, j)
    for i, j in inside:
        b = slab.copy()
        b[i, j] = ulp_up(b[i, j])
        got = check(b, 1)
        assert got["max_abs_diff"] == float(b[i, j]) - float(slab[i, j]) > 0, (i, j)
    b = slab.copy()
    for k, (i, j) in enumerate(outside + inside):
        b[i, j] += 1.0 + k
    assert abs(check(b, 4)["max_abs_diff"] - 8.0) < 1e-5
    # the whole sub-slab, and an empty window anywhere
    want = ref_compare(pair.base[g0:g0 + rows], b)
    assert same(pair.a.compare(sub, g0, rows, 0), want) and want[1] == 8
    assert pair.a.compare(sub, r0, 0, o0) == {"max_abs_diff": 0.0, "mismatches": 0}
    assert pair.a.compare(sub, n, 0, rows) == {"max_abs_diff": 0.0, "mismatches": 0}


@on_grids
def test_compare_rejects_bad_arguments(pair, pairs):
    n = pair.n
    sub = pair.sub(n // 3, n // 2)
    for args in ((n - 5, 6, 0), (-1, 3, 0), (0, 3, -1), (0, n // 2 + 1, 0), (0, -1, 0)):
        with pytest.raises(N.NativeError, match="outside the owned slabs"):
            pair.a.compare(sub, *args)
    with pytest.raises(N.NativeError, match="outside the owned slabs"):
        pair.a.compare(pair.b, 1, n, 1)
    other_n = pairs(pair.backend, 301 if n != 301 else (150 if pair.backend == "cpu" else 129), pair.dtype)
    with pytest.raises(N.NativeError, match="differ in width"):
        pair.a.compare(other_n.a, 0, 5, 0)
    other_dt = pairs(pair.backend, n, "fp32" if pair.dtype == "fp64" else "fp64")
    with pytest.raises(N.NativeError, match="differ in dtype or backend"):
        pair.a.compare(other_dt.a)
    if pair.backend == "hip":
        host = pairs("cpu", 301, pair.dtype)
        with pytest.raises(N.NativeError, match="differ in dtype or backend"):
            pair.a.compare(host.a, 0, 1, 0)


# =============================================================== stats
def poisoned(L, tdt, device, values):
    """A field whose whole allocation is NaN except the owned region (= values)."""
    f = K.empty_field(L, tdt, device)
    K.view2d(f, L).fill_(float("nan"))
    K.owned(f, L).copy_(torch.as_tensor(values).to(device))
    return f


def check_stats(st, v, o=None):
    """K.stats against math.fsum over the float64 values. The sums are plain
    recursive / tree summations of N terms: |sum - exact| <= N u sum|v| and,
    with one more rounding for each square and one for the reference,
    (N + 2) u sum v^2, u = 2^-53. min, max and the maximum difference are exact."""
    v = np.asarray(v, np.float64).ravel()
    n, u = v.size, 2.0 ** -53
    assert abs(st["sum"] - math.fsum(v)) <= n * u * math.fsum(np.abs(v))
    sq = math.fsum(v * v)
    assert abs(st["sum_sq"] - sq) <= (n + 2) * u * sq
    assert st["min"] == v.min() and st["max"] == v.max()
    if o is not None:
        d = v - np.asarray(o, np.float64).ravel()
        dd = math.fsum(d * d)
        assert abs(st["diff_l2"] ** 2 - dd) <= (n + 2) * u * dd
        assert st["diff_max"] == np.abs(d).max()
    else:
        assert "diff_l2" not in st and "diff_max" not in st


# (1, 1): one element; (30, 30): most of the 1024 blocks own no row, their
# DBL_MAX / -DBL_MAX seeds must not reach the result; (5, 1000): column tails;
# (1500, 37): more rows than blocks
STATS_LAYOUTS = [(1, 1, 4), (30, 30, 4), (5, 1000, 16), (1500, 37, 8)]


@pytest.mark.parametrize("dev", DEV, indirect=True)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", STATS_LAYOUTS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_stats(dev, dtype, shape):
    nrows, ncols, halo = shape
    L = K.make_layout(nrows, ncols, halo=halo)
    rng = np.random.default_rng(nrows * 1000 + ncols)
    for sign in ("mixed", "negative", "positive"):
        v = (rng.random((nrows, ncols)) * 10.0 + 0.01).astype(NPDT[dtype])
        if sign == "negative":
            v = -v
        elif sign == "mixed":
            v = (v - 5.0).astype(NPDT[dtype])
        o = (v + rng.standard_normal((nrows, ncols))).astype(NPDT[dtype])
        f = poisoned(L, TDT[dtype], dev, v)
        g = poisoned(L, TDT[dtype], dev, o)
        st = K.stats(f, L)
        check_stats(st, v)  # finite: no pad or ghost element was read
        st2 = K.stats(f, L, other=g)
        check_stats(st2, v, o)
        assert all(st2[k] == st[k] for k in st)
        # a fixed reduction order: the same bits on every call
        again = K.stats(f, L, other=g)
        assert all(np.float64(again[k]).view(np.uint64) == np.float64(st2[k]).view(np.uint64) for k in st2)


@pytest.mark.parametrize("dev", DEV, indirect=True)
@pytest.mark.parametrize("dtype", DTYPES)
def test_stats_nan_in_the_field(dev, dtype):
    """A NaN in the owned field is not lost: sum and sum_sq are NaN."""
    for nrows, ncols, at in ((30, 30, (29, 29)), (1500, 37, (1499, 0)), (5, 1000, (0, 999))):
        L = K.make_layout(nrows, ncols, halo=4)
        v = np.random.default_rng(3).random((nrows, ncols)).astype(NPDT[dtype])
        v[at] = np.nan
        st = K.stats(poisoned(L, TDT[dtype], dev, v), L)
        assert math.isnan(st["sum"]) and math.isnan(st["sum_sq"])


# =============================================================== pack / unpack
def random_bits(n, tdt, seed):
    """n elements of random bit patterns (NaNs, infs, subnormals among them)."""
    rng = np.random.default_rng(seed)
    if tdt == torch.float64:
        raw = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.int64)
    else:
        raw = rng.integers(0, 2 ** 32, n, dtype=np.uint32).view(np.int32)
    return torch.from_numpy(raw).view(tdt)


def bits(t):
    return t.contiguous().view(TINT[t.dtype]).cpu()


PACK_LAYOUTS = [(12, 9, 4), (40, 261, 24), (3, 1030, 16)]


@pytest.mark.parametrize("dev", DEV, indirect=True)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", PACK_LAYOUTS, ids=lambda s: f"{s[0]}x{s[1]}h{s[2]}")
def test_pack_unpack_rows(dev, dtype, shape):
    nrows, ncols, halo = shape
    tdt = TDT[dtype]
    L = K.make_layout(nrows, ncols, halo=halo)
    f = random_bits(L.elems(), tdt, 11).to(dev)
    fv = bits(K.view2d(f, L))
    # from row 0, in the middle, from the first ghost row into the owned rows,
    # up to the last ghost row, and every allocated row
    ranges = [(0, min(3, nrows)), (nrows // 2, 1), (-halo, halo + 1), (nrows - 1, halo + 1),
              (-halo, nrows + 2 * halo)]
    for row, k in ranges:
        rs = slice(halo + row, halo + row + k)
        cs = slice(L.cpad, L.cpad + ncols)
        buf = K.pack_rows(f, L, row, k)
        assert buf.shape == (k * ncols,) and buf.device == f.device
        assert torch.equal(bits(buf).view(k, ncols), fv[rs, cs]), (row, k)
        # unpack into a NaN-filled field: exactly the target rectangle changes
        g = torch.full((L.elems(),), float("nan"), dtype=tdt, device=dev)
        want = bits(K.view2d(g, L)).clone()
        src = random_bits(k * ncols, tdt, 100 + row + halo).to(dev)
        want[rs, cs] = bits(src).view(k, ncols)
        K.unpack_rows(g, L, row, k, src)
        assert torch.equal(bits(K.view2d(g, L)), want), (row, k)
        # round trips
        assert torch.equal(bits(K.pack_rows(g, L, row, k)), bits(src))
        h = f.clone()
        K.unpack_rows(h, L, row, k, buf)
        assert torch.equal(bits(h), bits(f))
    assert torch.equal(bits(K.view2d(f, L)), fv)  # pack reads only


# =============================================================== copy
@pytest.mark.gpu
@pytest.mark.parametrize("blocks", [1, 2])
def test_copy_kernel_loops_and_tails(native, gpu, blocks):
    """heat2d_copy with a grid of 1 or 2 blocks (stride 256 / 512 vectors): the
    4-way unrolled loop runs while i + 3 stride < n16, the tail loop after it —
    sizes on either side of every boundary, each copied exactly with the 64
    bytes behind the destination untouched."""
    stride = 256 * blocks
    sentinel = 0x5A5A5A5A
    for n16 in (0, 1, stride - 1, 3 * stride, 3 * stride + 1, 4 * stride, 4 * stride + 1, 11 * stride + 5):
        src = torch.from_numpy(np.random.default_rng(n16).integers(-2 ** 31, 2 ** 31, 4 * n16 + 4, dtype=np.int64)
                               .astype(np.int32)).cuda()
        dst = torch.full((4 * n16 + 16,), sentinel, dtype=torch.int32, device="cuda")
        N.call("heat2d_copy", C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), 16 * n16, K._stream(src), blocks)
        torch.cuda.synchronize()
        assert torch.equal(dst[:4 * n16], src[:4 * n16]), n16
        assert bool((dst[4 * n16:] == sentinel).all()), n16


def test_copy_rejects_partial_vectors(native):
    """A byte count that is not a multiple of 16 is refused before any launch."""
    buf = (C.c_char * 64)()
    for nbytes in (8, 24, 33):
        with pytest.raises(N.NativeError, match="multiple of 16"):
            N.call("heat2d_copy", C.cast(buf, C.c_void_p), C.cast(buf, C.c_void_p), nbytes, None, 1)


@pytest.mark.parametrize("dev", DEV, indirect=True)
def test_copy_small_and_default_grid(dev):
    """K.copy_: 3 fp32 elements (12 bytes) take the torch fallback; a field of a
    few hundred KB takes the kernel at its default grid. Both exact."""
    for n, tdt in ((3, torch.float32), (5, torch.float64), (70001 * 2, torch.float64), (4 * 30011, torch.float32)):
        src = random_bits(n, tdt, n).to(dev)
        dst = torch.zeros_like(src)
        K.copy_(dst, src)
        assert torch.equal(bits(dst), bits(src))


# =============================================================== init_field
def ic_cases(p):
    """The ICs with a distinguishable pad value."""
    mk = lambda name: dataclasses.replace(heat2d.utils.config.make_ic(name, p.dom_len, p.x), pad=-7.25)  # noqa: E731
    return {"uniform": mk("uniform"), "hat": mk("hat"), "hotspot": mk("hotspot"), "python-hat": mk("python-hat"),
            "const": IcSpec(kind=IC_CONST, a=3.5, pad=-7.25)}


# a full slab, and the last rank's slab: its ghost rows past the global frame hold the pad
SLABS = [pytest.param((70, 0), id="full"), pytest.param((23, 47), id="last-rank")]
N_INIT = 70


def init_on(device, dtype, ic, p, nrows, row0, halo=16):
    L = K.make_layout(nrows, N_INIT, halo=halo, row0=row0, nrows_global=N_INIT)
    f = torch.full((L.elems(),), float("nan"), dtype=TDT[dtype], device=device)
    K.init_field(f, L, ic, p.x)
    return L, K.view2d(f, L).cpu().numpy()


def check_init_against_golden(v, L, ic, p, dtype):
    """Rows / columns -1 .. n of the allocation are the golden initial field;
    everything past the global frame is the pad."""
    nrows, row0, h, c, n = L.nrows, L.row0, L.halo, L.cpad, L.ncols
    U = UINT[NPDT[dtype]]
    gold = R.initial_field(dataclasses.replace(p, ic=ic), NPDT[dtype])
    lo = max(-h, -1 - row0)  # first local row inside the frame
    hi = n + 1 - row0        # one past the last (the frame row n is local row n - row0)
    got = v[h + lo:h + hi, c - 1:c + n + 1]
    assert np.array_equal(got.view(U), gold[row0 + lo + 1:row0 + hi + 1].view(U))
    mask = np.ones(v.shape, bool)
    mask[h + lo:h + hi, c - 1:c + n + 1] = False
    assert np.array_equal(v[mask].view(U), np.full(mask.sum(), ic.pad, NPDT[dtype]).view(U))
    assert mask[h + hi:].all() and (row0 == 0 or hi < nrows + h)  # last rank: ghost rows past the frame exist


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slab", SLABS)
@pytest.mark.parametrize("name", ["uniform", "hat", "hotspot", "python-hat", "const"])
def test_init_field_cpu_matches_golden(native, name, slab, dtype):
    p = problem(N_INIT)
    ic = ic_cases(p)[name]
    L, v = init_on("cpu", dtype, ic, p, *slab)
    assert not np.isnan(v).any()  # every element of the allocation is written
    check_init_against_golden(v, L, ic, p, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slab", SLABS)
@pytest.mark.parametrize("name", ["uniform", "hat", "hotspot", "python-hat", "const"])
def test_init_field_gpu_matches_cpu_everywhere(native, gpu, name, slab, dtype):
    """The device allocation equals the CPU twin's bitwise over every element,
    pads and ghost rows included, and its frame-inclusive part the golden field."""
    p = problem(N_INIT)
    ic = ic_cases(p)[name]
    U = UINT[NPDT[dtype]]
    L, host = init_on("cpu", dtype, ic, p, *slab)
    _, dev_ = init_on("cuda", dtype, ic, p, *slab)
    assert np.array_equal(dev_.view(U), host.view(U))
    check_init_against_golden(dev_, L, ic, p, dtype)


def sine_reference(p, ic, g0, g1):
    """The kernel's formula, a sin(kx pi (x - x0) / (x1 - x0)) sin(ky pi (y - y0) / (y1 - y0))
    with the same double-precision constants, evaluated in long double: global rows [g0, g1)."""
    ld = np.longdouble
    x = p.x.astype(ld)
    pi = ld(np.pi)  # M_PI: the double nearest pi, as the kernel uses
    sx = np.sin(ld(ic.kx) * pi * (x - ld(ic.x0)) / (ld(ic.x1) - ld(ic.x0)))
    sy = np.sin(ld(ic.ky) * pi * (x - ld(ic.y0)) / (ld(ic.y1) - ld(ic.y0)))
    full = ld(ic.a) * sx[:, None] * sy[None, :]
    return full[1 + g0:1 + g1, 1:-1]


def sine_case(dtype, slab, device):
    """The sine IC on a slab: (layout, allocation, mask of the grid-interior
    points in it — the slab's own rows and the neighbour's rows in its upper
    ghost rows —, max error of those against long double, NumPy float64's own)."""
    p = problem(N_INIT, "sine")
    ic = dataclasses.replace(p.ic, a=1.75, kx=2.0, ky=3.0, pad=-7.25)
    nrows, row0 = slab
    L, v = init_on(device, dtype, ic, p, nrows, row0)
    h, c, n = L.halo, L.cpad, L.ncols
    g0, g1 = max(0, row0 - h), min(N_INIT, row0 + nrows + h)  # global interior rows the allocation holds
    inner = np.zeros(v.shape, bool)
    inner[h + g0 - row0:h + g1 - row0, c:c + n] = True
    ref = sine_reference(p, ic, g0, g1)
    err = float(np.abs(v[inner].reshape(ref.shape).astype(np.longdouble) - ref).max())
    # NumPy float64's own error in the same formula (cast to the field's dtype like the kernel's store)
    gold = R.owned(R.initial_field(dataclasses.replace(p, ic=ic), NPDT[dtype]))[g0:g1]
    base = float(np.abs(gold.astype(np.longdouble) - ref).max())
    return L, v, inner, err, base


@pytest.mark.parametrize("dev", DEV, indirect=True)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slab", SLABS)
def test_init_field_sine(dev, dtype, slab):
    """The sine IC: frame exactly 0.0, frame, pads and the ghost rows past it
    bitwise the CPU twin's, every grid-interior point within 4x NumPy float64's
    own error against a long-double evaluation of the same formula (device sin
    and host libm are different implementations of it)."""
    L, v, inner, err, base = sine_case(dtype, slab, dev)
    host = sine_case(dtype, slab, "cpu")[1]
    nrows, row0, h, c, n = L.nrows, L.row0, L.halo, L.cpad, L.ncols
    U = UINT[NPDT[dtype]]
    assert inner.sum() == (nrows + (h if row0 else 0)) * n
    assert np.array_equal(v[~inner].view(U), host[~inner].view(U))
    zero = np.zeros(1, NPDT[dtype]).view(U)[0]
    if row0 == 0:
        assert (v[h - 1, c - 1:c + n + 1].view(U) == zero).all()  # the global frame row -1
    assert (v[h + N_INIT - row0, c - 1:c + n + 1].view(U) == zero).all()  # the global frame row n
    assert (v[h:h + nrows, c - 1].view(U) == zero).all() and (v[h:h + nrows, c + n].view(U) == zero).all()
    assert (v[h + N_INIT - row0 + 1:] == -7.25).all()
    # measured on the 70 x 70 grid, a = 1.75, kx = 2, ky = 3 (max |error| against long double):
    #   fp64: NumPy 2.932e-15, CPU twin 2.932e-15, gfx950 device 2.932e-15
    #   fp32: NumPy 5.955e-08, CPU twin 5.955e-08, gfx950 device 5.955e-08
    # (both slabs alike: the argument's rounding, 3 pi here, dominates all three)
    print(f"sine IC {dtype} {dev} slab={slab}: max error {err:.3e}, NumPy float64 {base:.3e}")
    assert 0 < base and err <= 4 * base
