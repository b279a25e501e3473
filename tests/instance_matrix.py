"""The case table of tests/test_instance_matrix.py and the launch geometry it
rests on, in plain Python (no torch, no GPU, no native library at import).

cases() lists one row per (family, dtype, ring, arithmetic variant, mode); every
row runs all of its depths, and claimed_instances() names the template
instances of the library a row executes, so the table can be held against the
instances read out of the built code objects (no exclusion list).

The geometry functions mirror the host planner and the kernels' item lookup
line by line, so that kinds_run() can say from the plan a solver reports which
(kernel, edge kind) code paths its launches execute:

    kernel "main" tb_kernel<MAIN = true>  (kinds 0 and 2)
           "gen"  tb_kernel<MAIN = false> (kinds 0..3)
           "ins" / "src" / "var"  the insulated / heat-source / diffusivity-map kernels
    kind   bit 0: the item's march reaches a global frame row,
           bit 1: its strip reaches a frame column.
"""

DTYPES = ("fp64", "fp32")
ARITH = ("exact", "fma", "jacobi", "fast")  # the kernels' AR template argument, in order
MAX_TB = 24
# the smallest grids at which every (kernel, kind) path exists at every depth
# (tests/test_instance_matrix.py test_shapes_reach_every_kind): a strip clear of
# both frame columns needs n >= U + W - KA (fp64 250, fp32 500 at the worst depth)
N_OF = {"fp64": 301, "fp32": 517}

# variant -> (arith, sigma): see tests/test_instance_matrix.py for the oracles
VARIANTS = {"exact": ("exact", 0.2), "fma": ("fma", 0.2), "jacobi": ("jacobi", 0.25),
            "fast_quarter": ("fast", 0.25), "fast": ("fast", 0.2)}

MODES = {"split": {}, "single": {"HEAT2D_SPLIT_ORDER": "single", "HEAT2D_BANDS": "3"}}
# the (kernel, kind) paths a mode must execute, whatever the depth
NEED = {"split": {("main", 0), ("main", 2), ("gen", 1), ("gen", 3)},
        "single": {("gen", 0), ("gen", 1), ("gen", 2), ("gen", 3)}}


# ------------------------------------------------------------------ geometry

def vec_elems(dtype):
    """stencil_tb.hip vec_elems: elements per 16-byte lane."""
    return 4 if dtype == "fp32" else 2


def strip_width(dtype):
    """tb_impl.hpp TbShape::W = 64 * V."""
    return 64 * vec_elems(dtype)


def halo_cols(dtype, k):
    """stencil_tb.hip halo_cols: (k + v - 1) / v * v (TbShape::KA)."""
    v = vec_elems(dtype)
    return (k + v - 1) // v * v


def useful(dtype, k):
    """stencil_tb.hip useful_width: 64 * v - 2 * halo_cols (TbShape::U)."""
    return strip_width(dtype) - 2 * halo_cols(dtype, k)


def nstrips(dtype, k, n):
    """stencil_tb.hip plan_split / plan_single: ns = (ncols + U - 1) / U."""
    u = useful(dtype, k)
    return (n + u - 1) // u


def strip_kind_cols(dtype, k, s, n):
    """tb_impl.hpp tb_kernel, the column half of `ek`:
    c0 = strip * U - KA; ((c0 < 0) || (c0 + W > ncols)) ? 2 : 0."""
    c0 = s * useful(dtype, k) - halo_cols(dtype, k)
    return 2 if (c0 < 0 or c0 + strip_width(dtype) > n) else 0


def item_kind_rows(t0, t1, k, n):
    """tb_impl.hpp tb_kernel, the row half of `ek`:
    ((t0 - K < fixed_lo) || (t1 + K > fixed_hi)) ? 1 : 0, with fixed_lo = 0 and
    fixed_hi = n on one rank (stencil_tb.hip launch_rects_1: -row0, nrows_global - row0)."""
    return 1 if (t0 - k < 0 or t1 + k > n) else 0


def rect_pieces(rect):
    """Every (strip, t0, t1) the items of one rect [r0, r1, s0, s1, nb] march:
    tb_impl.hpp tb_span (an item's range [lin, lin_end) of the strip-major row
    sequence: nb > 0 row bands, band-major; nb < 0 segments) and tb_piece (the
    cut of that range at strip ends)."""
    r0, r1, s0, s1, nb = rect
    ns, rows = s1 - s0, r1 - r0
    if ns <= 0 or rows <= 0 or nb == 0:  # launch_rects_1 skips such rects
        return
    for local in range(nb * ns if nb > 0 else -nb):
        if nb > 0:
            band = local // ns
            sl = local - band * ns
            lin, lin_end = sl * rows + band * rows // nb, sl * rows + (band + 1) * rows // nb
        else:
            total, nseg = ns * rows, -nb
            lin, lin_end = local * total // nseg, (local + 1) * total // nseg
        while lin < lin_end:
            sl = lin // rows
            row = lin - sl * rows
            t0 = r0 + row
            t1 = t0 + min(rows - row, lin_end - lin)
            yield s0 + sl, t0, t1
            lin += t1 - t0


def edges_on_main(k, n, rects):
    """stencil_tb.hip edges_on_main: the boundary-band rects run on the interior
    kernel only if none of their marches reaches a global frame row."""
    return all(not (r[1] > r[0] and (r[0] - k < 0 or r[1] + k > n)) for r in rects)


def kinds_run(dtype, k, n, plan, family="plain"):
    """The set of (kernel, kind) code paths the launches of `plan` (the dict of
    HeatSolver.plan(k): valid, main_rect, main_rects, edge_rects) execute on one
    rank of an n x n grid: stencil_tb.hip launch_split picks the rects and the
    kernel, tb_kernel the kind per piece.

    family "plain": tb_kernel. "ins" (both axes insulated): the general launches
    and, carved out of the interior launch, the strips that reach a frame column
    run tb_kernel_ins (stencil_tb.hip launch_rects); the rest of the interior
    stays on tb_kernel<MAIN>. "src" / "var": every launch runs that kernel."""
    valid = plan["valid"]
    if valid not in (1, 2, 3):
        raise ValueError(f"not a split or single-launch plan: valid = {valid}")
    main = plan["main_rects"] or [plan["main_rect"]]  # launch_split: p.nrects > 0 ? p.rects : &p.main
    other = {"plain": "gen", "ins": "ins", "src": "src", "var": "var"}[family]
    out = set()

    def add(rects, interior):
        for rect in rects:
            for s, t0, t1 in rect_pieces(rect):
                kc = strip_kind_cols(dtype, k, s, n)
                if not interior:
                    out.add((other, kc | item_kind_rows(t0, t1, k, n)))
                elif family in ("src", "var"):
                    out.add((other, kc))
                elif family == "ins" and kc:
                    out.add(("ins", kc | item_kind_rows(t0, t1, k, n)))  # carved frame strips: any banding, same rows
                else:
                    out.add(("main", kc))  # tb_kernel<MAIN>: the column test alone

    if valid == 2:
        add(main, False)
    else:
        add(main, True)
        add(plan["edge_rects"], edges_on_main(k, n, plan["edge_rects"]))
    return out


def need(case):
    """The (kernel, kind) paths every depth of `case` must execute."""
    fam, mode = case["family"], case["mode"]
    if fam == "plain":
        return NEED[mode]
    if fam == "ins":
        return ({("main", 0), ("ins", 2), ("ins", 1), ("ins", 3)} if mode == "split"
                else {("ins", e) for e in range(4)})
    return {(fam, e) for e in range(4)}


def stats_bands(k, n):
    """The band count of the fused-statistics launch (stencil_tb.hip
    launch_tb_stats takes choose_bands' result): with one round of items the
    chooser's cost (S / (nb ns)) (1 + 2k nb / rows) falls strictly with nb, so
    it returns nb_max = rows / max(4k, 16) (at least 1)."""
    return max(1, n // max(4 * k, 16))


# ------------------------------------------------------------------ the table

def _depths(dtype, ring):
    # stencil_tb.hip ring_ok: fp32 K > 16 exists with ring 4 only; ring 8 is fp32, K <= 16, single launches
    return list(range(1, (16 if (dtype == "fp32" and ring != 4) else MAX_TB) + 1))


def cases(src_depth=16, var_depth=16):
    """One row per GPU test id. src_depth / var_depth: the deepest pass of the
    source / map kernels (info()["source"]["max_tb"], info()["rmap"]["max_tb"])."""
    out = []

    def row(family, dtype, ring, variant, arith, sigma, mode, depths, env=None):
        e = dict(MODES[mode] if mode in MODES else {})
        if ring and family == "plain":
            e["HEAT2D_TB_RING"] = str(ring)
        e.update(env or {})
        out.append(dict(family=family, dtype=dtype, ring=ring, variant=variant, arith=arith, sigma=sigma, mode=mode,
                        depths=list(depths), n=N_OF[dtype], env=e,
                        id=f"{family}-{dtype}-r{ring}-{variant}-{mode}"))

    for dtype in DTYPES:
        for ring, modes in ((4, ("split", "single")), (6, ("split", "single")), (8, ("single",))):
            if ring == 8 and dtype != "fp32":
                continue
            for variant, (arith, sigma) in VARIANTS.items():
                for mode in modes:
                    row("plain", dtype, ring, variant, arith, sigma, mode, _depths(dtype, ring))
    # fused statistics: the general kernel, ring 4, one launch over the whole slab
    for dtype in DTYPES:
        for variant, (arith, sigma) in VARIANTS.items():
            row("stats", dtype, 4, variant, arith, sigma, "stats", range(1, MAX_TB + 1))
    for dtype in DTYPES:
        for mode in ("split", "single"):
            # (fma at r = 1/4: the reference expression gives the contracted form's bits there)
            for variant, arith, sigma in (("exact", "exact", 0.2), ("fma", "fma", 0.25), ("jacobi", "jacobi", 0.25)):
                row("ins", dtype, 4, variant, arith, sigma, mode, range(1, MAX_TB + 1))
            for variant in ("exact", "fma"):
                row("src", dtype, 4, variant, variant, 0.2, mode, range(1, src_depth + 1))
                row("var", dtype, 4, variant, variant, 0.2, mode, range(1, var_depth + 1))
    return out


def claimed_instances(case):
    """The template instances the runs of `case` execute. plain / stats: the
    tuples tools/isa_report.tb_params returns, (dtype, NV, K, RING, MAIN, AR[,
    "stats"]); ins / src / var: (dtype, NV, K, RING, AR) as tests/test_insulated_isa.py,
    test_source_isa.py and test_rmap_isa.py parse them."""
    dt, ring, ar = case["dtype"], case["ring"], ARITH.index(case["arith"])
    out = set()
    for k in case["depths"]:
        if case["family"] == "plain":
            out.add((dt, 1, k, ring, False, ar))  # split: the boundary bands; single: everything
            if case["mode"] == "split":
                out.add((dt, 1, k, ring, True, ar))
        elif case["family"] == "stats":
            out.add((dt, 1, k, 4, False, ar, "stats"))
        else:
            out.add((dt, 1, k, 4, ar))
    return out
