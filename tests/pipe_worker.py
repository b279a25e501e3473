"""Worker for tests/test_gpu_pipe.py.

`python tests/pipe_worker.py OUTDIR`: runs every case of CASES on the GPU in
this process — HEAT2D_PIPE (the wave-pair interior kernel: 1 forced, 0 off) is
read once per process, so the test starts one worker per value — and writes
OUTDIR/<case>.npy (the final owned field) and OUTDIR/info.json (per case: the
plan of depth tb and, per member, cycle_hist() and the plan of every depth in it).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cycles import calls  # noqa: E402

# useful width of a wide strip (256 columns, halo of k rounded up to whole 4-double lanes)
def useful(k):
    return 256 - 2 * ((k + 3) // 4 * 4)


def halo(k):
    return (k + 3) // 4 * 4


def kind0_strips(n, k):
    """Wide strips of an n-column grid that reach no frame column: the kernel's
    scaled (kind 0) items — c0 = s U - KA >= 0 and c0 + 256 <= n."""
    u, ka = useful(k), halo(k)
    return [s for s in range(-(-n // u)) if s * u - ka >= 0 and s * u - ka + 256 <= n]


def cases():
    """name -> dict(n, tb, steps, ic, arith, env, kind; calls: the step() calls
    that make up `steps`; also: further depths the case names). Grids are
    square: the column cases set n around the wide strip's useful width U(tb),
    the row cases take the thinnest slab the split accepts (6 tb rows: an
    interior of 4 tb) and cut it into bands of 2 tb rows (5 FIFO depths).

    Every case makes its steps with cycles.calls(): one or two step(tb) calls —
    one cycle of depth tb each — and the remainder in a last call, which runs
    balanced cycles (one step(2 tb + 3) call runs three cycles of depth about
    2 tb / 3 and never one of depth tb; the pair kernel exists at depths 16..24
    only). The cases that run several items per pair, the dynamic queue or
    segments run depth tb twice: the second launch finds the queue and the
    FIFO flags as the first one left them."""
    c = {}

    def add(name, tb, steps, full=1, **kw):
        c[name] = dict(tb=tb, steps=steps, calls=calls(tb, steps, full), **kw)

    u20 = useful(20)
    # columns, depth 20 (K1 = K2 = 10): one kind-2 strip holding both frame columns; U - 1, U, U + 1; 2 strips + a partial one
    for name, n in [("cols_lt_u", 150), ("cols_u_minus_1", u20 - 1), ("cols_u", u20), ("cols_u_plus_1", u20 + 1),
                    ("cols_2u_partial", 2 * u20 + 37)]:
        add(name, 20, 2 * 20 + 3, 2, n=n, ic="rough")
    # rows: the thinnest interior the split accepts; short bands so the FIFO wraps several times per item
    add("rows_thinnest", 20, 20, n=6 * 20, ic="rough")
    add("rows_short_bands", 20, 2 * 20, 2, n=8 * 20 + 1, ic="rough", env={"HEAT2D_BANDS": "3"})
    # more items than pairs: each pair runs several items back to back (static stride, dynamic queue).
    # (2 tb + 5 steps, raised from tb + 5: two cycles of depth tb and a 5-step one)
    add("items_static", 20, 2 * 20 + 5, 2, n=2 * u20 + 37, ic="rough", env={"HEAT2D_BANDS": "5", "HEAT2D_MAX_WAVES": "2"})
    add("items_dynamic", 20, 2 * 20 + 5, 2, n=2 * u20 + 37, ic="rough",
        env={"HEAT2D_BANDS": "5", "HEAT2D_MAX_WAVES": "2", "HEAT2D_DYNAMIC": "1"})
    # segment plans whose pieces cross a strip end (static and dynamic; 2 tb + 5 steps raised from
    # tb + 5, 2 tb from tb: depth tb twice)
    add("segments", 20, 2 * 20 + 5, 2, n=2 * u20 + 37, ic="rough", env={"HEAT2D_SEGMENTS": "7"})
    add("segments_dynamic", 20, 2 * 20, 2, n=2 * u20 + 37, ic="rough",
        env={"HEAT2D_SEGMENTS": "11", "HEAT2D_MAX_WAVES": "3", "HEAT2D_DYNAMIC": "1"})
    # depths: 16, 19 and 21 (K1 != K2), 24 — three strips, the middle one of
    # kind 0 (scaled levels, one unscale at the store: needs n >= 2 U + KA)
    for k in (16, 19, 21, 24):
        add(f"depth_{k}", k, 2 * k + 1, 2, n=2 * useful(k) + 37, ic="rough", kind0=True)
    # ... and the deep ones with several items per pair: bands through the dynamic queue, segments
    # across strip ends (2 tb + 5 steps raised from tb + 5, 2 tb from tb: depth tb twice)
    add("depth_24_items", 24, 2 * 24 + 5, 2, n=2 * useful(24) + 37, ic="rough", kind0=True,
        env={"HEAT2D_BANDS": "4", "HEAT2D_MAX_WAVES": "2", "HEAT2D_DYNAMIC": "1"})
    add("depth_21_segments", 21, 2 * 21 + 5, 2, n=2 * useful(21) + 37, ic="rough", kind0=True,
        env={"HEAT2D_SEGMENTS": "7", "HEAT2D_MAX_WAVES": "3"})
    add("depth_19_items", 19, 2 * 19, 2, n=2 * useful(19) + 37, ic="rough", kind0=True,
        env={"HEAT2D_BANDS": "4", "HEAT2D_MAX_WAVES": "2"})
    # the reference IC (smooth, values in [1, 2])
    add("reference_ic", 20, 2 * 20, 2, n=u20 + 1, ic="uniform")
    # the other arithmetic forms' instances, kind-0 strip included: at r = 1/4,
    # and the forms that take any r at sigma 0.2 (fast: scaled by 1 / r per level)
    for arith in ("exact", "fma", "fast"):
        add(f"arith_{arith}", 20, 20 + 3, n=2 * u20 + 37, ic="rough", arith=arith, kind0=True)
    for arith, k in (("exact", 21), ("fma", 20), ("fast", 19)):
        add(f"arith_{arith}_r02", k, k + 3, n=2 * useful(k) + 37, ic="rough", arith=arith, sigma=0.2, kind0=True)
    # every instance once (depths 16..24 x 4 forms): the cols_2u_partial shape of its depth (three
    # strips, the middle one of kind 0), 2 k + 3 steps: two full passes and a shallower one.
    # exact and fma at sigma 0.2; fast at r = 1/4 (bitwise the jacobi form) at
    # even depths, at sigma 0.2 (within its bound) at odd ones
    for k in range(16, 25):
        for arith in ("exact", "fma", "jacobi", "fast"):
            sigma = 0.25 if arith == "jacobi" or (arith == "fast" and k % 2 == 0) else 0.2
            add(f"inst_{arith}_{k}", k, 2 * k + 3, 2, n=2 * useful(k) + 37, ic="rough", arith=arith, sigma=sigma, kind0=True)
    # graph replay: ONE call, whose pair branch replays the captured pair of depth tb while 2 tb steps are left
    c["graph"] = dict(n=u20 + 1, tb=16, steps=3 * 16, calls=[3 * 16], ic="rough", kind="graph")
    # loopback exchange between slabs: the boundary bands on the one-wave kernels, room left
    # beside the pairs for the exchange (spare_waves). Two slabs (both edge slabs) ...
    add("loopback", 16, 2 * 16 + 3, 2, n=2 * useful(16) + 37, ic="rough", kind="loopback", ranks=2)
    # ... three: a middle slab, both bands clear of the frame rows, between two edge slabs
    add("loopback_3", 20, 2 * 20 + 3, 2, n=2 * u20 + 37, ic="rough", kind="loopback", ranks=3)
    # ... and a deeper exchange after a pair cycle: ONE step(33) call at tb 17 runs 17, 16, and the
    # depth-16 cycle moves the 17 ghost rows the next call's first cycle reads, so it runs the plan
    # re-made over bands of B = 17 rows with the pipe flag kept (split_plan_banded(16, 17)). That plan
    # is valid while the thinnest slab leaves an interior rows - 2 B >= 4 k: 234 - 34 >= 64
    c["loopback_deeper_exchange"] = dict(n=2 * useful(17) + 37, tb=17, steps=33, calls=[33], also=[16], ic="rough",
                                         kind="loopback", ranks=2)
    return c


def problem(n, steps, sigma=0.25):
    import heat2d
    return heat2d.make_problem(heat2d.InputDat(n=n, sigma=sigma, nu=0.05, dom_len=1.0, ntime=steps), "ghost", "uniform")


def rough(n, seed=7):
    """Rough non-dyadic owned field, values 10**uniform(-1, 1)."""
    import numpy as np
    return 10.0 ** np.random.default_rng(seed).uniform(-1.0, 1.0, (n, n))


KNOBS = ("HEAT2D_BANDS", "HEAT2D_SEGMENTS", "HEAT2D_MAX_WAVES", "HEAT2D_DYNAMIC")
PLAN_KEYS = ("pipe", "valid", "dynamic", "main_bands", "main_items", "main_waves", "main_rect", "main_strip_w",
             "main_useful_w")


def main(outdir):
    import numpy as np
    import torch

    from heat2d.models.heat2d import HeatSolver, LoopbackGroup
    torch.cuda.set_device(0)
    info = {}
    for name, a in cases().items():
        for kn in KNOBS:
            os.environ.pop(kn, None)
        os.environ.update(a.get("env", {}))
        p = problem(a["n"], a["steps"], a.get("sigma", 0.25))
        assert p.n_owned == a["n"] and sum(a["calls"]) == a["steps"]
        arith = a.get("arith", "jacobi")
        kind = a.get("kind", "solver")
        if kind == "loopback":
            g = LoopbackGroup(p, a["ranks"], dtype="fp64", backend="hip", tb=a["tb"], device=0, arith=arith, autotune=0)
            if a["ic"] == "rough":
                g.upload(rough(a["n"]))
            for m in a["calls"]:
                g.step(m)
            out = g.download()
            hists = [g.cycle_hist(i) for i in range(a["ranks"])]
            plans = [{k: g.plan(i, k) for k in sorted(h)} for i, h in enumerate(hists)]
            plan = g.plan(0, a["tb"])
            slabs = [int(nr) for _, nr in g.slabs()]
            g.close()
        else:
            s = HeatSolver(p, dtype="fp64", backend="hip", tb=a["tb"], device=0, arith=arith, autotune=0,
                           graph=(kind == "graph"))
            if a["ic"] == "rough":
                s.upload(rough(a["n"]))
            for m in a["calls"]:
                s.step(m)
            out, plan = s.download(), s.plan(a["tb"])
            hists = [s.cycle_hist()]
            plans = [{k: s.plan(k) for k in sorted(hists[0])}]
            slabs = [a["n"]]
            s.close()
        np.save(os.path.join(outdir, name + ".npy"), out)
        info[name] = {k: plan.get(k) for k in PLAN_KEYS}  # the plan of depth tb
        # per member (one, or the loopback group's slabs): the cycles that ran,
        # {depth: count}, and the plan of every depth among them
        info[name]["members"] = [{"rows": nr, "hist": {str(k): v for k, v in h.items()},
                                  "plans": {str(k): {key: pl.get(key) for key in PLAN_KEYS} for k, pl in ps.items()}}
                                 for nr, h, ps in zip(slabs, hists, plans)]
        print(name, "tb", a["tb"], "cycle_hist", hists, {k: info[name][k] for k in PLAN_KEYS}, flush=True)
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump(info, f)


if __name__ == "__main__":
    main(sys.argv[1])
