"""Worker for tests/test_gpu_pipe.py.

`python tests/pipe_worker.py OUTDIR`: runs every case of CASES on the GPU in
this process — HEAT2D_PIPE (the wave-pair interior kernel: 1 forced, 0 off) is
read once per process, so the test starts one worker per value — and writes
OUTDIR/<case>.npy (the final owned field) and OUTDIR/info.json (per case: the
plan the cycle of depth tb ran).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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
    that make up `steps`, default one). Grids are square: the
    column cases set n around the wide strip's useful width U(tb), the row
    cases take the thinnest slab the split accepts (6 tb rows: an interior of
    4 tb) and cut it into bands of 2 tb rows (5 FIFO depths)."""
    c = {}
    u20 = useful(20)
    # columns, depth 20 (K1 = K2 = 10): one kind-2 strip holding both frame columns; U - 1, U, U + 1; 2 strips + a partial one
    for name, n in [("cols_lt_u", 150), ("cols_u_minus_1", u20 - 1), ("cols_u", u20), ("cols_u_plus_1", u20 + 1),
                    ("cols_2u_partial", 2 * u20 + 37)]:
        c[name] = dict(n=n, tb=20, steps=2 * 20 + 3, ic="rough")
    # rows: the thinnest interior the split accepts; short bands so the FIFO wraps several times per item
    c["rows_thinnest"] = dict(n=6 * 20, tb=20, steps=20, ic="rough")
    c["rows_short_bands"] = dict(n=8 * 20 + 1, tb=20, steps=2 * 20, ic="rough", env={"HEAT2D_BANDS": "3"})
    # more items than pairs: each pair runs several items back to back (static stride, dynamic queue)
    c["items_static"] = dict(n=2 * u20 + 37, tb=20, steps=20 + 5, ic="rough",
                             env={"HEAT2D_BANDS": "5", "HEAT2D_MAX_WAVES": "2"})
    c["items_dynamic"] = dict(n=2 * u20 + 37, tb=20, steps=20 + 5, ic="rough",
                              env={"HEAT2D_BANDS": "5", "HEAT2D_MAX_WAVES": "2", "HEAT2D_DYNAMIC": "1"})
    # segment plans whose pieces cross a strip end (static and dynamic)
    c["segments"] = dict(n=2 * u20 + 37, tb=20, steps=20 + 5, ic="rough", env={"HEAT2D_SEGMENTS": "7"})
    c["segments_dynamic"] = dict(n=2 * u20 + 37, tb=20, steps=20, ic="rough",
                                 env={"HEAT2D_SEGMENTS": "11", "HEAT2D_MAX_WAVES": "3", "HEAT2D_DYNAMIC": "1"})
    # depths: 16, 19 and 21 (K1 != K2), 24 — three strips, the middle one of
    # kind 0 (scaled levels, one unscale at the store: needs n >= 2 U + KA)
    for k in (16, 19, 21, 24):
        c[f"depth_{k}"] = dict(n=2 * useful(k) + 37, tb=k, steps=2 * k + 1, ic="rough", kind0=True)
    # ... and the deep ones with several items per pair: bands through the dynamic queue, segments across strip ends
    c["depth_24_items"] = dict(n=2 * useful(24) + 37, tb=24, steps=24 + 5, ic="rough", kind0=True,
                               env={"HEAT2D_BANDS": "4", "HEAT2D_MAX_WAVES": "2", "HEAT2D_DYNAMIC": "1"})
    c["depth_21_segments"] = dict(n=2 * useful(21) + 37, tb=21, steps=21 + 5, ic="rough", kind0=True,
                                  env={"HEAT2D_SEGMENTS": "7", "HEAT2D_MAX_WAVES": "3"})
    c["depth_19_items"] = dict(n=2 * useful(19) + 37, tb=19, steps=19, ic="rough", kind0=True,
                               env={"HEAT2D_BANDS": "4", "HEAT2D_MAX_WAVES": "2"})
    # the reference IC (smooth, values in [1, 2])
    c["reference_ic"] = dict(n=u20 + 1, tb=20, steps=2 * 20, ic="uniform")
    # the other arithmetic forms' instances, kind-0 strip included: at r = 1/4,
    # and the forms that take any r at sigma 0.2 (fast: scaled by 1 / r per level)
    for arith in ("exact", "fma", "fast"):
        c[f"arith_{arith}"] = dict(n=2 * u20 + 37, tb=20, steps=20 + 3, ic="rough", arith=arith, kind0=True)
    for arith, k in (("exact", 21), ("fma", 20), ("fast", 19)):
        c[f"arith_{arith}_r02"] = dict(n=2 * useful(k) + 37, tb=k, steps=k + 3, ic="rough", arith=arith, sigma=0.2,
                                       kind0=True)
    # every instance once (depths 16..24 x 4 forms): the cols_2u_partial shape of its depth (three
    # strips, the middle one of kind 0), 2 k + 3 steps: two full passes and a shallower one, as
    # three step() calls (`calls`: one step(2 k + 3) runs balanced cycles of depth ~2 k / 3, never
    # one of depth k). exact and fma at sigma 0.2; fast at r = 1/4 (bitwise the jacobi form) at
    # even depths, at sigma 0.2 (within its bound) at odd ones
    for k in range(16, 25):
        for arith in ("exact", "fma", "jacobi", "fast"):
            sigma = 0.25 if arith == "jacobi" or (arith == "fast" and k % 2 == 0) else 0.2
            c[f"inst_{arith}_{k}"] = dict(n=2 * useful(k) + 37, tb=k, steps=2 * k + 3, calls=[k, k, 3], ic="rough",
                                          arith=arith, sigma=sigma, kind0=True)
    # other paths: graph replay, loopback exchange between two slabs
    c["graph"] = dict(n=u20 + 1, tb=16, steps=3 * 16, ic="rough", kind="graph")
    c["loopback"] = dict(n=2 * useful(16) + 37, tb=16, steps=2 * 16 + 3, ic="rough", kind="loopback")
    return c


def problem(n, steps, sigma=0.25):
    import heat2d
    return heat2d.make_problem(heat2d.InputDat(n=n, sigma=sigma, nu=0.05, dom_len=1.0, ntime=steps), "ghost", "uniform")


def rough(n, seed=7):
    """Rough non-dyadic owned field, values 10**uniform(-1, 1)."""
    import numpy as np
    return 10.0 ** np.random.default_rng(seed).uniform(-1.0, 1.0, (n, n))


KNOBS = ("HEAT2D_BANDS", "HEAT2D_SEGMENTS", "HEAT2D_MAX_WAVES", "HEAT2D_DYNAMIC")


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
        assert p.n_owned == a["n"]
        arith = a.get("arith", "jacobi")
        kind = a.get("kind", "solver")
        if kind == "loopback":
            g = LoopbackGroup(p, 2, dtype="fp64", backend="hip", tb=a["tb"], device=0, arith=arith, autotune=0)
            if a["ic"] == "rough":
                g.upload(rough(a["n"]))
            g.step(p.ntime)
            out, plan = g.download(), g.plan(0, a["tb"])
            g.close()
        else:
            s = HeatSolver(p, dtype="fp64", backend="hip", tb=a["tb"], device=0, arith=arith, autotune=0,
                           graph=(kind == "graph"))
            if a["ic"] == "rough":
                s.upload(rough(a["n"]))
            for m in a.get("calls", [p.ntime]):
                s.step(m)
            out, plan = s.download(), s.plan(a["tb"])
            depths = sorted(s.cycle_hist())
            s.close()
        np.save(os.path.join(outdir, name + ".npy"), out)
        info[name] = {k: plan.get(k) for k in ("pipe", "valid", "dynamic", "main_bands", "main_items", "main_waves",
                                                "main_rect", "main_strip_w", "main_useful_w")}
        info[name]["depths"] = None if kind == "loopback" else depths  # the cycle depths that ran
        print(name, info[name], flush=True)
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump(info, f)


if __name__ == "__main__":
    main(sys.argv[1])
