#!/usr/bin/env python3
"""Cost of the conservative form div(k grad u): the same grid timed with rough
face coefficients and with the scalar r on the same build, interleaved (N F, F N,
...), both dtypes, one JSON line.

    python bench/faces_cost.py [--n 32768] [--dtypes fp64,fp32] [--steps 48] [--reps 5]

Each timed run is one step(steps) after prepare(steps) and one warm-up
step(steps), between two host clock reads around a synchronised stream. The
run with faces puts every launch on tb_kernel_div (two more 16-B loads per lane
and march row, two LDS reads per lane and level, 11 (exact) floating-point
operations per point and level where the scalar form has 6) at the depth
prepare() picks under the kernels' clamp; the run without is the solver's own
best schedule. The schedules are recorded.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rough_faces(n, np_dtype, tile=2048):
    """Two frame-inclusive arrays of face diffusion numbers uniform(0.0025, 0.25), 3 % of them 0:
    one random tile each, repeated."""
    import numpy as np
    rng = np.random.default_rng(2002)
    reps = (n + 2 + tile - 1) // tile
    out = []
    for _ in range(2):
        t = rng.uniform(0.0025, 0.25, (tile, tile))
        t[rng.uniform(size=(tile, tile)) < 0.03] = 0.0
        out.append(np.ascontiguousarray(np.tile(t.astype(np_dtype), (reps, reps))[:n + 2, :n + 2]))
    return tuple(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--dtypes", default="fp64,fp32")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.25)
    a = ap.parse_args()
    import numpy as np
    import torch

    import heat2d
    from heat2d.models.heat2d import HeatSolver
    torch.cuda.set_device(0)
    prob = heat2d.make_problem(heat2d.InputDat(n=a.n, sigma=a.sigma, nu=0.05, dom_len=1.0, ntime=a.steps), "ghost", "uniform")
    rec = {"n": a.n, "steps": a.steps, "sigma": a.sigma, "reps": a.reps}
    for dtype in a.dtypes.split(","):
        S = rough_faces(a.n, np.float64 if dtype == "fp64" else np.float32)
        solvers = {}
        for kind in ("none", "faces"):
            # the same arithmetic form on both sides: exact, what auto is with faces
            s = HeatSolver(prob, dtype=dtype, backend="hip", device=0, arith="exact", faces=S if kind == "faces" else None)
            s.prepare(a.steps)
            s.step(a.steps)  # warm-up
            s.synchronize()
            solvers[kind] = s
        del S
        kinds = list(solvers)
        ms = {k: [] for k in kinds}
        for rep in range(a.reps):
            for kind in (kinds if rep % 2 == 0 else kinds[::-1]):
                s = solvers[kind]
                s.synchronize()
                t0 = time.perf_counter()
                s.step(a.steps)
                s.synchronize()
                ms[kind].append((time.perf_counter() - t0) * 1e3)
        out = {"arith": solvers["faces"].info()["arith"], "depth_clamp": solvers["faces"].info()["faces"]["max_tb"],
               "schedule": {k: solvers[k].schedule(a.steps) for k in kinds}}
        for k in kinds:
            med = statistics.median(ms[k])
            out[k] = {"ms": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                      "gpts_per_s": round(a.n * a.n * a.steps / med / 1e6, 1)}
        out["faces_over_none"] = round(out["faces"]["median_ms"] / out["none"]["median_ms"], 4)
        rec[dtype] = out
        for s in solvers.values():
            s.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
