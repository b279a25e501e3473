#!/usr/bin/env python3
"""Cost of a heat source: the same grid timed with a rough source and without
one on the same build, interleaved (N S, S N, ...), both dtypes, one JSON line.

    python bench/source_cost.py [--n 32768] [--dtypes fp64,fp32] [--steps 48] [--reps 5]

Each timed run is one step(steps) after prepare(steps) and one warm-up
step(steps), between two host clock reads around a synchronised stream. The
run with a source puts every launch on the source kernel (tb_kernel_src: one
more 16-B load per lane and march row, one LDS read and one add per point and
level) at the depth prepare() picks under the source kernels' clamp; the run
without one is the solver's own best schedule. The schedules are recorded.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rough_source(n, np_dtype, tile=2048):
    """Frame-inclusive source of both signs, magnitudes 1e-3 .. 1e-1: one random tile repeated."""
    import numpy as np
    rng = np.random.default_rng(1)
    t = (10.0 ** rng.uniform(-3.0, -1.0, (tile, tile)) * rng.choice([-1.0, 1.0], (tile, tile))).astype(np_dtype)
    reps = (n + 2 + tile - 1) // tile
    return np.ascontiguousarray(np.tile(t, (reps, reps))[:n + 2, :n + 2])


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
        S = rough_source(a.n, np.float64 if dtype == "fp64" else np.float32)
        solvers = {}
        for kind in ("none", "source"):
            # the same arithmetic form on both sides: auto with a source (fma at r = 1/4, exact else)
            s = HeatSolver(prob, dtype=dtype, backend="hip", device=0, arith="auto", source=S if kind == "source" else None)
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
        out = {"arith": solvers["source"].info()["arith"], "depth_clamp": solvers["source"].info()["source"]["max_tb"],
               "schedule": {k: solvers[k].schedule(a.steps) for k in kinds}}
        for k in kinds:
            med = statistics.median(ms[k])
            out[k] = {"ms": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                      "gpts_per_s": round(a.n * a.n * a.steps / med / 1e6, 1)}
        out["source_over_none"] = round(out["source"]["median_ms"] / out["none"]["median_ms"], 4)
        rec[dtype] = out
        for s in solvers.values():
            s.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
