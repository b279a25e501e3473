#!/usr/bin/env python3
"""Cost of the five-weight operator: the same grid timed with rough weights (fma)
and with the scalar r (fma) on the same build, interleaved (S W, W S, ...), and
the weights' exact form once; one JSON line.

    python bench/weights_cost.py [--n 32768] [--dtype fp64] [--steps 20] [--reps 5]

Each timed run is one step(steps) after prepare(steps) and one warm-up
step(steps), between two host clock reads around a synchronised stream. The
weights run every rect of every launch on the general five-weight kernel
(tb_kernel_w5: all four edge kinds, no priming skip), the scalar-r run its
interior on the interior kernel: the ratio is the price of that, and the figure
an interior variant of the five-weight kernel would be judged by.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROUGH = (0.11, 0.07, 0.23, 0.19, 0.37)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--dtype", default="fp64", choices=["fp32", "fp64"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.2)
    a = ap.parse_args()
    import torch

    import heat2d
    from heat2d.models.heat2d import HeatSolver
    torch.cuda.set_device(0)
    prob = heat2d.make_problem(heat2d.InputDat(n=a.n, sigma=a.sigma, nu=0.05, dom_len=1.0, ntime=a.steps), "ghost", "uniform")

    def make(arith, weights):
        s = HeatSolver(prob, dtype=a.dtype, backend="hip", device=0, arith=arith, weights=weights)
        s.prepare(a.steps)
        s.step(a.steps)  # warm-up
        s.synchronize()
        return s

    def timed(s):
        s.synchronize()
        t0 = time.perf_counter()
        s.step(a.steps)
        s.synchronize()
        return (time.perf_counter() - t0) * 1e3

    kinds = ["scalar", "weights"]
    solvers = {"scalar": make("fma", None), "weights": make("fma", ROUGH)}
    ms = {k: [] for k in kinds}
    for rep in range(a.reps):
        for kind in (kinds if rep % 2 == 0 else kinds[::-1]):  # S W, W S, ...
            ms[kind].append(timed(solvers[kind]))
    rec = {"n": a.n, "dtype": a.dtype, "steps": a.steps, "reps": a.reps, "weights": ROUGH,
           "schedule": {k: solvers[k].schedule(a.steps) for k in kinds},
           "cycles": {k: solvers[k].step_cycles(a.steps) for k in kinds}}
    for k in kinds:
        med = statistics.median(ms[k])
        rec[k] = {"arith": "fma", "ms": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                  "gpts_per_s": round(a.n * a.n * a.steps / med / 1e6, 1)}
    solvers.pop("scalar").close()
    ex = make("exact", ROUGH)
    t = timed(ex)
    ex.close()
    rec["weights_exact"] = {"arith": "exact", "ms": [round(t, 4)], "gpts_per_s": round(a.n * a.n * a.steps / t / 1e6, 1)}
    rec["weights_over_scalar"] = round(rec["weights"]["median_ms"] / rec["scalar"]["median_ms"], 4)
    rec["exact_over_fma"] = round(t / rec["weights"]["median_ms"], 4)
    print(json.dumps(rec), flush=True)
    solvers["weights"].close()


if __name__ == "__main__":
    main()
