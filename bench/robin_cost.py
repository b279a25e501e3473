#!/usr/bin/env python3
"""Cost of Robin walls: the same grid timed fully Robin (four different pairs),
fully insulated and with the Dirichlet frame on the same build, interleaved
(D I R, R I D, ...), one JSON line.

    python bench/robin_cost.py [--n 32768] [--dtype fp64] [--steps 20] [--reps 5] [--only robin|insulated|dirichlet]

Each timed run is one step(steps) after prepare(steps) and one warm-up
step(steps), between two host clock reads around a synchronised stream. All
three run the same arithmetic form (default fma: Robin walls have no jacobi
form). Robin against insulated is the number of interest: the two have the same
launch structure (the interior kernel's wall-column strips become items of
tb_kernel_rob / tb_kernel_ins, the frame entries are refreshed behind every
launch); the Robin kernel forms a * C + b where the insulated one takes C.
--only times one setting alone (for a kernel trace of its own).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIRS = {"x_lo": (0.8125, 0.37), "x_hi": (0.6, -0.21), "y_lo": (0.93, 0.055), "y_hi": (-0.45, 1.3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--dtype", default="fp64", choices=["fp32", "fp64"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.25)
    ap.add_argument("--arith", default="fma", choices=["fma", "exact"])
    ap.add_argument("--only", default=None, choices=["robin", "insulated", "dirichlet"])
    a = ap.parse_args()
    import torch

    import heat2d
    from heat2d.models.heat2d import HeatSolver
    torch.cuda.set_device(0)
    prob = heat2d.make_problem(heat2d.InputDat(n=a.n, sigma=a.sigma, nu=0.05, dom_len=1.0, ntime=a.steps), "ghost", "uniform")
    kinds = [a.only] if a.only else ["dirichlet", "insulated", "robin"]
    solvers = {}
    for kind in kinds:
        s = HeatSolver(prob, dtype=a.dtype, backend="hip", device=0, arith=a.arith, bc_x=kind, bc_y=kind,
                       robin=PAIRS if kind == "robin" else None)
        s.prepare(a.steps)
        s.step(a.steps)  # warm-up
        s.synchronize()
        solvers[kind] = s
    ms = {k: [] for k in kinds}
    for rep in range(a.reps):
        for kind in (kinds if rep % 2 == 0 else kinds[::-1]):  # D I R, R I D, ...
            s = solvers[kind]
            s.synchronize()
            t0 = time.perf_counter()
            s.step(a.steps)
            s.synchronize()
            ms[kind].append((time.perf_counter() - t0) * 1e3)
    rec = {"n": a.n, "dtype": a.dtype, "steps": a.steps, "arith": a.arith, "reps": a.reps,
           "schedule": {k: solvers[k].schedule(a.steps) for k in kinds}}
    for k in kinds:
        med = statistics.median(ms[k])
        rec[k] = {"ms": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                  "gpts_per_s": round(a.n * a.n * a.steps / med / 1e6, 1)}
    if len(kinds) == 3:
        rec["robin_over_insulated"] = round(rec["robin"]["median_ms"] / rec["insulated"]["median_ms"], 4)
        rec["robin_over_dirichlet"] = round(rec["robin"]["median_ms"] / rec["dirichlet"]["median_ms"], 4)
        rec["insulated_over_dirichlet"] = round(rec["insulated"]["median_ms"] / rec["dirichlet"]["median_ms"], 4)
    print(json.dumps(rec), flush=True)
    for s in solvers.values():
        s.close()


if __name__ == "__main__":
    main()
