#!/usr/bin/env python3
"""Cost of insulated boundaries: the same grid timed fully insulated and with
the Dirichlet frame on the same build, interleaved (D I I D ...), one JSON line.

    python bench/insulated_cost.py [--n 32768] [--dtype fp64] [--steps 20] [--reps 5] [--only insulated|dirichlet]

Each timed run is one step(steps) after prepare(steps) and one warm-up
step(steps), between two host clock reads around a synchronised stream. The
insulated run swaps the interior kernel's frame-column strips for items of the
insulated-edge kernel and refreshes the frame images behind every launch.
--only times one setting alone (for a kernel trace of its own).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--dtype", default="fp64", choices=["fp32", "fp64"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.25)
    ap.add_argument("--arith", default="auto")
    ap.add_argument("--only", default=None, choices=["insulated", "dirichlet"])
    a = ap.parse_args()
    import torch

    import heat2d
    from heat2d.models.heat2d import HeatSolver
    torch.cuda.set_device(0)
    prob = heat2d.make_problem(heat2d.InputDat(n=a.n, sigma=a.sigma, nu=0.05, dom_len=1.0, ntime=a.steps), "ghost", "uniform")
    arith = "jacobi" if a.arith == "auto" and prob.r == 0.25 else a.arith
    kinds = [a.only] if a.only else ["dirichlet", "insulated"]
    solvers = {}
    for kind in kinds:
        s = HeatSolver(prob, dtype=a.dtype, backend="hip", device=0, arith=arith, bc_x=kind, bc_y=kind)
        s.prepare(a.steps)
        s.step(a.steps)  # warm-up
        s.synchronize()
        solvers[kind] = s
    ms = {k: [] for k in kinds}
    for rep in range(a.reps):
        for kind in (kinds if rep % 2 == 0 else kinds[::-1]):  # D I, I D, D I ...
            s = solvers[kind]
            s.synchronize()
            t0 = time.perf_counter()
            s.step(a.steps)
            s.synchronize()
            ms[kind].append((time.perf_counter() - t0) * 1e3)
    rec = {"n": a.n, "dtype": a.dtype, "steps": a.steps, "arith": arith, "reps": a.reps,
           "schedule": {k: solvers[k].schedule(a.steps) for k in kinds}}
    for k in kinds:
        med = statistics.median(ms[k])
        rec[k] = {"ms": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                  "gpts_per_s": round(a.n * a.n * a.steps / med / 1e6, 1)}
    if len(kinds) == 2:
        rec["insulated_over_dirichlet"] = round(rec["insulated"]["median_ms"] / rec["dirichlet"]["median_ms"], 4)
    print(json.dumps(rec), flush=True)
    for s in solvers.values():
        s.close()


if __name__ == "__main__":
    main()
