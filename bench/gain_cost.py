#!/usr/bin/env python3
"""Cost of a source gain schedule: the same grid timed with a rough schedule
(source_gain=) and with the source alone on the same build, interleaved (S G,
G S, ...), both dtypes, one JSON line.

    python bench/gain_cost.py [--n 32768] [--dtypes fp64,fp32] [--steps 48] [--reps 5] [--parent DIR]

Each timed run is one step(steps) after prepare(steps) and one warm-up
step(steps), between two host clock reads around a synchronised stream; the
schedule is rewound (set_source_gain(G), untimed) before every run, so each run
takes the same entries. The run with a schedule puts every launch on
tb_kernel_gain (tb_kernel_src plus K wave-uniform loads per wave; in "fma" the
add becomes an fma, in "exact" one more multiply per point and level) and adds
one one-thread launch per cycle; both sides use the depth prepare() picks under
the source kernels' clamp. The schedules are recorded.

--parent DIR: a checkout of the parent commit with its native build. Then the
Dirichlet 20-step headline (bench.py --gpus 1 --steps 20 --warmup 5, no source)
is run from DIR (A) and from this tree (B) in the order A B B A, each in a
process of its own, and both result lines are recorded under "headline".
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from source_cost import rough_source  # noqa: E402


def rough_gain(steps):
    import numpy as np
    g = 10.0 ** np.random.default_rng(7).uniform(-1.0, 0.5, steps)
    g[2::5] = 0.0
    g[4::7] = 1.0
    return g


def headline(tree):
    tree = os.path.abspath(tree)
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"],
                         cwd=tree, capture_output=True, text=True, timeout=900,
                         env={k: v for k, v in os.environ.items() if k not in ("HEAT2D_LIB", "PYTHONPATH")})
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    if out.returncode != 0 or not lines:
        raise RuntimeError(f"bench.py in {tree} failed ({out.returncode}): {out.stdout[-500:]}{out.stderr[-500:]}")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--dtypes", default="fp64,fp32")
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.25)
    ap.add_argument("--parent", default=None, metavar="DIR")
    a = ap.parse_args()
    rec = {"n": a.n, "steps": a.steps, "sigma": a.sigma, "reps": a.reps}
    if a.parent:  # before this process opens the GPU: one process at a time
        runs = [(tag, headline(a.parent if tag == "A" else ROOT)) for tag in "ABBA"]
        rec["headline"] = {"order": "ABBA", "runs": [{"tree": t, "result": r} for t, r in runs]}
    import numpy as np
    import torch

    import heat2d
    from heat2d.models.heat2d import HeatSolver
    torch.cuda.set_device(0)
    prob = heat2d.make_problem(heat2d.InputDat(n=a.n, sigma=a.sigma, nu=0.05, dom_len=1.0, ntime=a.steps), "ghost", "uniform")
    G = rough_gain(a.steps)
    for dtype in a.dtypes.split(","):
        S = rough_source(a.n, np.float64 if dtype == "fp64" else np.float32)
        solvers = {}
        for kind in ("source", "gain"):
            s = HeatSolver(prob, dtype=dtype, backend="hip", device=0, arith="auto", source=S,
                           source_gain=G if kind == "gain" else None)
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
                if kind == "gain":
                    s.set_source_gain(G)  # rewind, untimed (it drops this solver's captured graphs)
                s.prepare(a.steps)  # (both sides alike: graphs re-captured, the same warm state)
                s.synchronize()
                t0 = time.perf_counter()
                s.step(a.steps)
                s.synchronize()
                ms[kind].append((time.perf_counter() - t0) * 1e3)
        out = {"arith": solvers["gain"].info()["arith"], "depth_clamp": solvers["gain"].info()["source"]["max_tb"],
               "schedule": {k: solvers[k].schedule(a.steps) for k in kinds},
               "cycles": {k: {str(d): c for d, c in solvers[k].cycle_hist().items() if c} for k in kinds}}
        for k in kinds:
            med = statistics.median(ms[k])
            out[k] = {"ms": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                      "gpts_per_s": round(a.n * a.n * a.steps / med / 1e6, 1)}
        out["gain_over_source"] = round(out["gain"]["median_ms"] / out["source"]["median_ms"], 4)
        rec[dtype] = out
        for s in solvers.values():
            s.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
