#!/usr/bin/env python3
"""Cost of probe points: the same grid timed with P probes spread over it and
with none on the same build, interleaved (N P, P N, ...), one JSON line.

    python bench/probes_cost.py [--n 32768] [--dtype fp64] [--steps 20] [--probes 1024] [--reps 5]

Each timed run is one step(steps) after prepare(steps) and one warm-up
step(steps), between two host clock reads around a synchronised stream. The run
with probes adds, per cycle, one probe_cone launch of P workgroups and a
one-thread launch ahead of the cycle's boundary-band launch; the stencil
launches are the same. The cone's own time (the kernel alone, P points at the
deepest depth of the schedule, device events around 10 launches) is recorded
beside it, and so are the phase timers of one more step(steps) of each solver:
the band launch's timer brackets the cone, so its difference is the cone's time
on the GPU timeline.
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(n, count):
    """`count` owned points on a jittered square lattice over the n x n grid (frame-inclusive indices)."""
    import numpy as np
    side = int(np.ceil(np.sqrt(count)))
    rng = np.random.default_rng(2003)
    cell = n / side
    ij = [(int(a * cell + rng.uniform(0, cell)), int(b * cell + rng.uniform(0, cell))) for a in range(side) for b in range(side)]
    return np.clip(np.array(ij[:count], dtype=np.int64) + 1, 1, n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--dtype", default="fp64")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--probes", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=0.25)
    a = ap.parse_args()
    import torch

    import heat2d
    from heat2d.models.heat2d import HeatSolver
    from heat2d.ops import kernels as K
    torch.cuda.set_device(0)
    prob = heat2d.make_problem(heat2d.InputDat(n=a.n, sigma=a.sigma, nu=0.05, dom_len=1.0, ntime=a.steps), "ghost", "uniform")
    pts = spread(a.n, a.probes)
    solvers = {}
    for kind in ("none", "probes"):
        s = HeatSolver(prob, dtype=a.dtype, backend="hip", device=0, probes=pts if kind == "probes" else None,
                       probe_steps=a.steps)
        s.prepare(a.steps)
        s.step(a.steps)  # warm-up
        s.synchronize()
        solvers[kind] = s
    kinds = list(solvers)
    ms = {k: [] for k in kinds}
    for rep in range(a.reps):
        for kind in (kinds if rep % 2 == 0 else kinds[::-1]):
            s = solvers[kind]
            s.clear_probe_history()  # (synchronises; outside the clock)
            s.synchronize()
            t0 = time.perf_counter()
            s.step(a.steps)
            s.synchronize()
            ms[kind].append((time.perf_counter() - t0) * 1e3)
    sp = solvers["probes"]
    rec = {"n": a.n, "dtype": a.dtype, "steps": a.steps, "sigma": a.sigma, "reps": a.reps, "nprobes": a.probes,
           "recorded": sp.info()["probes"]["recorded"], "arith": sp.info()["arith"],
           "schedule": {k: solvers[k].schedule(a.steps) or solvers[k].step_cycles(a.steps) for k in kinds}}
    # the last recorded row against the field itself, at every 16th probe (one small region download each)
    import ctypes as C

    import numpy as np

    from heat2d.ops import _native as N
    H = sp.probe_history()
    one = np.empty((1, 1), dtype=H.dtype)
    same = True
    for p in range(0, len(pts), 16):
        i, j = int(pts[p, 0]) - 1, int(pts[p, 1]) - 1
        N.call("heat2d_solver_download_region", sp._h, i, i + 1, j, j + 1, one.ctypes.data_as(C.c_void_p), 1)
        same = same and one[0, 0] == H[-1, p]
    rec["last_row_is_the_field"] = bool(same)
    for k in kinds:
        med = statistics.median(ms[k])
        rec[k] = {"ms": [round(v, 4) for v in ms[k]], "median_ms": round(med, 4),
                  "gpts_per_s": round(a.n * a.n * a.steps / med / 1e6, 1)}
    rec["probes_over_none"] = round(rec["probes"]["median_ms"] / rec["none"]["median_ms"], 4)
    # the band launch's phase timer (device events around it) brackets the cone and the advance too:
    # its difference between the two solvers is the cone's own time on the GPU timeline
    for k in kinds:
        s = solvers[k]
        s.clear_probe_history()
        s.set_timing(True)
        s.step(a.steps)
        ph = s.phase_times()
        s.set_timing(False)
        rec[k]["phase_ms"] = {q: round(ph[q], 4) for q in ("main_ms", "edge_ms", "cycle_ms")}
        rec[k]["cycles"] = ph["cycles"]
    for s in solvers.values():
        s.close()
    # the cone alone: P points of a 1024-row slab of the same width, the schedule's deepest depth
    depth = max(rec["schedule"]["probes"])
    L = K.make_layout(1024, a.n, halo=24)
    tdt = torch.float64 if a.dtype == "fp64" else torch.float32
    src = torch.rand(L.elems(), dtype=tdt, device="cuda")
    small = pts.copy()
    small[:, 0] = (small[:, 0] - 1) % 1024 + 1
    arith = ("exact", "fma", "jacobi")[rec["arith"]]
    K.probe_cone(src, L, depth, prob.r, small, arith=arith)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10):
        K.probe_cone(src, L, depth, prob.r, small, arith=arith)
    e1.record()
    e1.synchronize()
    rec["cone_alone"] = {"depth": depth, "ms_per_launch_incl_host": round(e0.elapsed_time(e1) / 10, 4)}
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
