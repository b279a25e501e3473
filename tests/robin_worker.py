"""Worker for tests/test_robin.py.

`python tests/robin_worker.py OUTDIR JSON_ARGS`: a one-rank run with Robin walls on
the GPU in a fresh process (HEAT2D_SPLIT_ORDER, HEAT2D_BANDS, HEAT2D_PIPE,
HEAT2D_DYNAMIC and HEAT2D_MAX_WAVES are read once per process); writes
OUTDIR/result.npy (the owned points) and OUTDIR/info.json (the plan of depth tb,
info()'s tb / arith / bc / robin, cycle_hist() and the cycle depths of the first step() call).
JSON_ARGS: n, steps, tb, dtype, arith, bc_x, bc_y, and optionally rows (a
rows x n domain), graph, sigma, calls (the step() calls that make up the steps).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from source_worker import problem, rough_field  # noqa: E402,F401

PAIRS = {"x_lo": (0.8125, 0.37), "x_hi": (0.6, -0.21), "y_lo": (0.93, 0.055), "y_hi": (-0.45, 1.3)}


def pairs_for(bc_x, bc_y, pairs=PAIRS):
    """The pairs of exactly the Robin sides of (bc_x, bc_y)."""
    return {k: v for k, v in pairs.items() if (bc_x if k[0] == "x" else bc_y) == "robin"}


def main(argv):
    outdir, a = argv[0], json.loads(argv[1])
    import numpy as np
    import torch

    from heat2d.models.heat2d import HeatSolver
    torch.cuda.set_device(0)
    rows = a.get("rows")
    p = problem(a["n"], a["steps"], a.get("sigma", 0.2371))
    s = HeatSolver(p, dtype=a["dtype"], backend="hip", tb=a["tb"], arith=a["arith"], device=0, rows=rows,
                   graph=bool(a.get("graph")), bc_x=a["bc_x"], bc_y=a["bc_y"], robin=pairs_for(a["bc_x"], a["bc_y"]))
    s.upload(rough_field(a["n"], a["dtype"], rows=rows))
    sizes = a.get("calls", [a["steps"]])
    assert sum(sizes) == a["steps"]
    first_cycles = s.step_cycles(sizes[0])  # the cycle depths the first call will run (graph pairs: depth tb, twice)
    for m in sizes:
        s.prepare(m)
        s.step(m)
    np.save(os.path.join(outdir, "result.npy"), s.download())
    info = s.info()
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump({"plan": s.plan(a["tb"]), "info": {k: info[k] for k in ("tb", "arith", "bc_x", "bc_y", "robin")},
                   "cycle_hist": {str(k): v for k, v in s.cycle_hist().items()},
                   "first_call_cycles": first_cycles}, f)
    s.close()


if __name__ == "__main__":
    main(sys.argv[1:])
