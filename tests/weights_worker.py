"""Data and helpers of the five-weight tests (tests/test_weights*.py): plain
functions, no test in here."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from source_worker import problem, rough_field  # noqa: E402,F401

NP = {"fp64": np.float64, "fp32": np.float32}
# rough weights (wS, wE, wN, wW, wC): all different, no power of two, sum 0.97
ROUGH = (0.11, 0.07, 0.23, 0.19, 0.37)
BCS = [("dirichlet", "dirichlet"), ("periodic", "dirichlet"), ("dirichlet", "periodic"), ("periodic", "periodic")]
BC_IDS = ["dd", "pd", "dp", "pp"]


def signed_field(n, dtype, seed=0):
    """source_worker.rough_field (10**uniform(-1, 1), frame included) with random signs: rough, signed, no zero."""
    T = rough_field(n, dtype, seed)
    sign = np.random.default_rng(7000 + seed).choice([-1.0, 1.0], T.shape).astype(T.dtype)
    return T * sign


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def signed_rect(n, rows, dtype, seed=0):
    """signed_field for a rows x n domain."""
    T = rough_field(n, dtype, seed, rows=rows)
    return T * np.random.default_rng(7000 + seed).choice([-1.0, 1.0], T.shape).astype(T.dtype)


def main(argv):
    """`python tests/weights_worker.py OUTDIR JSON_ARGS`: a one-rank run with weights on the GPU in a fresh
    process (HEAT2D_SPLIT_ORDER, HEAT2D_BANDS, HEAT2D_PIPE, HEAT2D_DYNAMIC and HEAT2D_MAX_WAVES are read once
    per process); writes OUTDIR/result.npy (the owned points) and OUTDIR/info.json. JSON_ARGS: n, steps, tb,
    dtype, arith, and optionally rows (a rows x n domain), graph, bc_x, bc_y, calls (the step() calls)."""
    import json

    import torch

    from heat2d.models.heat2d import HeatSolver
    outdir, a = argv[0], json.loads(argv[1])
    torch.cuda.set_device(0)
    rows = a.get("rows")
    s = HeatSolver(problem(a["n"], a["steps"]), dtype=a["dtype"], backend="hip", tb=a["tb"], arith=a["arith"], device=0,
                   rows=rows, graph=bool(a.get("graph")), bc_x=a.get("bc_x", "dirichlet"), bc_y=a.get("bc_y", "dirichlet"),
                   weights=ROUGH)
    s.upload(signed_rect(a["n"], rows, a["dtype"]) if rows else signed_field(a["n"], a["dtype"]))
    sizes = a.get("calls", [a["steps"]])
    assert sum(sizes) == a["steps"]
    first_cycles = s.step_cycles(sizes[0])
    for m in sizes:
        s.prepare(m)
        s.step(m)
    np.save(os.path.join(outdir, "result.npy"), s.download())
    info = s.info()
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump({"plan": s.plan(a["tb"]), "info": {k: info[k] for k in ("tb", "arith", "bc_x", "bc_y", "weights")},
                   "cycle_hist": {str(k): v for k, v in s.cycle_hist().items()}, "first_call_cycles": first_cycles}, f)
    s.close()


if __name__ == "__main__":
    main(sys.argv[1:])
