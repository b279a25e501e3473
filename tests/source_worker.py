"""Data and worker for tests/test_source.py.

`python tests/source_worker.py OUTDIR JSON_ARGS`: a one-rank run with a heat
source on the GPU in a fresh process (HEAT2D_SPLIT_ORDER, HEAT2D_DYNAMIC,
HEAT2D_MAX_WAVES and HEAT2D_PIPE are read once per process); writes
OUTDIR/result.npy and OUTDIR/info.json.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(n, steps, sigma=0.2):
    import heat2d
    return heat2d.make_problem(heat2d.InputDat(n=n, sigma=sigma, nu=0.05, dom_len=1.0, ntime=steps), "ghost", "uniform")


def rough_field(n, dtype, seed=0, rows=None):
    """Frame-inclusive field of rough values 10**uniform(-1, 1) (two decades), frame included:
    (n + 2)^2, or (rows + 2) x (n + 2)."""
    import numpy as np
    dt = np.float64 if dtype == "fp64" else np.float32
    shape = ((n if rows is None else rows) + 2, n + 2)
    return (10.0 ** np.random.default_rng(seed).uniform(-1.0, 1.0, shape)).astype(dt)


def rough_source(n, dtype, seed=1, rows=None):
    """Frame-inclusive source: both signs, magnitudes 10**uniform(-3, -1) of the field value at
    the point (nonzero frame entries too: the engine must ignore them)."""
    import numpy as np
    dt = np.float64 if dtype == "fp64" else np.float32
    T = rough_field(n, "fp64", rows=rows)
    rng = np.random.default_rng(1000 + seed)
    return (T * 10.0 ** rng.uniform(-3.0, -1.0, T.shape) * rng.choice([-1.0, 1.0], T.shape)).astype(dt)


def main(argv):
    outdir, a = argv[0], json.loads(argv[1])
    import numpy as np
    import torch

    from heat2d.models.heat2d import HeatSolver
    torch.cuda.set_device(0)
    rows = a.get("rows")
    p = problem(a["n"], a["steps"], a["sigma"])
    s = HeatSolver(p, dtype=a["dtype"], backend="hip", tb=a["tb"], arith=a["arith"], device=0, rows=rows,
                   source=rough_source(a["n"], a["dtype"], rows=rows))
    s.upload(rough_field(a["n"], a["dtype"], rows=rows))
    sizes = a.get("calls", [a["steps"]])  # the step() calls that make up the steps (tests/cycles.py calls())
    assert sum(sizes) == a["steps"]
    for m in sizes:
        s.prepare(m)
        s.step(m)
    np.save(os.path.join(outdir, "result.npy"), s.download())
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump({"plan": s.plan(a["tb"]), "info": {k: v for k, v in s.info().items() if k in ("tb", "arith", "source")},
                   "cycle_hist": {str(k): v for k, v in s.cycle_hist().items()}}, f)
    s.close()


if __name__ == "__main__":
    main(sys.argv[1:])
