"""Data and worker for tests/test_rmap.py.

`python tests/rmap_worker.py OUTDIR JSON_ARGS`: a one-rank run with a
diffusivity map on the GPU in a fresh process (HEAT2D_SPLIT_ORDER,
HEAT2D_DYNAMIC, HEAT2D_MAX_WAVES and HEAT2D_PIPE are read once per process);
writes OUTDIR/result.npy and OUTDIR/info.json.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from source_worker import problem, rough_field  # noqa: E402,F401


def rough_map(n, dtype, seed=1, rows=None):
    """Frame-inclusive map of diffusion numbers uniform(0.01, 0.25), exactly 0 at the owned points
    where a second uniform draw is < 0.03 (embedded fixed points). The frame entries are nonzero:
    the engine must ignore them. No -0.0."""
    import numpy as np
    dt = np.float64 if dtype == "fp64" else np.float32
    shape = ((n if rows is None else rows) + 2, n + 2)
    rng = np.random.default_rng(2000 + seed)
    R = rng.uniform(0.01, 0.25, shape)
    hold = rng.uniform(size=shape) < 0.03
    R[1:-1, 1:-1][hold[1:-1, 1:-1]] = 0.0
    return R.astype(dt)


def main(argv):
    outdir, a = argv[0], json.loads(argv[1])
    import numpy as np
    import torch

    from heat2d.models.heat2d import HeatSolver
    torch.cuda.set_device(0)
    rows = a.get("rows")
    p = problem(a["n"], a["steps"], a["sigma"])
    s = HeatSolver(p, dtype=a["dtype"], backend="hip", tb=a["tb"], arith=a["arith"], device=0, rows=rows,
                   rmap=rough_map(a["n"], a["dtype"], rows=rows))
    s.upload(rough_field(a["n"], a["dtype"], rows=rows))
    sizes = a.get("calls", [a["steps"]])  # the step() calls that make up the steps (tests/cycles.py calls())
    assert sum(sizes) == a["steps"]
    for m in sizes:
        s.prepare(m)
        s.step(m)
    np.save(os.path.join(outdir, "result.npy"), s.download())
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump({"plan": s.plan(a["tb"]), "info": {k: v for k, v in s.info().items() if k in ("tb", "arith", "rmap")},
                   "cycle_hist": {str(k): v for k, v in s.cycle_hist().items()}}, f)
    s.close()


if __name__ == "__main__":
    main(sys.argv[1:])
