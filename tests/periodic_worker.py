"""Worker for tests/test_periodic.py.

`python tests/periodic_worker.py gloo RANK WORLD PORT OUTDIR JSON_ARGS`: one
rank of a periodic run on the CPU twin over torch.distributed (gloo, the
callback transport); rank 0 gathers the field into OUTDIR/result.npy.

`python tests/periodic_worker.py single OUTDIR JSON_ARGS`: a one-rank run on
the GPU in a fresh process (HEAT2D_SPLIT_ORDER and HEAT2D_PIPE are read once
per process); writes OUTDIR/result.npy and OUTDIR/info.json (the plan of depth
tb, cycle_hist() and the plan of every depth that ran). JSON_ARGS may hold
"calls", the step() calls that make up the steps, and may be a list of runs.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(n, steps, sigma=0.2371):
    import heat2d
    return heat2d.make_problem(heat2d.InputDat(n=n, sigma=sigma, nu=0.05, dom_len=1.0, ntime=steps), "ghost", "uniform")


def rough_field(n, dtype, seed=0, lo=-1.0, hi=1.0):
    """Frame-inclusive (n + 2)^2 field of rough values 10**uniform(lo, hi), frame included."""
    import numpy as np
    dt = np.float64 if dtype == "fp64" else np.float32
    return (10.0 ** np.random.default_rng(seed).uniform(lo, hi, (n + 2, n + 2))).astype(dt)


def gloo(argv):
    rank, world, port, outdir = int(argv[0]), int(argv[1]), int(argv[2]), argv[3]
    a = json.loads(argv[4])
    from datetime import timedelta

    import numpy as np
    import torch.distributed as dist

    from heat2d.models.heat2d import HeatSolver
    from heat2d.parallel.transport import TorchDistTransport
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            timeout=timedelta(seconds=float(os.environ.get("HEAT2D_COMM_TIMEOUT", "600"))))
    p = problem(a["n"], a["steps"])
    s = HeatSolver(p, dtype=a["dtype"], backend="cpu", tb=a["tb"], arith="exact", transport=TorchDistTransport(),
                   bc_x=a["bc_x"], bc_y=a["bc_y"])
    T0 = rough_field(a["n"], a["dtype"])
    s.upload(T0[s.row0:s.row0 + s.nrows + 2])  # this rank's rows with their frame
    s.step(a["steps"])
    full = s.gather()
    if rank == 0:
        np.save(os.path.join(outdir, "result.npy"), full)
    s.close()
    dist.barrier()
    dist.destroy_process_group()


def single(argv):
    outdir, a = argv[0], json.loads(argv[1])
    import torch
    torch.cuda.set_device(0)
    if isinstance(a, list):  # several runs in this one process: result_<i>.npy, info.json a list
        infos = [single_run(outdir, x, f"result_{i}.npy") for i, x in enumerate(a)]
    else:
        infos = single_run(outdir, a, "result.npy")
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump(infos, f)


def single_run(outdir, a, result):
    """One run: the steps as one step(steps) call, or as the step() calls of
    a["calls"] (tests/cycles.py calls(): cycles of depth tb). Returns the plan
    of depth tb, cycle_hist() and the plan of every depth that ran."""
    import numpy as np

    from heat2d.models.heat2d import HeatSolver
    p = problem(a["n"], a["steps"])
    s = HeatSolver(p, dtype=a["dtype"], backend="hip", tb=a["tb"], arith="exact", device=0, bc_x=a["bc_x"],
                   bc_y=a["bc_y"])
    s.upload(rough_field(a["n"], a["dtype"]))
    sizes = a.get("calls", [a["steps"]])
    assert sum(sizes) == a["steps"]
    for m in sizes:
        s.prepare(m)
        s.step(m)
    np.save(os.path.join(outdir, result), s.download())
    hist = s.cycle_hist()
    info = {"plan": s.plan(a["tb"]), "transport": s.info()["transport"], "cycle_hist": {str(k): v for k, v in hist.items()},
            "plans": {str(k): s.plan(k) for k in sorted(hist)}}
    s.close()
    print(a, "cycle_hist", hist, flush=True)
    return info


if __name__ == "__main__":
    {"gloo": gloo, "single": single}[sys.argv[1]](sys.argv[2:])
