"""Data and worker for tests/test_faces.py and tests/test_faces_instances.py.

`python tests/faces_worker.py OUTDIR JSON_ARGS`: a one-rank run of the
conservative form (faces=) on the GPU in a fresh process (HEAT2D_SPLIT_ORDER,
HEAT2D_BANDS, HEAT2D_DYNAMIC and HEAT2D_MAX_WAVES are read once per process);
writes OUTDIR/result.npy and OUTDIR/info.json.

`python tests/faces_worker.py gloo RANK WORLD PORT OUTDIR JSON_ARGS`: one rank of
a run on the CPU twin over torch.distributed (gloo); rank 0 writes the gathered
field to OUTDIR/result.npy.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from source_worker import problem, rough_field  # noqa: E402,F401

BLOCK = (slice(10, 14), slice(20, 25))  # frame-inclusive cells cut off from the rest: all four faces zero


def two_materials(n, seed=1, rows=None):
    """Frame-inclusive cell conductivities: 1.0 or 0.01 at random (100 : 1), each times uniform(0.5, 1)."""
    import numpy as np
    shape = ((n if rows is None else rows) + 2, n + 2)
    rng = np.random.default_rng(3000 + seed)
    return rng.choice([1.0, 0.01], shape) * rng.uniform(0.5, 1.0, shape)


def rough_faces(n, dtype, seed=1, rows=None, closed=False):
    """(RX, RY) of two_materials(): 0.25 times the harmonic mean of the two cells of a face, so
    the face sum of a point is at most 1; 3 % of the faces exactly 0 (walls); the cells of BLOCK
    with all four faces 0. closed: every face to the frame 0 (nothing leaves the domain). The
    entries no point uses (the last column and the frame rows of RX, the last row and the frame
    columns of RY) hold NaN: the engine must ignore them. No -0.0."""
    import numpy as np
    dt = np.float64 if dtype == "fp64" else np.float32
    k = two_materials(n, seed, rows)
    rng = np.random.default_rng(4000 + seed)

    def hmean(a, b):
        return 2.0 * a * b / (a + b)

    RX = np.full(k.shape, np.nan)
    RY = np.full(k.shape, np.nan)
    RX[1:-1, :-1] = 0.25 * hmean(k[1:-1, :-1], k[1:-1, 1:])
    RY[:-1, 1:-1] = 0.25 * hmean(k[:-1, 1:-1], k[1:, 1:-1])
    RX[rng.uniform(size=k.shape) < 0.03] *= 0.0
    RY[rng.uniform(size=k.shape) < 0.03] *= 0.0
    bi, bj = BLOCK
    RX[bi, bj.start - 1:bj.stop] = 0.0  # west face of the first column .. east face of the last
    RY[bi.start - 1:bi.stop, bj] = 0.0
    RX[bi, bj] = 0.0
    RY[bi, bj] = 0.0
    if closed:
        RX[1:-1, 0] = RX[1:-1, -2] = 0.0
        RY[0, 1:-1] = RY[-2, 1:-1] = 0.0
    RX[0] = RX[-1] = RX[:, -1] = np.nan
    RY[-1] = RY[:, 0] = RY[:, -1] = np.nan
    return np.abs(RX).astype(dt), np.abs(RY).astype(dt)


def face_sum(RX, RY):
    """RX[i,j] + RX[i,j-1] + RY[i,j] + RY[i-1,j] at the owned points, in float64."""
    import numpy as np
    RX, RY = RX.astype(np.float64), RY.astype(np.float64)
    return RX[1:-1, 1:-1] + RX[1:-1, :-2] + RY[1:-1, 1:-1] + RY[:-2, 1:-1]


def signed_field(n, dtype, seed=0, rows=None):
    """The conservation test's data: rough_field()'s magnitudes, positive in the cells of the poor
    conductor of two_materials() and negative in the good one (hot inclusions in a cold matrix).
    What the map form creates per step is sum_i T_i (sum_nb r_nb - 4 r_i): it averages out where
    the sign is independent of the material and is largest where the temperature follows it, the
    case a composite is modelled for."""
    import numpy as np
    T = rough_field(n, dtype, seed, rows)
    return np.where(two_materials(n, rows=rows) < 0.02, T, -T).astype(T.dtype)


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
    s = HeatSolver(p, dtype=a["dtype"], backend="cpu", tb=a["tb"], arith=a["arith"], transport=TorchDistTransport(),
                   faces=rough_faces(a["n"], a["dtype"]))  # (the global arrays: every rank slices its rows)
    # the owned points of rough_field() inside the problem's own Dirichlet frame
    lay = s.layout
    s.upload(rough_field(a["n"], a["dtype"])[1:-1, 1:-1][lay.row0:lay.row0 + lay.nrows])
    s.step(a["steps"])
    full = s.gather()
    if rank == 0:
        np.save(os.path.join(outdir, "result.npy"), full)
    s.close()
    dist.barrier()
    dist.destroy_process_group()


def main(argv):
    if argv[0] == "gloo":
        return gloo(argv[1:])
    outdir, a = argv[0], json.loads(argv[1])
    import numpy as np
    import torch

    from heat2d.models.heat2d import HeatSolver
    torch.cuda.set_device(0)
    rows = a.get("rows")
    p = problem(a["n"], a["steps"], a["sigma"])
    s = HeatSolver(p, dtype=a["dtype"], backend="hip", tb=a["tb"], arith=a["arith"], device=0, rows=rows,
                   graph=bool(a.get("graph")), faces=rough_faces(a["n"], a["dtype"], rows=rows))
    s.upload(rough_field(a["n"], a["dtype"], rows=rows))
    sizes = a.get("calls", [a["steps"]])  # the step() calls that make up the steps (tests/cycles.py calls())
    assert sum(sizes) == a["steps"]
    for m in sizes:
        s.prepare(m)
        s.step(m)
    np.save(os.path.join(outdir, "result.npy"), s.download())
    with open(os.path.join(outdir, "info.json"), "w") as f:
        json.dump({"plan": s.plan(a["tb"]), "info": {k: v for k, v in s.info().items() if k in ("tb", "arith", "faces")},
                   "cycle_hist": {str(k): v for k, v in s.cycle_hist().items()}}, f)
    s.close()


if __name__ == "__main__":
    main(sys.argv[1:])
