"""Worker for tests/test_probes.py.

`python tests/probes_worker.py OUTDIR JSON_ARGS`: one-rank runs with probe
points on the GPU in a fresh process (HEAT2D_SPLIT_ORDER, HEAT2D_BANDS and
HEAT2D_PIPE are read once per process), one per depth in JSON_ARGS["tbs"]; for
each depth K it writes OUTDIR/H_K.npy (the history), OUTDIR/P_K.npy (the probe
points, chosen from the plan the solver reports), OUTDIR/T_K.npy (download())
and OUTDIR/info_K.json.

`python tests/probes_worker.py gloo RANK WORLD PORT OUTDIR JSON_ARGS`: one rank
of a run on the CPU twin over torch.distributed (gloo); every rank writes its
columns (OUTDIR/H_RANK.npy) and their positions (OUTDIR/I_RANK.npy).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cycles as Y  # noqa: E402
import instance_matrix as M  # noqa: E402
from source_worker import problem, rough_field  # noqa: E402,F401


def plan_points(n, dtype, k, plan):
    """The probe set of the fused-pass tests: the corners, both columns on either
    side of a strip's useful-width boundary (the one-wave strips' and the main
    launch's own), both rows on either side of a band seam of `plan`, one
    interior point. Global frame-inclusive (i, j)."""
    pts = [(1, 1), (1, n), (n, 1), (n, n), (n // 2, n // 2 + 3)]
    for u in {M.useful(dtype, k), int(plan["main_useful_w"])}:
        if 0 < u < n:
            pts += [(n // 3, u), (n // 3, u + 1), (1, u), (n, u + 1)]
    rects = plan["edge_rects"]
    if rects:  # the first band's last row | the interior's first
        seams = [rects[0][1], rects[-1][0]]
    else:      # one launch of nb row bands per strip (instance_matrix.rect_pieces)
        r0, r1, _, _, nb = plan["main_rect"]
        seams = [r0 + b * (r1 - r0) // nb for b in range(1, max(nb, 1))] or [n // 2]
    for r in seams:
        if 0 < r < n:  # local rows r - 1 | r: global frame-inclusive r, r + 1
            pts += [(r, 1), (r + 1, 1), (r, n // 2), (r + 1, n // 2), (r, n), (r + 1, n)]
    return pts


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
                   probes=a["probes"])  # (the global list: every rank keeps the points of its rows)
    lay = s.layout
    s.upload(rough_field(a["n"], a["dtype"])[1:-1, 1:-1][lay.row0:lay.row0 + lay.nrows])
    s.step(a["steps"])
    np.save(os.path.join(outdir, f"H_{rank}.npy"), s.probe_history())
    np.save(os.path.join(outdir, f"I_{rank}.npy"), s.probe_index)
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
    n, dtype = a["n"], a["dtype"]
    for tb in a["tbs"]:
        steps = 2 * tb + 3
        sizes = Y.calls(tb, steps, 2)  # tb, tb, 3
        s = HeatSolver(problem(n, steps, a["sigma"]), dtype=dtype, backend="hip", tb=tb, arith=a["arith"], device=0)
        plan = s.plan(tb)
        pts = plan_points(n, dtype, tb, plan)
        s.set_probes(pts, steps)
        s.upload(rough_field(n, dtype))
        for m in sizes:
            s.prepare(m)
            s.step(m)
        np.save(os.path.join(outdir, f"H_{tb}.npy"), s.probe_history())
        np.save(os.path.join(outdir, f"P_{tb}.npy"), np.array(pts, dtype=np.int64))
        np.save(os.path.join(outdir, f"T_{tb}.npy"), s.download())
        with open(os.path.join(outdir, f"info_{tb}.json"), "w") as f:
            json.dump({"plan": plan, "probes": s.info()["probes"],
                       "cycle_hist": {str(k): v for k, v in s.cycle_hist().items()}}, f)
        s.close()


if __name__ == "__main__":
    main(sys.argv[1:])
