"""Memory-fit planner: the largest grid a run can hold in device memory.

The reference sizes nothing — its grid is input.dat's n, allocated as two
device fields plus a whole-field host mirror (fortran/hip/heat.F90:161-176),
so its largest run is whatever the user guessed. Here the IC is generated on
the device and nothing mirrors the field on the host, so a rank's footprint is
its solver's two pitched fields with their ghost bands plus a few KiB of
workspaces — solver_footprint() in csrc/runtime/solver.cpp, the very formula
the Solver constructor allocates by (tests/test_memory_plan.py). The planner
finds the largest n x n grid whose largest slab fits the free device memory
(hipMemGetInfo) minus a reserve for what the solver does not own: the HIP
runtime's growth, the transport's buffers (RCCL channels), hipRTC modules of
the field check and graph workspaces.

    heat2d.utils.memplan.plan_max_grid("fp32", nranks=1)   # ~186k^2 on one MI355X
    bench.py --weak --dtype fp32 --grid max                 # full-HBM weak scaling
    heat2d input.dat --n max                                # the native CLI
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

from ..ops import _native as N

DTYPES = {"fp32": 0, "float32": 0, "fp64": 1, "float64": 1}

# not owned by the solver: runtime growth, RCCL's channel buffers, modules
RESERVE_FIXED = 2 << 30
RESERVE_FRACTION = 0.01


def reserve_bytes(free_bytes: int) -> int:
    """Device memory left unplanned for what the solver does not allocate."""
    return int(RESERVE_FIXED + RESERVE_FRACTION * free_bytes)


def mem_info(device: int = 0) -> tuple:
    """(free, total) device bytes (hipMemGetInfo)."""
    f, t = C.c_int64(), C.c_int64()
    N.call("heat2d_mem_info", int(device), C.byref(f), C.byref(t))
    return f.value, t.value


def probe_bytes(probes: int, probe_steps: int, dtype: str = "fp32") -> int:
    """Device bytes of a rank that holds ``probes`` probe points with room for
    ``probe_steps`` steps (Solver::set_probes): the history, the index list and
    the row-base word. The worst case of a decomposition: every point on one rank."""
    if probes <= 0:
        return 0
    return int(probes) * int(probe_steps) * (8 if DTYPES[dtype] else 4) + 16 * int(probes) + 8


MAX_TB_SRC = 16  # common.hpp kMaxTBSrc: the padding past a gain schedule's end


def gain_bytes(source_gain: int, dtype: str = "fp32") -> int:
    """Device bytes of a source gain schedule of that many entries
    (HeatSolver source_gain=): the padded array and the two position words."""
    if source_gain <= 0:
        return 0
    return (int(source_gain) + MAX_TB_SRC) * (8 if DTYPES[dtype] else 4) + 16


def footprint(n: int, nranks: int = 1, dtype: str = "fp32", rank: int = 0, backend: str = "hip",
              source: bool = False, rmap: bool = False, faces: bool = False, probes: int = 0,
              probe_steps: int = 0, source_gain: int = 0) -> dict:
    """Device bytes of one rank's solver for an n x n grid on nranks ranks:
    {"field_bytes", "work_bytes", "total_bytes"} (the constructor's allocations).
    source: a solver with a heat source (a third buffer in the field's layout);
    rmap: one with a diffusivity map (one more); faces: one with per-face
    diffusion numbers (two more); probes, probe_steps: one with that many probe
    points and room for that many steps (probe_bytes, counted as work bytes);
    source_gain: one with a gain schedule of that many entries (gain_bytes, work bytes)."""
    cfg = N.Config()
    cfg.n_rows = cfg.n_cols = int(n)
    cfg.dtype = DTYPES[dtype]
    cfg.backend = N.BACKEND_HIP if backend == "hip" else N.BACKEND_CPU
    cfg.source = int(bool(source))
    cfg.rmap = int(bool(rmap))
    cfg.faces = int(bool(faces))
    out = (C.c_int64 * 3)()
    N.call("heat2d_solver_footprint", C.byref(cfg), int(rank), int(nranks), out)
    pb = probe_bytes(probes, probe_steps, dtype) + gain_bytes(source_gain, dtype)
    return {"field_bytes": out[0], "work_bytes": out[1] + pb, "total_bytes": out[2] + pb}


def plan_max_grid(dtype: str = "fp32", nranks: int = 1, free_bytes: Optional[int] = None, device: int = 0,
                  reserve: Optional[int] = None, source: bool = False, rmap: bool = False,
                  faces: bool = False, probes: int = 0, probe_steps: int = 0, source_gain: int = 0) -> dict:
    """The largest n x n grid of ``dtype`` whose largest slab on ``nranks``
    ranks fits ``free_bytes`` (default: this device's hipMemGetInfo free
    memory) minus ``reserve`` (default: reserve_bytes(free)). Returns {"n",
    "free_bytes", "reserve_bytes", "footprint_bytes" (rank 0's solver),
    "fraction_of_free"}."""
    free = mem_info(device)[0] if free_bytes is None else int(free_bytes)
    res = reserve_bytes(free) if reserve is None else int(reserve)
    n = C.c_int64()
    pb = probe_bytes(probes, probe_steps, dtype) + gain_bytes(source_gain, dtype)  # (does not grow with n: off the budget)
    N.call("heat2d_plan_max_grid_faces", DTYPES[dtype], int(nranks), int(free - res - pb), int(bool(source)),
           int(bool(rmap)), int(bool(faces)), C.byref(n))
    fp = footprint(n.value, nranks, dtype, source=source, rmap=rmap, faces=faces, probes=probes,
                   probe_steps=probe_steps, source_gain=source_gain)["total_bytes"]
    return {"n": int(n.value), "nranks": int(nranks), "dtype": dtype, "free_bytes": free, "reserve_bytes": res,
            "footprint_bytes": fp, "fraction_of_free": fp / free if free > 0 else 0.0}
