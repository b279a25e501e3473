"""The heat-equation model: a distributed 2-D FTCS slab solver on the native engine.

One :class:`HeatSolver` per rank (process or host thread). It owns a native
``heat2d::Solver`` (csrc/runtime/solver.cpp) holding this rank's slab of the
global grid in two pitched device (or host) fields, and a transport for the
halo exchange. Everything in the time loop runs natively; Python only issues
``step(n)``.

Parity map (reference -> here):
  * fortran/hip/heat.F90 setup()/heat_eqn()/swap()  -> HeatSolver(problem, backend="hip")
  * fortran/mpi+cuda/heat.F90 (CUDA-aware / staged)  -> RCCL transport (device-direct)
  * fortran/cuda_kernel/heat_managed.F90             -> managed=True
  * fortran/serial/heat.f90                          -> backend="cpu"
  * per-step D2D ``Td_old = Td`` (heat.F90:243)      -> copy_swap=True (parity mode)
"""
from __future__ import annotations

import ctypes as C
import hashlib
from typing import Optional

import numpy as np

from ..ops import _native as N
from ..ops import kernels as K
from ..parallel import transport as T
from ..utils.config import Problem

DTYPES = {"fp32": N.F32, "float32": N.F32, "fp64": N.F64, "float64": N.F64}
NP_DTYPES = {N.F32: np.float32, N.F64: np.float64}


def resolve_backend(backend: str) -> str:
    if backend == "auto":
        try:
            import torch
            return "hip" if torch.cuda.is_available() else "cpu"
        except Exception:  # pragma: no cover
            return "cpu"
    if backend not in ("hip", "cpu"):
        raise ValueError("backend must be hip|cpu|auto")
    return backend


PLAN_ORIGINS = {-1: "none", 0: "planned", 1: "tuned", 2: "cache"}


def _plan(h, k: int) -> dict:
    p, ms, org = N.SplitPlan(), C.c_float(), C.c_int32()
    N.call("heat2d_solver_plan", h, int(k), C.byref(p), C.byref(ms))
    N.call("heat2d_solver_plan_origin", h, int(k), C.byref(org))
    # flags & 8: the interior runs the wave-pair kernel on wide strips; the
    # strip shape of the main launch comes from the library either way
    sw, uw = C.c_int64(), C.c_int64()
    N.call("heat2d_solver_plan_strip_shape", h, int(k), C.byref(sw), C.byref(uw))
    return {"main_strip_w": sw.value, "main_useful_w": uw.value, "pipe": int((p.flags >> 3) & 1), "k": p.k, "ring": p.ring, "valid": p.valid,
            "order": ("lead" if p.valid == 1 and p.flags & 4 else
                      {1: "concurrent", 2: "single", 3: "edge-first"}.get(p.valid, "serial")),
            "dynamic": int((p.flags >> 1) & 1), "origin": PLAN_ORIGINS.get(org.value, "?"),
            "main_bands": p.main.nb, "main_items": p.main_items, "main_waves": p.main_waves,
            "edge_items": p.edge_items, "edge_waves": p.edge_waves, "tuned_ms": ms.value,
            "main_rect": [p.main.r0, p.main.r1, p.main.s0, p.main.s1, p.main.nb],
            "edge_rects": [[e.r0, e.r1, e.s0, e.s1, e.nb] for e in list(p.edge)[:p.nedge]],
            # the rects launched instead of main_rect: frame-weighted (arith 2)
            "main_rects": [[e.r0, e.r1, e.s0, e.s1, e.nb] for e in list(p.rects)[:p.nrects]]}


def _cycle_hist(h, reset: bool) -> dict:
    n = N.max_tb() + 1
    out = (C.c_int64 * n)()
    N.call("heat2d_solver_cycle_hist", h, out, n, int(bool(reset)))
    return {k: int(out[k]) for k in range(n) if out[k]}


def _source_array(source, nrows_global: int, ncols: int, np_dtype) -> np.ndarray:
    """The global frame-inclusive source array in the field's dtype (a wrong shape fails)."""
    a = np.ascontiguousarray(source, dtype=np_dtype)
    if a.shape != (nrows_global + 2, ncols + 2):
        raise ValueError(f"source must be the frame-inclusive global array {(nrows_global + 2, ncols + 2)}, "
                         f"got {a.shape}")
    return a


def _gain_array(source_gain, np_dtype) -> np.ndarray:
    """The gain schedule in the field's dtype: 1-D, non-empty, every entry
    finite and >= 0 (ValueError otherwise). The solver's copy of the source
    holds -0.0 at pinned points and g * -0.0 keeps -0.0 only for g >= 0: the
    sign of the heating belongs into the source."""
    a = np.asarray(source_gain)
    if a.ndim != 1 or a.size == 0:
        raise ValueError(f"source_gain must be a non-empty 1-D array, got shape {a.shape}")
    a = np.ascontiguousarray(a, dtype=np_dtype)
    if not np.isfinite(a).all() or (a < 0).any():
        raise ValueError("source_gain entries must be finite and >= 0 (put the sign into the source)")
    return a


def _gain_info(h) -> dict:
    """info()["source_gain"]: whether a schedule is set, its length and the
    position of the next step's entry."""
    v = (C.c_int64 * 3)()
    N.call("heat2d_solver_source_gain", h, v)
    return {"set": bool(v[0]), "length": int(v[1]), "position": int(v[2])}


def _source_info(h) -> dict:
    """info()["source"]: whether the solver was built for a heat source, whether
    one is set, and the depth clamp that then applies (0: none)."""
    v = (C.c_int32 * 3)()
    N.call("heat2d_solver_source", h, v)
    return {"enabled": bool(v[0]), "set": bool(v[1]), "max_tb": int(v[2]) if v[0] else 0}


def _rmap_array(rmap, nrows_global: int, ncols: int, np_dtype) -> np.ndarray:
    """The global frame-inclusive diffusivity map in the field's dtype (a wrong
    shape, or an owned entry that is negative or not finite, fails)."""
    a = np.ascontiguousarray(rmap, dtype=np_dtype)
    if a.shape != (nrows_global + 2, ncols + 2):
        raise ValueError(f"rmap must be the frame-inclusive global array {(nrows_global + 2, ncols + 2)}, "
                         f"got {a.shape}")
    own = a[1:-1, 1:-1]
    if not (np.isfinite(own).all() and (own >= 0).all()):
        raise ValueError("the owned entries of rmap must be finite and >= 0")
    return a


def _rmap_info(h) -> dict:
    """info()["rmap"]: whether the solver was built for a diffusivity map,
    whether one is set, and the depth clamp that then applies (0: none)."""
    v = (C.c_int32 * 3)()
    N.call("heat2d_solver_rmap", h, v)
    return {"enabled": bool(v[0]), "set": bool(v[1]), "max_tb": int(v[2]) if v[0] else 0}


def rmap_from_nu(problem: Problem, nu_xy) -> np.ndarray:
    """The diffusion-number map of a diffusivity field: ``problem.r * nu_xy /
    problem.nu`` in float64 (r = nu dt / dx^2 scales with nu; ``nu_xy`` is nu on
    the frame-inclusive grid, the array ``rmap=`` takes)."""
    return np.float64(problem.r) * np.asarray(nu_xy, dtype=np.float64) / np.float64(problem.nu)


def _faces_arrays(faces, nrows_global: int, ncols: int, np_dtype) -> tuple:
    """The two global frame-inclusive face arrays in the field's dtype (a wrong
    shape, or a used face that is negative or not finite, fails). Used: RX[i, j]
    for i = 1..n, j = 0..n; RY[i, j] for i = 0..n, j = 1..n."""
    try:
        rx, ry = faces
    except (TypeError, ValueError):
        raise ValueError("faces must be a pair (RX, RY) of frame-inclusive arrays") from None
    rx = np.ascontiguousarray(rx, dtype=np_dtype)
    ry = np.ascontiguousarray(ry, dtype=np_dtype)
    want = (nrows_global + 2, ncols + 2)
    if rx.shape != want or ry.shape != want:
        raise ValueError(f"faces must be two frame-inclusive global arrays {want}, got {rx.shape} and {ry.shape}")
    for used in (rx[1:-1, :-1], ry[:-1, 1:-1]):
        if not (np.isfinite(used).all() and (used >= 0).all()):
            raise ValueError("the used face coefficients must be finite and >= 0")
    return rx, ry


def faces_sum_max(rx, ry) -> float:
    """max over the owned points of RX[i,j] + RX[i,j-1] + RY[i,j] + RY[i-1,j]: the
    4r of the scalar case (above 1 FTCS is unstable)."""
    rx = np.asarray(rx, dtype=np.float64)
    ry = np.asarray(ry, dtype=np.float64)
    return float((rx[1:-1, 1:-1] + rx[1:-1, :-2] + ry[1:-1, 1:-1] + ry[:-2, 1:-1]).max())


def _faces_sha256(rx: np.ndarray, ry: np.ndarray) -> str:
    """What a checkpoint records of the faces: the digest of the converted arrays' bytes, RX then RY."""
    return hashlib.sha256(rx.tobytes() + ry.tobytes()).hexdigest()


def _faces_info(h) -> dict:
    """info()["faces"]: whether the solver was built for face coefficients,
    whether they are set, and the depth clamp that then applies (0: none)."""
    v = (C.c_int32 * 3)()
    N.call("heat2d_solver_faces", h, v)
    return {"enabled": bool(v[0]), "set": bool(v[1]), "max_tb": int(v[2]) if v[0] else 0}


def faces_from_k(problem: Problem, k_xy, mean: str = "harmonic") -> tuple:
    """The per-face diffusion numbers (RX, RY) of a cell conductivity
    (diffusivity) field ``k_xy`` on the frame-inclusive grid, in float64:
    ``dt / dx^2`` (= problem.r / problem.nu) times the mean of the two cells a
    face separates. ``mean``: "harmonic" (2ab / (a + b), conductors in series —
    the default) or "arithmetic"; the mean of a 0 and anything is 0 (a wall).
    RX[i, j] is the face between (i, j) and (i, j+1), RY[i, j] the one between
    (i, j) and (i+1, j); the unused last column / row is 0."""
    if mean not in ("harmonic", "arithmetic"):
        raise ValueError(f"mean must be 'harmonic' or 'arithmetic', got {mean!r}")
    k = np.asarray(k_xy, dtype=np.float64)
    m = problem.n_owned + 2
    if k.shape != (m, m):
        raise ValueError(f"k_xy must be the frame-inclusive grid {(m, m)}, got {k.shape}")
    scale = np.float64(problem.r) / np.float64(problem.nu)

    def face(a, b):
        zero = (a == 0) | (b == 0)
        if mean == "arithmetic":
            v = 0.5 * (a + b)
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                v = 2.0 * a * b / (a + b)
        return np.where(zero, 0.0, v)

    rx = np.zeros((m, m), dtype=np.float64)
    ry = np.zeros((m, m), dtype=np.float64)
    rx[:, :-1] = scale * face(k[:, :-1], k[:, 1:])
    ry[:-1, :] = scale * face(k[:-1, :], k[1:, :])
    return rx, ry


def robin_from_h(problem: Problem, h_over_k: float, t_inf: float) -> tuple:
    """The Robin pair (a, b) of a convective wall, -k du/dn = h (u_wall - t_inf)
    with the wall value u_wall = (C + G) / 2 half a cell outside the adjacent
    owned point C and the outward derivative (G - C) / dx: with beta =
    h_over_k * dx (dx: the problem's grid spacing), a = (2 - beta) / (2 + beta)
    and b = 2 beta t_inf / (2 + beta). Computed in float64. beta = 0 is the
    insulated wall (1, 0); beta -> inf approaches the wall at t_inf, (-1, 2 t_inf)."""
    beta = np.float64(h_over_k) * np.float64(problem.delta)
    return float((2.0 - beta) / (2.0 + beta)), float(2.0 * beta * np.float64(t_inf) / (2.0 + beta))


def robin_from_flux(problem: Problem, q_over_k: float) -> tuple:
    """The Robin pair of a prescribed inward heat flux q through the wall,
    k du/dn = q: G = C + (q / k) dx, i.e. (1.0, q_over_k * dx), in float64."""
    return 1.0, float(np.float64(q_over_k) * np.float64(problem.delta))


def robin_wall_temperature(t_wall: float) -> tuple:
    """The Robin pair of a fixed temperature AT the wall (half a cell outside
    the adjacent owned point, not at the frame point): (C + G) / 2 = t_wall,
    i.e. (-1.0, 2 * t_wall), in float64."""
    return -1.0, float(2.0 * np.float64(t_wall))


def weights_from(problem: Problem, nu_x=None, nu_y=None, vx: float = 0.0, vy: float = 0.0, decay: float = 0.0,
                 scheme: str = "upwind") -> tuple:
    """The five weights (wS, wE, wN, wW, wC) of ``weights=`` for
    u_t + v . grad(u) = nu_x u_xx + nu_y u_yy - decay * u on the problem's grid,
    in float64. x is the row axis (toward increasing i), y the column axis;
    nu_x / nu_y default to problem.nu. With rx = nu_x dt/dx², ry = nu_y dt/dx²,
    cx = vx dt/dx, cy = vy dt/dx:
        central: wS = rx - cx/2, wN = rx + cx/2, wE = ry - cy/2, wW = ry + cy/2
        upwind:  wS = rx + max(-cx, 0), wN = rx + max(cx, 0), wE = ry + max(-cy, 0), wW = ry + max(cy, 0)
    and in both wC = 1 - (wS + wE + wN + wW) - decay*dt. A negative weight loses
    the maximum principle (the solvers warn)."""
    if scheme not in ("upwind", "central"):
        raise ValueError(f"scheme must be 'upwind' or 'central', got {scheme!r}")
    f = np.float64
    dt, dx = f(problem.dt), f(problem.delta)
    rx = f(problem.nu if nu_x is None else nu_x) * dt / (dx * dx)
    ry = f(problem.nu if nu_y is None else nu_y) * dt / (dx * dx)
    cx, cy = f(vx) * dt / dx, f(vy) * dt / dx
    if scheme == "central":
        wS, wN, wE, wW = rx - cx / 2, rx + cx / 2, ry - cy / 2, ry + cy / 2
    else:
        wS, wN = rx + max(-cx, f(0)), rx + max(cx, f(0))
        wE, wW = ry + max(-cy, f(0)), ry + max(cy, f(0))
    wC = f(1) - (wS + wE + wN + wW) - f(decay) * dt
    return float(wS), float(wE), float(wN), float(wW), float(wC)


_WEIGHT_NAMES = ("wS", "wE", "wN", "wW", "wC")


def _check_weights(weights, np_dtype, *, arith, engine="tb", copy_swap=False, bc_x, bc_y, source=None, rmap=None,
                   faces=None, source_gain=None):
    """What a solver refuses with ``weights=`` (RuntimeError), the converted 5 doubles, and the
    warning for a negative weight (today's r > 1/4 warning, generalised)."""
    arr, w = N.weights_array(weights, np_dtype)
    if arith in ("jacobi", "fast"):
        raise RuntimeError(f"weights have no arith {arith!r}: the scaled levels assume one r (use exact, fma or auto)")
    if engine == "jit":
        raise RuntimeError("weights need the temporal-blocked engine (engine 'jit' takes one r)")
    if copy_swap:
        raise RuntimeError("weights have no copy-swap mode")
    for name, bc in (("bc_x", bc_x), ("bc_y", bc_y)):
        if bc in ("insulated", "robin"):
            raise RuntimeError(f"weights need 'dirichlet' or 'periodic' axes: {name}={bc!r} has no five-weight kernels")
    for name, v in (("source", source), ("rmap", rmap), ("faces", faces), ("source_gain", source_gain)):
        if v is not None:
            raise RuntimeError(f"weights together with {name}=: no kernel carries them together")
    neg = {n: v for n, v in zip(_WEIGHT_NAMES, w) if v < 0}
    if neg:
        import warnings
        warnings.warn("negative weight " + ", ".join(f"{n} = {v:.6g}" for n, v in neg.items()) +
                      ": the update is no convex combination, the maximum principle is lost", RuntimeWarning, stacklevel=3)
    return arr, w


def _weights_info(h) -> dict:
    """info()["weights"]: whether the native solver runs with weights, the values it runs (converted to the
    run's dtype; None without) and the depth clamp of the five-weight kernels."""
    v, s, m = (C.c_double * 5)(), C.c_int32(), C.c_int32()
    N.call("heat2d_solver_weights", h, v, C.byref(s), C.byref(m))
    return {"set": bool(s.value), "values": tuple(float(x) for x in v) if s.value else None, "max_tb": int(m.value)}


def _robin_info(h, bc_x: str, bc_y: str) -> dict:
    """info()["robin"]: the pairs the native solver runs (converted to the
    run's dtype) for the sides of its Robin axes, and the depth clamp of the
    Robin kernels (0 without a Robin axis)."""
    v, m = (C.c_double * 8)(), C.c_int32()
    N.call("heat2d_solver_robin", h, v, C.byref(m))
    sides = [s for ax, bc in (("x", bc_x), ("y", bc_y)) if bc == "robin" for s in (ax + "_lo", ax + "_hi")]
    out = {s: (float(v[2 * N.ROBIN_SIDES.index(s)]), float(v[2 * N.ROBIN_SIDES.index(s) + 1])) for s in sides}
    out["max_tb"] = int(m.value)
    return out


def _set_robin(cfg, robin, bc_x: str, bc_y: str, np_dtype) -> dict:
    """Check ``robin=`` against the axes (ValueError: a missing or surplus side,
    an entry that is not finite) and put the converted pairs into the config."""
    arr, pairs = N.robin_array(robin, bc_x, bc_y, np_dtype)
    for i in range(8):
        cfg.robin[i] = arr[i]
    return pairs


def _arith(h) -> int:
    """The arithmetic form (ops._native.ARITH code) a native solver runs: "auto" resolved."""
    v = C.c_int32()
    N.call("heat2d_solver_arith", h, C.byref(v))
    return v.value


class HeatSolver:
    """Distributed FTCS solver for one rank.

    Args:
        problem: resolved :class:`~utils.config.Problem`.
        dtype: "fp64" (reference precision) or "fp32".
        backend: "hip", "cpu" or "auto".
        tb: largest temporal-block depth K (time steps fused per HBM pass; fp64
            1..24, fp32 1..20). 0: all depths up to that limit for the measured
            schedules of prepare() (autotuned slabs), balanced cycles of the
            steady-state best (fp64 14 / fp32 16) otherwise; 8 on the CPU twin.
        overlap: boundary/interior split with the halo exchange on a comm stream.
        copy_swap: reference-parity schedule (full field copy every step, K=1).
        managed: allocate fields with hipMallocManaged.
        graph: replay step pairs from a captured hipGraph (single-rank / serial schedule).
        transport: a :class:`parallel.transport.Transport`; default picks self / RCCL / gloo.
        device: HIP device ordinal (default: torch's current device).
        comm_cus: room for the bands + RCCL beside the interior kernel when
            overlapping: >0 CUs masked off the compute stream; 0 (default): the
            interior planned for all wave slots but 8 spare ones, no mask; -1 none.
        engine: "tb" — the temporal-blocked gfx950 kernels; "jit" — a kernel
            rendered for this slab and r and compiled at run time with hipRTC
            (one step per launch; the reference's PyCUDA program, ops/jit.py).
        autotune: overlapped (split) schedule: time candidate (ring, band count)
            launch plans on the first cycle of each depth and keep the fastest
            (-1: only for slabs of >= 2**24 points, 0: off, 1: on).
        rows: solve only the first ``rows`` x-rows of the grid (a rectangular
            rows x n domain, e.g. one rank's slab shape for a 1-GPU rehearsal).
        slab_row0: with ``rows``: own rows [slab_row0, slab_row0 + rows) of the
            WHOLE grid instead — a middle rank's slab (its boundary bands are
            interior bands, as on rank 3 of 8) for 1-GPU rehearsals.
        arith: "exact" — every operation of the reference update rounded as
            written (-ffp-contract=off; bitwise equal to the NumPy golden);
            "fma" — the update contracted to fma(r, sum - 4c, c), what hipcc's
            default contraction makes of fortran/hip/heat_kernel.cpp:43: one op
            fewer per point; identical to "exact" when r is a power of two
            (sigma = 0.25), bitwise equal to the CPU twin for any r;
            "jacobi" — r == 1/4 only: the centre weight 1 - 4r is zero and the
            update is r * (((S + E) + N) + W) (3 adds per interior point and
            level in the kernels instead of 5); bitwise equal to the CPU twin
            and to models.reference.ftcs(arith="jacobi"), and to "exact"
            wherever sum - 4c is exact (e.g. the reference IC, values in [1, 2]).
        edge_shift: rows each edge slab (rank 0 and the last rank: the global
            frame rows on one side) gives to the middle slabs of a >= 3-rank
            decomposition (common.hpp decompose): an edge slab's cycle costs
            more per row, and a step lasts as long as the slowest rank;
            bench.py measures the excess and picks the shift. Same on every rank.
        bc_x, bc_y: boundary condition of the row (x, decomposed over ranks) and
            column (y) axis: "dirichlet" (the frame keeps its values),
            "periodic" (the n owned points are the period) or "insulated" (a
            zero-flux wall half a cell outside the first and last owned point;
            the frame entries are images of the adjacent owned point). The
            results are bitwise equal to models.reference.ftcs(bc_x=, bc_y=)
            at any depth, plan and rank count; engine "tb" only, no copy_swap;
            on more than one rank periodic x runs on the loopback, host-thread
            and torch.distributed (host-staged) transports (insulated x: every
            transport); "insulated" not with arith "fast".
            "robin": a Robin (convective) wall in the insulated geometry, with
            ``robin=`` (below).
        robin: ``{"x_lo": (a, b), "x_hi": (a, b), "y_lo": (a, b), "y_hi": (a, b)}``
            for exactly the sides of the axes that are "robin" (x_lo: the wall
            before the first owned row, x_hi: after the last; y_*: columns); a
            missing or surplus key raises ValueError. The value beyond a wall
            is the ghost G = a * C + b of the adjacent owned point C (the
            product rounded, then the add; arith "fma": fma(a, C, b)), formed
            at every fused level, so K fused levels have the bits of K single
            steps of models.reference.ftcs(robin=) at any depth, plan and rank
            count. a and b finite, converted to the run's dtype
            (:func:`robin_from_h`, :func:`robin_from_flux`,
            :func:`robin_wall_temperature`); (1, -0.0) is the insulated wall,
            bit for bit. arith "exact" / "fma" ("auto": fma when r is a power
            of two, else exact — never jacobi), engine "tb", no copy_swap, no
            source / rmap / faces; info()["robin"] holds the converted pairs
            and the depth clamp.
        weights: (wS, wE, wN, wW, wC), the constant-coefficient five-point
            operator T' = wS*S + wE*E + wN*N + wW*W + wC*C at every fused level
            (S = T[i+1,j], E = T[i,j+1], N = T[i-1,j], W = T[i,j-1], C = T[i,j];
            :func:`weights_from` computes them for a moving medium, unequal
            diffusivities on the two axes and a linear loss). Every product and
            sum is rounded, ((((wS*S + wE*E) + wN*N) + wW*W) + wC*C); "fma": the
            first product, then one fma per further operand: bitwise equal to
            models.reference.ftcs(weights=) at any depth, plan and rank count.
            problem.r is not used. Five finite entries, converted to the run's
            dtype; a negative one warns (the maximum principle is lost).
            "dirichlet" / "periodic" axes, arith "exact" / "fma" ("auto": fma),
            engine "tb", no copy_swap, no source / rmap / faces / source_gain
            (RuntimeError). :meth:`set_weights` replaces or drops them between
            steps; info()["weights"] holds the converted values and the depth clamp.
        source: a heat source, u_t = nu lap(u) + f: the GLOBAL frame-inclusive
            array (rows + 2) x (n + 2) of the per-step increment S = dt * f (the
            solver does no scaling; converted to the field's dtype; its frame
            entries are ignored). One step is the update followed by one
            separately rounded add, T' = update(T) + S, at every fused level:
            bitwise equal to models.reference.ftcs(source=) at any depth, plan
            and rank count. Each rank slices its own rows. Dirichlet axes,
            engine "tb", no copy_swap, arith "exact" / "fma" ("auto" picks fma
            when r is a power of two, else exact — never jacobi); the depth is
            clamped to the source kernels' deepest pass (info()["source"]).
            :meth:`set_source` replaces or clears it between steps.
        source_gain: with source=, a 1-D array G of per-step gains, finite and
            >= 0, converted to the run's dtype: the separable time-dependent
            source G[q] * S. The step at position q adds G[q] * S — the product
            rounded, then the add; "fma": fma(G[q], S, update), one rounding —
            at every fused level of any pass (models.reference.ftcs(source_gain=)
            bitwise). The position starts at 0 and moves by one per step taken by
            step() / step_stats(), however the call is cut into cycles; prepare()
            and the autotuner consume nothing; a step(n) past the end of G raises
            before it launches anything. G == 1 gives the bits of source= alone.
            :meth:`set_source_gain` replaces or clears it between steps.
        rmap: a diffusivity map, u_t = nu(x, y) lap(u) (the NON-divergence
            form: variable heat capacity over constant conductivity; not
            div(k grad u)): the GLOBAL frame-inclusive array (rows + 2) x
            (n + 2) of the per-point diffusion number R = nu(x, y) dt / dx^2
            (:func:`rmap_from_nu`; the solver does no scaling; converted to the
            field's dtype; frame entries are ignored; owned entries finite and
            >= 0). One step is T' = C + R[i,j] * (sum - 4C) in the reference's
            operand order ("fma": fma(R, fma(-4, C, sum), C)), bitwise equal to
            models.reference.ftcs(rmap=) at any depth, plan and rank count;
            R == 0 holds a point at its value. Each rank slices its own rows.
            Dirichlet axes, engine "tb", no copy_swap, no source, arith "exact"
            / "fma" ("auto" is exact); the depth is clamped to the map kernels'
            deepest pass (info()["rmap"]). :meth:`set_rmap` replaces it, or
            returns to the scalar r, between steps.
        faces: the conservative form u_t = div(k grad u): a pair (RX, RY) of
            GLOBAL frame-inclusive arrays (rows + 2) x (n + 2) of per-face
            diffusion numbers, already multiplied by dt / dx^2
            (:func:`faces_from_k`; the solver does no scaling; converted to the
            field's dtype). RX[i, j] is the face between (i, j) and (i, j+1)
            (used for j = 0..n), RY[i, j] the one between (i, j) and (i+1, j)
            (used for i = 0..n); used faces finite and >= 0. One step is
            T' = C + (((RY[i,j]*(S-C) + RX[i,j]*(E-C)) + RY[i-1,j]*(N-C)) +
            RX[i,j-1]*(W-C)) ("fma": the sums contracted), bitwise equal to
            models.reference.ftcs(faces=) at any depth, plan and rank count.
            What a face takes from one cell it gives the other; a zero face is
            a wall. Dirichlet axes, engine "tb", no copy_swap, no source, no
            rmap, arith "exact" / "fma" ("auto" is exact); the depth is clamped
            to info()["faces"]["max_tb"]. :meth:`set_faces` replaces them, or
            returns to the scalar r, between steps.
        probes: P owned points (i, j) in global frame-inclusive indices,
            1 <= i, j <= n (shape (P, 2), integers, duplicates allowed, at most
            4096), whose temperature is recorded after EVERY step — the levels
            inside a fused pass included, which exist only in registers. One
            history row per step taken by step() / step_stats(), however the
            call is cut into cycles; prepare() records nothing.
            :meth:`probe_history` returns it, bitwise equal to
            models.reference.probe_history wherever the field equals
            models.reference.ftcs bitwise. A small kernel beside the march
            advances the patch around each probe (csrc/kernels/probe_cone.hip);
            no stencil kernel changes. Each rank keeps the probes of its rows
            (:attr:`probe_index`). Not with arith "fast", engine "jit" or
            copy_swap. :meth:`set_probes` replaces or clears them between steps.
        probe_steps: steps the history has room for (default problem.ntime); a
            step(n) that would overflow it raises before it launches anything.
    """

    def __init__(self, problem: Problem, *, dtype: str = "fp64", backend: str = "auto", tb: int = 0,
                 overlap: bool = True, copy_swap: bool = False, managed: bool = False, graph: bool = False,
                 tile_rows: int = 0, halo: int = 0, transport: Optional[T.Transport] = None,
                 device: Optional[int] = None, init: bool = True, rows: Optional[int] = None,
                 comm_cus: int = 0, autotune: int = -1, engine: str = "tb", arith: str = "auto",
                 slab_row0: Optional[int] = None, edge_shift: int = 0, bc_x: str = "dirichlet",
                 bc_y: str = "dirichlet", source=None, rmap=None, faces=None, probes=None,
                 probe_steps: Optional[int] = None, source_gain=None, robin=None, weights=None):
        self.problem = problem
        self.edge_shift = 0 if bc_x == "periodic" else int(edge_shift)  # (periodic x: no edge slabs)
        self.bc_x, self.bc_y = bc_x, bc_y
        self.backend = resolve_backend(backend)
        self.dtype = DTYPES[dtype]
        self.np_dtype = NP_DTYPES[self.dtype]
        if self.backend == "hip" and device is None:
            import torch
            device = torch.cuda.current_device()
        self.device = -1 if self.backend == "cpu" else int(device)
        self.transport = transport or T.default_transport(self.backend, None if self.device < 0 else self.device)
        cfg = N.Config()
        if rows is not None and not 1 <= rows <= problem.n_owned:
            raise ValueError(f"rows must be in [1, {problem.n_owned}]")
        cfg.n_rows = problem.n_owned if rows is None else int(rows)  # rows < n: the first rows x n of the grid
        if slab_row0 is not None:  # 1-rank rehearsal of the middle slab rows [slab_row0, slab_row0 + rows)
            if rows is None or not 0 <= slab_row0 <= problem.n_owned - rows:
                raise ValueError("slab_row0 needs rows and must keep the slab inside the grid")
            cfg.slab_row0 = int(slab_row0)
            cfg.slab_rows_global = problem.n_owned
        cfg.n_cols = problem.n_owned
        cfg.dtype = self.dtype
        cfg.backend = N.BACKEND_HIP if self.backend == "hip" else N.BACKEND_CPU
        cfg.r = problem.r
        cfg.tb = tb
        cfg.overlap = int(overlap)
        cfg.copy_swap = int(copy_swap)
        cfg.managed = int(managed)
        cfg.device = self.device
        cfg.use_graph = int(graph)
        cfg.tile_rows = tile_rows
        cfg.halo = halo
        cfg.comm_cus = comm_cus
        cfg.autotune = autotune
        cfg.edge_shift = self.edge_shift
        cfg.bc_x = N.bc_code(bc_x, "bc_x")
        cfg.bc_y = N.bc_code(bc_y, "bc_y")
        self.robin = _set_robin(cfg, robin, bc_x, bc_y, self.np_dtype)  # the converted pairs of the Robin sides
        if engine not in ("tb", "jit"):
            raise ValueError("engine must be 'tb' (temporal-blocked kernels) or 'jit' (hipRTC, one step per launch)")
        cfg.engine = 1 if engine == "jit" else 0
        if arith not in N.ARITH:
            raise ValueError(f"arith must be one of {sorted(N.ARITH)}")
        cfg.arith = N.ARITH[arith]
        self.arith = arith
        self.weights = None  # the converted five weights (set_weights)
        if weights is not None:  # (refused before anything is built)
            _check_weights(weights, self.np_dtype, arith=arith, engine=engine, copy_swap=copy_swap, bc_x=bc_x, bc_y=bc_y,
                           source=source, rmap=rmap, faces=faces, source_gain=source_gain)
        cfg.source = int(source is not None)
        self.source_sha256 = None
        self.source_gain_sha256 = None
        cfg.rmap = int(rmap is not None)
        self.rmap_sha256 = None
        if rmap is not None and arith == "auto":
            self.arith = "exact"  # (the native solver resolves it the same way)
        cfg.faces = int(faces is not None)
        self.faces_sha256 = None
        if faces is not None and arith == "auto":
            self.arith = "exact"
        self._cfg = cfg
        h = C.c_void_p()
        N.call("heat2d_solver_create", C.byref(cfg), self.transport.handle, C.byref(h))
        self._h = h
        self.layout = N.Layout()
        N.call("heat2d_solver_layout", self._h, C.byref(self.layout))
        if source is not None:
            self.set_source(source)
        if source_gain is not None:
            self.set_source_gain(source_gain)
        if rmap is not None:
            self.set_rmap(rmap)
        if faces is not None:
            self.set_faces(faces)
        if weights is not None:
            self.set_weights(weights)
        if probes is not None:
            self.set_probes(probes, probe_steps)
        if init:
            self.init()

    def set_weights(self, weights) -> None:
        """Replace the five weights (wS, wE, wN, wW, wC) of the constant-coefficient
        operator T' = wS*S + wE*E + wN*N + wW*W + wC*C (``weights_from``; operands
        S = T[i+1,j], E = T[i,j+1], N = T[i-1,j], W = T[i,j-1], C = T[i,j]) or
        drop them (None: the scalar-r kernels again, bit for bit), between step()
        calls. problem.r is not used with weights; arith "auto" runs "fma".
        "dirichlet" / "periodic" axes, arith exact / fma / auto, engine "tb", no
        copy_swap, no source / rmap / faces (RuntimeError); five finite entries
        (ValueError); a negative weight warns. Captured graphs are dropped."""
        if weights is None:
            N.call("heat2d_solver_set_weights", self._h, None)
            self.weights = None
            return
        arr, w = _check_weights(weights, self.np_dtype, arith=self.arith, bc_x=self.bc_x, bc_y=self.bc_y)
        N.call("heat2d_solver_set_weights", self._h, arr)
        self.weights = w

    def set_probes(self, points, steps: Optional[int] = None) -> None:
        """Replace the probe points (see the class docstring) or clear them
        (None), between step() calls. The history starts empty, with room for
        ``steps`` steps (default: problem.ntime). Nothing but captured graphs is
        invalidated."""
        if points is None:
            N.call("heat2d_solver_set_probes", self._h, None, 0, 0)
            return
        a = K.probe_points(points, int(self.layout.nrows_global), self.ncols)
        cap = int(self.problem.ntime if steps is None else steps)
        if len(a) and cap < 1:
            raise ValueError(f"probe_steps must be at least 1, got {cap}")
        N.call("heat2d_solver_set_probes", self._h, a.ctypes.data_as(C.c_void_p), len(a), cap)

    def _probes(self) -> dict:
        v = (C.c_int64 * 4)()
        N.call("heat2d_solver_probes", self._h, v)
        return {"count": int(v[0]), "capacity": int(v[1]), "recorded": int(v[2])}

    @property
    def probe_index(self) -> np.ndarray:
        """Positions of this rank's probes in the list set_probes was given (the
        points whose row this rank owns, in the list's order)."""
        n = self._probes()["count"]
        out = (C.c_int64 * max(1, n))()
        N.call("heat2d_solver_probe_index", self._h, out)
        return np.array(out[:n], dtype=np.int64)

    def probe_history(self) -> np.ndarray:
        """The recorded history (recorded, P_local) in the run's dtype: row q
        holds the temperature at this rank's probes after step q + 1 counted
        from set_probes / clear_probe_history. Synchronises."""
        pr = self._probes()
        out = np.empty((pr["recorded"], pr["count"]), dtype=self.np_dtype)
        if out.size:
            N.call("heat2d_solver_probe_history", self._h, out.ctypes.data_as(C.c_void_p))
        return out

    def clear_probe_history(self) -> None:
        """Forget the recorded rows (the probes and the capacity stay)."""
        N.call("heat2d_solver_clear_probe_history", self._h)

    def set_faces(self, faces) -> None:
        """Replace the face coefficients (the pair of global frame-inclusive
        arrays, see the class docstring) or drop them (None: the solver then
        runs the scalar-r kernels), between step() calls. The solver must have
        been created with faces; nothing but captured graphs is invalidated."""
        if faces is None:
            N.call("heat2d_solver_set_faces", self._h, None, None, 0)
            self.faces_sha256 = None
            return
        rx, ry = _faces_arrays(faces, int(self.layout.nrows_global), self.ncols, self.np_dtype)
        N.call("heat2d_solver_set_faces", self._h, rx.ctypes.data_as(C.c_void_p), ry.ctypes.data_as(C.c_void_p),
               rx.shape[1])
        self.faces_sha256 = _faces_sha256(rx, ry)

    def set_rmap(self, rmap) -> None:
        """Replace the diffusivity map (the global frame-inclusive array, see
        the class docstring) or drop it (None: the solver then runs the
        scalar-r kernels), between step() calls. The solver must have been
        created with a map; nothing but captured graphs is invalidated."""
        if rmap is None:
            N.call("heat2d_solver_set_rmap", self._h, None, 0)
            self.rmap_sha256 = None
            return
        a = _rmap_array(rmap, int(self.layout.nrows_global), self.ncols, self.np_dtype)
        N.call("heat2d_solver_set_rmap", self._h, a.ctypes.data_as(C.c_void_p), a.shape[1])
        # what a checkpoint records of the map (utils/checkpoint.py): the digest of the converted array
        self.rmap_sha256 = hashlib.sha256(a.tobytes()).hexdigest()

    def set_source(self, source) -> None:
        """Replace the heat source (the global frame-inclusive array, see the
        class docstring) or clear it (None: the solver then runs as one
        without), between step() calls. The solver must have been created with
        a source; nothing but captured graphs is invalidated."""
        if source is None:
            N.call("heat2d_solver_set_source", self._h, None, 0)
            self.source_sha256 = None
            self.source_gain_sha256 = None  # (a schedule scales a source: cleared with it)
            return
        a = _source_array(source, int(self.layout.nrows_global), self.ncols, self.np_dtype)
        N.call("heat2d_solver_set_source", self._h, a.ctypes.data_as(C.c_void_p), a.shape[1])
        # what a checkpoint records of the source (utils/checkpoint.py): the digest of the converted array
        self.source_sha256 = hashlib.sha256(a.tobytes()).hexdigest()

    # ------------------------------------------------------------------ info
    def set_source_gain(self, source_gain, start: int = 0) -> None:
        """Replace the source's gain schedule (see the class docstring) or clear
        it (None: the source as it is again, bit for bit), between step()
        calls. The next step takes ``source_gain[start]``. Needs a source
        (RuntimeError without one); entries finite and >= 0, 1-D, non-empty
        (ValueError). Synchronises; captured graphs are dropped."""
        if source_gain is None:
            N.call("heat2d_solver_set_source_gain", self._h, None, 0, 0)
            self.source_gain_sha256 = None
            return
        a = _gain_array(source_gain, self.np_dtype)
        if not 0 <= int(start) <= a.size:
            raise ValueError(f"start must be in [0, {a.size}], got {start}")
        N.call("heat2d_solver_set_source_gain", self._h, a.ctypes.data_as(C.c_void_p), a.size, int(start))
        # what a checkpoint records of the schedule: the digest of the converted bytes
        self.source_gain_sha256 = hashlib.sha256(a.tobytes()).hexdigest()

    @property
    def rank(self) -> int:
        return self.transport.rank

    @property
    def size(self) -> int:
        return self.transport.size

    @property
    def row0(self) -> int:
        return int(self.layout.row0)

    @property
    def nrows(self) -> int:
        return int(self.layout.nrows)

    @property
    def ncols(self) -> int:
        return int(self.layout.ncols)

    def info(self) -> dict:
        tb, band, steps = C.c_int32(), C.c_int64(), C.c_int64()
        field, stream = C.c_void_p(), C.c_void_p()
        N.call("heat2d_solver_info", self._h, C.byref(tb), C.byref(band), C.byref(steps), C.byref(field),
               C.byref(stream))
        return {"tb": tb.value, "band": band.value, "steps": steps.value, "field": field.value,
                "stream": stream.value, "backend": self.backend, "transport": self.transport.name,
                "arith": _arith(self._h),  # the resolved code: 0 exact, 1 fma, 2 jacobi, 3 fast
                "bc_x": self._bc()[0], "bc_y": self._bc()[1],  # "dirichlet" | "periodic" | "insulated" | "robin", as the native solver runs
                "robin": _robin_info(self._h, *self._bc()),  # the converted pairs of the Robin sides, "max_tb"
                "source": _source_info(self._h),
                "source_gain": _gain_info(self._h),  # {"set", "length", "position"}
                "rmap": _rmap_info(self._h),
                "faces": _faces_info(self._h),
                "weights": _weights_info(self._h),  # {"set", "values": the converted five or None, "max_tb"}
                "probes": self._probes(),  # {"count": this rank's, "capacity", "recorded"}
                "rank": self.rank, "size": self.size, "layout": self.layout.as_dict()}

    def _bc(self) -> tuple:
        bx, by = C.c_int32(), C.c_int32()
        N.call("heat2d_solver_bc", self._h, C.byref(bx), C.byref(by))
        return N.BC_NAMES[bx.value], N.BC_NAMES[by.value]

    def set_timing(self, on: bool = True) -> None:
        """Record hipEvent phase timers for every cycle from now on (HIP backend)."""
        N.call("heat2d_solver_timing", self._h, int(bool(on)))

    def phase_times(self) -> dict:
        """Sum of the phase timers since the last call (synchronises, then resets):
        main / edge / exchange / cycle milliseconds and the number of cycles."""
        out = (C.c_double * 5)()
        N.call("heat2d_solver_phase_times", self._h, out)
        return {"main_ms": out[0], "edge_ms": out[1], "exchange_ms": out[2], "cycle_ms": out[3],
                "cycles": int(out[4])}

    def prepare(self, n: int) -> None:
        """Plan / autotune every cycle depth a ``step(n)`` will use (call before timing it)."""
        N.call("heat2d_solver_prepare", self._h, int(n))

    def plan(self, k: Optional[int] = None) -> dict:
        """The split plan (MAIN / EDGE launches) used for depth k (default: tb)."""
        return _plan(self._h, self.tb if k is None else k)

    def schedule(self, n: int):
        """Depths of the measured cycle schedule prepare(n) chose for step(n), or None
        (balanced cycles of the preferred depth)."""
        ln = C.c_int64()
        N.call("heat2d_solver_schedule", self._h, int(n), None, 0, C.byref(ln))
        if ln.value < 0:
            return None
        out = (C.c_int32 * max(1, ln.value))()
        N.call("heat2d_solver_schedule", self._h, int(n), out, ln.value, C.byref(ln))
        return [int(v) for v in out[:ln.value]]

    def schedule_replayed(self, n: int) -> bool:
        """Whether step(n) replays its measured schedule as one captured hipGraph
        (graph=True and short cycles; long-cycle schedules launch eagerly)."""
        out = C.c_int32()
        N.call("heat2d_solver_schedule_replayed", self._h, int(n), C.byref(out))
        return bool(out.value)

    def cycle_hist(self, reset: bool = False) -> dict:
        """{depth: cycles} that step() launched since the last reset (graph replays count 2 each)."""
        return _cycle_hist(self._h, reset)

    def step_cycles(self, n: int) -> list:
        """The cycle depths step(n) will run from the current state, in order."""
        ln = C.c_int64()
        N.call("heat2d_solver_step_cycles", self._h, int(n), None, 0, C.byref(ln))
        out = (C.c_int32 * max(1, ln.value))()
        N.call("heat2d_solver_step_cycles", self._h, int(n), out, ln.value, C.byref(ln))
        return [int(v) for v in out[:ln.value]]

    def halo_rows_exchanged(self, reset: bool = False) -> int:
        """Halo rows this rank exchanged per side since the last reset (each
        cycle moves the rows the NEXT cycle reads: its depth, not the maximum)."""
        v = C.c_int64()
        N.call("heat2d_solver_halo_rows", self._h, int(bool(reset)), C.byref(v))
        return v.value

    @property
    def plan_cache_hits(self) -> int:
        """Plans / schedules taken from the persistent plan cache (re-validated by one re-time)."""
        v = C.c_int64()
        N.call("heat2d_solver_plan_cache_hits", self._h, C.byref(v))
        return v.value

    @property
    def tune_stats(self) -> dict:
        """{"depths": depths autotuned in this process, "candidates": plans screened for them}."""
        d, c = C.c_int64(), C.c_int64()
        N.call("heat2d_solver_tune_stats", self._h, C.byref(d), C.byref(c))
        return {"depths": d.value, "candidates": c.value}

    @property
    def ghost_rows(self) -> int:
        """Valid ghost rows of the current field (the last exchange's depth)."""
        v = C.c_int32()
        N.call("heat2d_solver_ghost_rows", self._h, C.byref(v))
        return v.value

    @property
    def plans_made(self) -> int:
        """Split plans made so far (each the first use of a depth; autotuned on
        big slabs). After prepare(n), step(n) must not add any."""
        v = C.c_int64()
        N.call("heat2d_solver_plans_made", self._h, C.byref(v))
        return v.value

    @property
    def tb(self) -> int:
        """Largest temporal depth this solver may run (the halo / band depth)."""
        return self.info()["tb"]

    @property
    def pref_depth(self) -> int:
        """Depth of the balanced cycles when no measured schedule applies."""
        v = C.c_int32()
        N.call("heat2d_solver_pref_depth", self._h, C.byref(v))
        return v.value

    @property
    def steps_done(self) -> int:
        return self.info()["steps"]

    # ------------------------------------------------------------------ ops
    def init(self) -> None:
        x = np.ascontiguousarray(self.problem.x, dtype=np.float64)
        ic = self.problem.ic.to_native()
        N.call("heat2d_solver_init", self._h, C.byref(ic), x.ctypes.data_as(C.c_void_p),
               x.ctypes.data_as(C.c_void_p))

    def step(self, n: int = 1) -> None:
        """Advance n time steps (asynchronous on the GPU)."""
        N.call("heat2d_solver_step", self._h, int(n))

    def step_stats(self, n: int) -> dict:
        """step(n), returning the global statistics of the new field and its
        one-step residual T_n - T_{n-1}, fused into the last cycle's stencil
        launch on the HIP engine (no extra pass over the field)."""
        out = (C.c_double * 6)()
        N.call("heat2d_solver_step_stats", self._h, int(n), out)
        s = list(out)
        return {"sum": s[0], "sum_sq": s[1], "min": s[2], "max": s[3], "residual_l2": float(np.sqrt(s[4])),
                "residual_max": s[5]}

    def run(self, ntime: Optional[int] = None) -> None:
        self.step(self.problem.ntime if ntime is None else ntime)

    def synchronize(self) -> None:
        N.call("heat2d_solver_sync", self._h)

    def stats(self, residual: bool = False) -> dict:
        """Global (all-rank) statistics of the current field (a separate pass).
        residual=True: the one-step residual, available only right after a
        depth-1 cycle (else NaN) — step_stats(n) gives it at any depth."""
        out = (C.c_double * 6)()
        N.call("heat2d_solver_stats", self._h, out, int(residual))
        s = list(out)
        d = {"sum": s[0], "sum_sq": s[1], "min": s[2], "max": s[3]}
        if residual:  # NaN unless the last cycle had depth 1 (see step_stats)
            d["residual_l2"] = float(np.sqrt(s[4]))
            d["residual_max"] = s[5]
        return d

    def download(self) -> np.ndarray:
        """This rank's owned rows (nrows x ncols) as a host array."""
        out = np.empty((self.nrows, self.ncols), dtype=self.np_dtype)
        N.call("heat2d_solver_download", self._h, out.ctypes.data_as(C.c_void_p), self.ncols)
        return out

    def download_field(self) -> np.ndarray:
        """This rank's rows with their frame, (nrows + 2) x (ncols + 2): local
        rows -1 .. nrows (the global frame rows on the first / last rank, else
        the neighbours' rows) and columns -1 .. ncols. On a periodic axis the
        frame entries are wrap images of the owned points, on an insulated one
        images of the adjacent owned point, on a Robin one its ghost values."""
        out = np.empty((self.nrows + 2, self.ncols + 2), dtype=self.np_dtype)
        N.call("heat2d_solver_download_region", self._h, -1, self.nrows + 1, -1, self.ncols + 1,
               out.ctypes.data_as(C.c_void_p), self.ncols + 2)
        return out

    def upload(self, arr: np.ndarray) -> None:
        """Set this rank's owned rows (collective: followed by a halo exchange).
        ``arr``: the owned points (nrows, ncols), or the frame-inclusive local
        field (nrows + 2, ncols + 2) — then the frame lines of a Dirichlet axis
        are set too, and the entries on a periodic, insulated or Robin axis are
        ignored (they become wrap / edge images / ghost values of the owned points)."""
        a = np.ascontiguousarray(arr, dtype=self.np_dtype)
        if a.shape == (self.nrows + 2, self.ncols + 2):
            N.call("heat2d_solver_upload_field", self._h, a.ctypes.data_as(C.c_void_p), self.ncols + 2)
            return
        if a.shape != (self.nrows, self.ncols):
            raise ValueError(f"expected {(self.nrows, self.ncols)} (or the frame-inclusive "
                             f"{(self.nrows + 2, self.ncols + 2)}), got {a.shape}")
        N.call("heat2d_solver_upload", self._h, a.ctypes.data_as(C.c_void_p), self.ncols)

    def compare(self, other: "HeatSolver", r0: int = 0, nrows: Optional[int] = None, other_r0: Optional[int] = None
                ) -> dict:
        """This rank's current field, local rows [r0, r0 + nrows), against
        ``other``'s current field, local rows [other_r0, other_r0 + nrows)
        (default: the same rows), on the device (same GPU, dtype and width):
        {"max_abs_diff": max |a - b| (NaN if either holds one), "mismatches":
        elements whose bit patterns differ}. Local to this rank."""
        n = self.nrows - r0 if nrows is None else int(nrows)
        out = (C.c_double * 2)()
        N.call("heat2d_solver_compare", self._h, other._h, int(r0), n, int(r0 if other_r0 is None else other_r0), out)
        return {"max_abs_diff": float(out[0]), "mismatches": int(out[1])}

    def gather(self) -> Optional[np.ndarray]:
        """Whole owned grid on rank 0 (None elsewhere). Uses torch.distributed when size > 1."""
        local = self.download()
        if self.size == 1:
            return local
        import torch
        import torch.distributed as dist
        parts = [None] * self.size if self.rank == 0 else None
        dist.gather_object(local, parts, dst=0)
        return np.concatenate(parts, axis=0) if self.rank == 0 else None

    def close(self) -> None:
        if getattr(self, "_h", None):
            N.call("heat2d_solver_free", self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class LoopbackGroup:
    """P slabs of one domain on a single device (or host), exchanging halos
    through the native loopback transport.

    Every member is a full native solver with its own compute / comm streams,
    split plans and autotuner — one rank of a multi-GPU run — and the halo
    messages are the ones the RCCL transport sends (whole padded rows, shared
    ``halo_msgs`` plan), copied device-to-device and ordered by events. So the
    overlapped multi-rank schedule (both split orders, balanced depths) runs
    with real exchanges on one GPU; results must be bitwise identical to P = 1.
    """

    def __init__(self, problem: Problem, nranks: int, *, dtype: str = "fp64", backend: str = "auto",
                 tb: int = 0, tile_rows: int = 0, device: Optional[int] = None, arith: str = "auto",
                 overlap: bool = True, autotune: int = -1, comm_cus: int = 0, edge_shift: int = 0,
                 bc_x: str = "dirichlet", bc_y: str = "dirichlet", source=None, rmap=None, faces=None,
                 probes=None, probe_steps: Optional[int] = None, source_gain=None, robin=None, weights=None):
        self.problem = problem
        self.bc_x, self.bc_y = bc_x, bc_y
        self.arith = arith
        self.weights = None
        if weights is not None:  # the five-weight operator (HeatSolver weights=); refused before anything is built
            _check_weights(weights, NP_DTYPES[DTYPES[dtype]], arith=arith, bc_x=bc_x, bc_y=bc_y, source=source, rmap=rmap,
                           faces=faces, source_gain=source_gain)
        self.backend = resolve_backend(backend)
        self.dtype = DTYPES[dtype]
        if self.backend == "hip" and device is None:
            import torch
            device = torch.cuda.current_device()
        cfg = N.Config()
        cfg.n_rows = problem.n_owned
        cfg.n_cols = problem.n_owned
        cfg.dtype = self.dtype
        cfg.backend = N.BACKEND_HIP if self.backend == "hip" else N.BACKEND_CPU
        cfg.r = problem.r
        cfg.tb = tb
        cfg.overlap = int(overlap)
        cfg.autotune = autotune
        cfg.comm_cus = comm_cus
        cfg.device = -1 if device is None else int(device)
        cfg.tile_rows = tile_rows
        cfg.arith = N.ARITH[arith]
        cfg.edge_shift = int(edge_shift)
        cfg.bc_x = N.bc_code(bc_x, "bc_x")
        cfg.bc_y = N.bc_code(bc_y, "bc_y")
        self.robin = _set_robin(cfg, robin, bc_x, bc_y, NP_DTYPES[self.dtype])  # Robin walls (HeatSolver robin=)
        cfg.source = int(source is not None)  # a heat source (HeatSolver source=): each member slices its rows
        cfg.rmap = int(rmap is not None)  # a diffusivity map (HeatSolver rmap=): likewise
        cfg.faces = int(faces is not None)  # face coefficients (HeatSolver faces=): likewise
        self.nranks = nranks
        h = C.c_void_p()
        N.call("heat2d_group_create", C.byref(cfg), nranks, C.byref(h))
        self._h = h
        if source is not None:
            self.set_source(source)
        if source_gain is not None:
            self.set_source_gain(source_gain)
        if rmap is not None:
            self.set_rmap(rmap)
        if faces is not None:
            self.set_faces(faces)
        if weights is not None:
            self.set_weights(weights)
        self._nprobes = 0
        if probes is not None:
            self.set_probes(probes, probe_steps)
        x = np.ascontiguousarray(problem.x, dtype=np.float64)
        ic = problem.ic.to_native()
        N.call("heat2d_group_init", self._h, C.byref(ic), x.ctypes.data_as(C.c_void_p),
               x.ctypes.data_as(C.c_void_p))

    def step(self, n: int) -> None:
        N.call("heat2d_group_step", self._h, int(n))

    def set_source(self, source) -> None:
        """Replace (the global frame-inclusive array) or clear (None) the heat
        source of every member, between step() calls (HeatSolver.set_source)."""
        if source is None:
            N.call("heat2d_group_set_source", self._h, None, 0)
            return
        m = self.problem.n_owned
        a = _source_array(source, m, m, NP_DTYPES[self.dtype])
        N.call("heat2d_group_set_source", self._h, a.ctypes.data_as(C.c_void_p), m + 2)

    def set_source_gain(self, source_gain, start: int = 0) -> None:
        """The source's gain schedule on every member (HeatSolver.set_source_gain):
        each takes the whole schedule, nothing is exchanged. None clears it."""
        if source_gain is None:
            N.call("heat2d_group_set_source_gain", self._h, None, 0, 0)
            return
        a = _gain_array(source_gain, NP_DTYPES[self.dtype])
        if not 0 <= int(start) <= a.size:
            raise ValueError(f"start must be in [0, {a.size}], got {start}")
        N.call("heat2d_group_set_source_gain", self._h, a.ctypes.data_as(C.c_void_p), a.size, int(start))

    def gain_info(self, i: int = 0) -> dict:
        """info()["source_gain"] of member i."""
        return _gain_info(self._member(i))

    def set_rmap(self, rmap) -> None:
        """Replace (the global frame-inclusive array) or drop (None) the
        diffusivity map of every member, between step() calls (HeatSolver.set_rmap)."""
        if rmap is None:
            N.call("heat2d_group_set_rmap", self._h, None, 0)
            return
        m = self.problem.n_owned
        a = _rmap_array(rmap, m, m, NP_DTYPES[self.dtype])
        N.call("heat2d_group_set_rmap", self._h, a.ctypes.data_as(C.c_void_p), m + 2)

    def set_faces(self, faces) -> None:
        """Replace (the pair of global frame-inclusive arrays) or drop (None) the
        face coefficients of every member, between step() calls (HeatSolver.set_faces)."""
        if faces is None:
            N.call("heat2d_group_set_faces", self._h, None, None, 0)
            return
        m = self.problem.n_owned
        rx, ry = _faces_arrays(faces, m, m, NP_DTYPES[self.dtype])
        N.call("heat2d_group_set_faces", self._h, rx.ctypes.data_as(C.c_void_p), ry.ctypes.data_as(C.c_void_p), m + 2)

    def set_weights(self, weights) -> None:
        """The five weights on every member, or None to drop them (HeatSolver.set_weights)."""
        if weights is None:
            N.call("heat2d_group_set_weights", self._h, None)
            self.weights = None
            return
        arr, w = _check_weights(weights, NP_DTYPES[self.dtype], arith=self.arith, bc_x=self.bc_x, bc_y=self.bc_y)
        N.call("heat2d_group_set_weights", self._h, arr)
        self.weights = w

    def weights_info(self, i: int = 0) -> dict:
        """info()["weights"] of member i."""
        return _weights_info(self._member(i))

    def set_probes(self, points, steps: Optional[int] = None) -> None:
        """Probe points on every member (HeatSolver.set_probes; the global list:
        each member keeps the points of its rows). None clears them."""
        if points is None:
            N.call("heat2d_group_set_probes", self._h, None, 0, 0)
            self._nprobes = 0
            return
        m = self.problem.n_owned
        a = K.probe_points(points, m, m)
        cap = int(self.problem.ntime if steps is None else steps)
        if len(a) and cap < 1:
            raise ValueError(f"probe_steps must be at least 1, got {cap}")
        N.call("heat2d_group_set_probes", self._h, a.ctypes.data_as(C.c_void_p), len(a), cap)
        self._nprobes = len(a)

    def probe_history(self) -> np.ndarray:
        """The members' histories merged: (recorded, P), columns in the order of
        the list set_probes was given."""
        out = None
        for i in range(self.nranks):
            h = self._member(i)
            v = (C.c_int64 * 4)()
            N.call("heat2d_solver_probes", h, v)
            cnt, rec = int(v[0]), int(v[2])
            if out is None:
                out = np.empty((rec, self._nprobes), dtype=NP_DTYPES[self.dtype])
            if cnt == 0 or rec == 0:
                continue
            idx = (C.c_int64 * cnt)()
            N.call("heat2d_solver_probe_index", h, idx)
            part = np.empty((rec, cnt), dtype=NP_DTYPES[self.dtype])
            N.call("heat2d_solver_probe_history", h, part.ctypes.data_as(C.c_void_p))
            out[:, list(idx)] = part
        return out

    def upload(self, arr: np.ndarray) -> None:
        """Whole owned grid -> the members' slabs, then a loopback halo exchange."""
        m = self.problem.n_owned
        a = np.ascontiguousarray(arr, dtype=NP_DTYPES[self.dtype])
        if a.shape == (m + 2, m + 2):  # frame-inclusive (HeatSolver.upload)
            N.call("heat2d_group_upload_field", self._h, a.ctypes.data_as(C.c_void_p), m + 2)
            return
        if a.shape != (m, m):
            raise ValueError(f"expected {(m, m)} (or the frame-inclusive {(m + 2, m + 2)}), got {a.shape}")
        N.call("heat2d_group_upload", self._h, a.ctypes.data_as(C.c_void_p), m)

    def download(self) -> np.ndarray:
        m = self.problem.n_owned
        out = np.empty((m, m), dtype=NP_DTYPES[self.dtype])
        N.call("heat2d_group_download", self._h, out.ctypes.data_as(C.c_void_p), m)
        return out

    def _member(self, i: int):
        h = C.c_void_p()
        N.call("heat2d_group_member", self._h, int(i), C.byref(h))
        return h

    def slabs(self) -> list:
        """(row0, nrows) of every member's slab."""
        out = []
        for i in range(self.nranks):
            L = N.Layout()
            N.call("heat2d_solver_layout", self._member(i), C.byref(L))
            out.append((int(L.row0), int(L.nrows)))
        return out

    def plan(self, i: int, k: int) -> dict:
        """Member i's split plan for depth k (as HeatSolver.plan)."""
        return _plan(self._member(i), k)

    def cycle_hist(self, i: int, reset: bool = False) -> dict:
        return _cycle_hist(self._member(i), reset)

    def robin_info(self, i: int = 0) -> dict:
        """info()["robin"] of member i."""
        return _robin_info(self._member(i), self.bc_x, self.bc_y)

    def arith_code(self, i: int) -> int:
        """The arithmetic form member i runs ("auto" resolved; as HeatSolver.info()["arith"])."""
        return _arith(self._member(i))

    def close(self) -> None:
        if getattr(self, "_h", None):
            N.call("heat2d_group_free", self._h)
            self._h = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass
