"""NumPy golden models (the test oracle; no native code).

* :func:`initial_field` / :func:`ftcs` — the frame-inclusive FTCS solver in the
  reference's exact arithmetic order ``c + r*((((S + E) + N) + W) - 4c)``
  (fortran/hip/heat_kernel.cpp:43, fortran/serial/heat.f90:66). The native
  engine (any K, any P, CPU or GPU) must match it **bitwise**.
* :func:`python_serial_demo` — python/serial/heat.py as written (31x31, index-slice
  hat, ``diffuse(10)`` = 11 steps, its own update formula).
* :func:`eigenmode` — closed form of FTCS on a zero-Dirichlet sine mode:
  ``T_m = g^m T_0``, ``g = 1 - 4r(sin^2(k pi d/2L) + sin^2(l pi d/2L))``.
"""
from __future__ import annotations

import numpy as np

from ..utils.config import (IC_BOX, IC_CONST, IC_INDEX_BOX, IC_SINE, IC_UNIFORM, IcSpec, Problem)


def initial_field(problem: Problem, dtype=np.float64) -> np.ndarray:
    """Frame-inclusive (m+2)x(m+2) initial field (row = x index, column = y index)."""
    x = problem.x
    m = problem.n_owned
    ic: IcSpec = problem.ic
    X = x[:, None]
    Y = x[None, :]
    frame = np.zeros((m + 2, m + 2), dtype=bool)
    frame[0, :] = frame[-1, :] = frame[:, 0] = frame[:, -1] = True
    if ic.kind == IC_UNIFORM:
        T = np.where(frame, ic.b, ic.a)
    elif ic.kind == IC_BOX:
        inside = (X <= ic.x1) & (X >= ic.x0) & (Y <= ic.y1) & (Y >= ic.y0)
        T = np.where(inside, ic.a, ic.b)
    elif ic.kind == IC_INDEX_BOX:
        gi = np.arange(m + 2)[:, None]
        gj = np.arange(m + 2)[None, :]
        inside = (gi >= ic.i0) & (gi < ic.i1) & (gj >= ic.j0) & (gj < ic.j1)
        T = np.where(inside, ic.a, ic.b)
    elif ic.kind == IC_SINE:
        T = ic.a * np.sin(ic.kx * np.pi * (X - ic.x0) / (ic.x1 - ic.x0)) * \
            np.sin(ic.ky * np.pi * (Y - ic.y0) / (ic.y1 - ic.y0))
        T = np.where(frame, 0.0, T)
    elif ic.kind == IC_CONST:
        T = np.full((m + 2, m + 2), ic.a)
    else:
        raise ValueError(ic.kind)
    return np.ascontiguousarray(T, dtype=np.float64).astype(dtype)


_PAD_MODE = {"periodic": "wrap", "insulated": "edge"}
_ROBIN_SIDES = {"bc_x": ("x_lo", "x_hi"), "bc_y": ("y_lo", "y_hi")}


def robin_pairs(robin, bc_x: str, bc_y: str, dtype) -> dict:
    """The (a, b) pairs of the Robin sides, checked and converted to ``dtype``:
    ``robin`` maps exactly the sides of the axes that are "robin" ("x_lo" /
    "x_hi": the wall before the first / after the last owned row, "y_lo" /
    "y_hi": the same for columns) to a finite pair. A missing or surplus key,
    or an entry that is not finite, raises ValueError."""
    want = [k for name, bc in (("bc_x", bc_x), ("bc_y", bc_y)) if bc == "robin" for k in _ROBIN_SIDES[name]]
    have = {} if robin is None else dict(robin)
    missing = [k for k in want if k not in have]
    surplus = sorted(k for k in have if k not in want)
    if missing:
        raise ValueError(f"robin= lacks the pair of {', '.join(missing)} (every side of a \"robin\" axis needs one)")
    if surplus:
        raise ValueError(f"robin= has a pair for {', '.join(map(str, surplus))}, which is no side of a \"robin\" axis")
    t = np.dtype(dtype).type
    out = {}
    for k in want:
        try:
            a, b = have[k]
        except (TypeError, ValueError):
            raise ValueError(f"robin[{k!r}] must be a pair (a, b)") from None
        with np.errstate(over="ignore"):
            a, b = t(a), t(b)
        if not (np.isfinite(a) and np.isfinite(b)):
            raise ValueError(f"robin[{k!r}] must be finite in the run's dtype, got ({a}, {b})")
        out[k] = (a, b)
    return out


def robin_ghost(C: np.ndarray, a, b, arith: str = "exact") -> np.ndarray:
    """The value beyond a Robin wall from the adjacent owned points C:
    exact: a * C + b (the product rounded, then the add); fma: one rounding."""
    t = C.dtype.type
    if arith == "fma":
        a, b = t(a), t(b)
        g = fma(np.broadcast_to(a, C.shape), C, np.broadcast_to(b, C.shape))
        # :func:`fma` emulates the normal range and returns +0.0 for every zero; a hardware fma returns -0.0
        # where the product and the addend are both negative zeros (so that (1, -0.0) keeps a -0.0)
        neg = (g == 0) & (b == 0) & np.signbit(b) & ((C == 0) | (a == 0)) & (np.signbit(C) ^ np.signbit(a))
        return np.where(neg, t(-0.0), g).astype(C.dtype, copy=False)
    if arith != "exact":
        raise ValueError("a Robin wall needs arith 'exact' or 'fma'")
    return t(a) * C + t(b)


def _pad_axis(out: np.ndarray, axis: int, bc: str, lo, hi, arith: str) -> np.ndarray:
    if bc != "robin":
        return np.pad(out, ((1, 1), (0, 0)) if axis == 0 else ((0, 0), (1, 1)), mode=_PAD_MODE[bc])
    first, last = (out[:1], out[-1:]) if axis == 0 else (out[:, :1], out[:, -1:])
    return np.concatenate([robin_ghost(first, *lo, arith), out, robin_ghost(last, *hi, arith)], axis=axis)


def wrap_frame(T: np.ndarray, bc_x: str = "dirichlet", bc_y: str = "dirichlet", robin=None,
               arith: str = "exact") -> np.ndarray:
    """The frame-inclusive field with its frame entries on periodic axes
    replaced by wrap images of the owned points (``np.pad(mode="wrap")``) and on
    insulated axes by images of the adjacent owned point (``mode="edge"``: the
    wall sits half a cell outside the first and last owned point, T[0] = T[1],
    T[n+1] = T[n]). With only y periodic / insulated the Dirichlet frame rows
    get images at their ends too: the point (0, -1) reads (-1, -1) / (0, 0).
    x is padded first, then y over the padded rows. Dirichlet on both axes: T
    itself.
    "robin" (with ``robin=``, :func:`robin_pairs`): the insulated geometry with
    the affine ghost value G = a * C + b of the adjacent owned point C in place
    of its image, formed in the form ``arith`` names (:func:`robin_ghost`);
    x first, then y over the filled rows, so the corner entries are the y ghost
    of the x ghost (no owned point reads them)."""
    for name, bc in (("bc_x", bc_x), ("bc_y", bc_y)):
        if bc not in ("dirichlet", "periodic", "insulated", "robin"):
            raise ValueError(f"{name} must be 'dirichlet', 'periodic', 'insulated' or 'robin', got {bc!r}")
    rb = robin_pairs(robin, bc_x, bc_y, T.dtype)
    px, py = bc_x != "dirichlet", bc_y != "dirichlet"
    if not (px or py):
        return T
    out = T[(1 if px else 0):(-1 if px else None), (1 if py else 0):(-1 if py else None)]
    if px:
        out = _pad_axis(out, 0, bc_x, rb.get("x_lo"), rb.get("x_hi"), arith)
    if py:
        out = _pad_axis(out, 1, bc_y, rb.get("y_lo"), rb.get("y_hi"), arith)
    return out


def _two_sum(a, b):
    """s + e == a + b exactly (Knuth), s the rounded sum."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _sum_round_odd(a, b):
    """a + b rounded to odd (float64): the rounded sum, moved to its odd
    neighbour on the side of the exact sum when it is inexact and even. A
    value rounded to odd rounds again, to nearest at a precision at least two
    bits shorter, as the exact value would (Boldo & Melquiond, "Emulation of
    FMA and correctly rounded sums", 2008)."""
    s, e = _two_sum(a, b)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where((e != 0) & even, np.nextafter(s, toward), s)


def fma(a, b, c):
    """Elementwise fused multiply-add a * b + c with ONE rounding, in the arrays'
    dtype (float32 or float64), for the normal range the golden runs in: what
    the engine's contracted arithmetic ("fma") executes. float32: the product
    is exact in float64, the sum rounded to odd there, then to float32.
    float64: the product split exactly (Veltkamp / Dekker), then Boldo &
    Melquiond's emulation RN(th + RO(tl + ul))."""
    a, b, c = np.broadcast_arrays(np.asarray(a), np.asarray(b), np.asarray(c))
    if a.dtype == np.float32:
        p = a.astype(np.float64) * b.astype(np.float64)
        return _sum_round_odd(p, c.astype(np.float64)).astype(np.float32)
    if a.dtype != np.float64:
        raise TypeError("fma: float32 or float64 arrays")
    uh = a * b
    k = np.float64(134217729.0)  # 2^27 + 1
    t = k * a
    ah = t - (t - a)
    al = a - ah
    t = k * b
    bh = t - (t - b)
    bl = b - bh
    ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl  # a * b == uh + ul
    th, tl = _two_sum(c, uh)
    return th + _sum_round_odd(tl, ul)


def _ftcs_step_source(T: np.ndarray, r, arith: str, source: np.ndarray, gain=None) -> np.ndarray:
    """One step with a heat source: the update of :func:`ftcs_step`, rounded as
    it is there, then one separately rounded add of the source,
        exact: T' = (C + r*((((S_+E)+N)+W) - 4C)) + S[i,j]
        fma:   T' = fma(r, fma(-4, C, sum), C)    + S[i,j]
    at the owned points; the frame stays pinned and the frame entries of
    ``source`` are ignored.
    gain (a scalar g, finite and >= 0, converted to the field's dtype): the step
    of a time-dependent source g(t) * S,
        exact: T' = upd + (g * S[i,j])      (the product rounded, then the add)
        fma:   T' = fma(g, S[i,j], upd)     (one rounding)
    g == 1 gives the bits of the source alone in both forms. None: no gain."""
    if arith not in ("exact", "fma"):
        raise ValueError("a heat source needs arith 'exact' or 'fma'")
    if source.shape != T.shape:
        raise ValueError(f"source must be frame-inclusive like the field, {T.shape}, got {source.shape}")
    S = np.ascontiguousarray(source, dtype=T.dtype)
    r = T.dtype.type(r)
    four = T.dtype.type(4)
    c = T[1:-1, 1:-1]
    total = ((T[2:, 1:-1] + T[1:-1, 2:]) + T[:-2, 1:-1]) + T[1:-1, :-2]
    out = T.copy()
    if arith == "fma":
        upd = fma(np.broadcast_to(r, c.shape), fma(np.broadcast_to(-four, c.shape), c, total), c)
    else:
        upd = c + r * (total - four * c)
    if gain is None:
        out[1:-1, 1:-1] = upd + S[1:-1, 1:-1]
        return out
    g = T.dtype.type(gain)
    if not (np.isfinite(g) and g >= 0):
        raise ValueError("a source gain must be finite and >= 0 (put the sign into the source)")
    if arith == "fma":
        out[1:-1, 1:-1] = fma(np.broadcast_to(g, c.shape), S[1:-1, 1:-1], upd)
    else:
        out[1:-1, 1:-1] = upd + g * S[1:-1, 1:-1]
    return out


def _ftcs_step_rmap(T: np.ndarray, arith: str, rmap: np.ndarray) -> np.ndarray:
    """One step with a diffusivity map (u_t = nu(x, y) lap(u), the
    non-divergence form): the scalar r of :func:`ftcs_step` replaced by the
    map's element at every owned point, in the reference's operand order,
        exact: T' = C + R[i,j] * ((((S_+E)+N)+W) - 4C)
        fma:   T' = fma(R[i,j], fma(-4, C, sum), C)      (:func:`fma`: one rounding each)
    The frame stays pinned and the frame entries of ``rmap`` are ignored;
    R[i,j] == 0 holds the point at its value."""
    if arith not in ("exact", "fma"):
        raise ValueError("a diffusivity map needs arith 'exact' or 'fma' (jacobi assumes r == 1/4 everywhere)")
    if rmap.shape != T.shape:
        raise ValueError(f"rmap must be frame-inclusive like the field, {T.shape}, got {rmap.shape}")
    R = np.ascontiguousarray(rmap, dtype=T.dtype)[1:-1, 1:-1]
    four = T.dtype.type(4)
    c = T[1:-1, 1:-1]
    total = ((T[2:, 1:-1] + T[1:-1, 2:]) + T[:-2, 1:-1]) + T[1:-1, :-2]
    out = T.copy()
    if arith == "fma":
        out[1:-1, 1:-1] = fma(R, fma(np.broadcast_to(-four, c.shape), c, total), c)
    else:
        out[1:-1, 1:-1] = c + R * (total - four * c)
    return out


def _ftcs_step_faces(T: np.ndarray, arith: str, faces) -> np.ndarray:
    """One step of the conservative (divergence) form u_t = div(k grad u) from
    per-face diffusion numbers ``faces = (RX, RY)``, two frame-inclusive arrays
    already multiplied by dt / dx^2: RX[i,j] is the face between (i,j) and
    (i,j+1) (used for j = 0..n), RY[i,j] the face between (i,j) and (i+1,j)
    (used for i = 0..n). At every owned point, operands in the march's order
    S, E, N, W,
        exact: T' = C + (((RY[i,j]*(S-C) + RX[i,j]*(E-C)) + RY[i-1,j]*(N-C)) + RX[i,j-1]*(W-C))
        fma:   p = RY[i,j]*(S-C); p = fma(RX[i,j], E-C, p); p = fma(RY[i-1,j], N-C, p);
               p = fma(RX[i,j-1], W-C, p); T' = C + p     (:func:`fma`: one rounding each)
    The frame stays pinned. The product a face contributes to a point is the
    exact negative of the one it contributes to the neighbour (E-C and C-E
    differ in sign only), so what leaves one cell enters the other; a zero
    face is a wall, and a point whose four faces are zero keeps its bits."""
    if arith not in ("exact", "fma"):
        raise ValueError("face coefficients need arith 'exact' or 'fma' (jacobi assumes one r == 1/4)")
    RX, RY = faces
    if RX.shape != T.shape or RY.shape != T.shape:
        raise ValueError(f"faces must be two frame-inclusive arrays like the field, {T.shape}, got {RX.shape} and {RY.shape}")
    RX = np.ascontiguousarray(RX, dtype=T.dtype)
    RY = np.ascontiguousarray(RY, dtype=T.dtype)
    c = T[1:-1, 1:-1]
    ds, de, dn, dw = T[2:, 1:-1] - c, T[1:-1, 2:] - c, T[:-2, 1:-1] - c, T[1:-1, :-2] - c
    ys, xe, yn, xw = RY[1:-1, 1:-1], RX[1:-1, 1:-1], RY[:-2, 1:-1], RX[1:-1, :-2]
    out = T.copy()
    if arith == "fma":
        out[1:-1, 1:-1] = c + fma(xw, dw, fma(yn, dn, fma(xe, de, ys * ds)))
    else:
        out[1:-1, 1:-1] = c + (((ys * ds + xe * de) + yn * dn) + xw * dw)
    return out


def weights_tuple(weights, dtype) -> tuple:
    """``weights`` = (wS, wE, wN, wW, wC) checked and converted to ``dtype``: five
    entries, each finite in the run's dtype. ValueError otherwise."""
    try:
        w = [x for x in weights]
    except TypeError:
        raise ValueError("weights must be a 5-tuple (wS, wE, wN, wW, wC)") from None
    if len(w) != 5:
        raise ValueError(f"weights must be a 5-tuple (wS, wE, wN, wW, wC), got {len(w)} entries")
    t = np.dtype(dtype).type
    with np.errstate(over="ignore"):
        w = tuple(t(x) for x in w)
    if not all(np.isfinite(x) for x in w):
        raise ValueError(f"weights must be finite in the run's dtype, got {w}")
    return w


def _ftcs_step_weights(T: np.ndarray, arith: str, weights, bc_x: str, bc_y: str) -> np.ndarray:
    """One step of the constant-coefficient five-point operator
    T' = wS*S + wE*E + wN*N + wW*W + wC*C (a moving medium, unequal diffusion
    numbers on the two axes, a linear loss: ``heat2d.weights_from``), operands in
    the march's order, every product and sum rounded,
        exact: T' = ((((wS*S + wE*E) + wN*N) + wW*W) + wC*C)
        fma:   p = wS*S; p = fma(wE,E,p); p = fma(wN,N,p); p = fma(wW,W,p); T' = fma(wC,C,p)
    (:func:`fma`: one rounding each). Axes "dirichlet" (frame pinned) or
    "periodic" (:func:`wrap_frame` before the step); ``r`` is not used."""
    if arith not in ("exact", "fma"):
        raise ValueError("weights need arith 'exact' or 'fma' (jacobi / fast assume one r)")
    for name, bc in (("bc_x", bc_x), ("bc_y", bc_y)):
        if bc not in ("dirichlet", "periodic"):
            raise ValueError(f"weights need 'dirichlet' or 'periodic' axes, got {name}={bc!r}")
    wS, wE, wN, wW, wC = weights_tuple(weights, T.dtype)
    T = wrap_frame(T, bc_x, bc_y)
    c, s, e, n, w = T[1:-1, 1:-1], T[2:, 1:-1], T[1:-1, 2:], T[:-2, 1:-1], T[1:-1, :-2]
    out = T.copy()
    if arith == "fma":
        b = lambda x: np.broadcast_to(x, c.shape)  # noqa: E731
        out[1:-1, 1:-1] = fma(b(wC), c, fma(b(wW), w, fma(b(wN), n, fma(b(wE), e, wS * s))))
    else:
        out[1:-1, 1:-1] = (((wS * s + wE * e) + wN * n) + wW * w) + wC * c
    return out


def ftcs_step(T: np.ndarray, r, arith: str = "exact", bc_x: str = "dirichlet", bc_y: str = "dirichlet",
              source: np.ndarray | None = None, rmap: np.ndarray | None = None, faces=None, gain=None,
              robin=None, weights=None) -> np.ndarray:
    """One FTCS step of a frame-inclusive field. On a Dirichlet axis the frame
    is kept fixed; on a periodic or insulated one it is refreshed from the
    owned points before the step (:func:`wrap_frame`) — the update and its
    operation order are the same — and holds the images of T at time t on
    return.
    arith "jacobi" (r == 1/4 only): r * sum, the zero centre weight folded
    away — the engine's arith 2.
    source (frame-inclusive, the per-step increment S = dt * f; Dirichlet axes,
    arith "exact" or "fma"): added after the update as an operation of its own
    (:func:`_ftcs_step_source`). None: no source.
    An asymmetry to know: WITH a source, "fma" is the contracted update with a
    single rounding (:func:`fma`), what the engine's arith 1 executes; WITHOUT
    one, "fma" keeps taking the exact expression as it always has here (equal
    bits only where r is a power of two). So at such an r as 0.2,
    ``ftcs(arith="fma", source=None)`` and ``ftcs(arith="fma", source=<all -0.0>)``
    differ, while with "exact" they are bitwise equal.
    faces ((RX, RY), per-face diffusion numbers; Dirichlet axes, arith "exact" or
    "fma", no source, no rmap): the conservative form (:func:`_ftcs_step_faces`);
    ``r`` is then not used. None: today's function.
    gain (with source=): this step's gain of a time-dependent source
    (:func:`_ftcs_step_source`). None: the source as it is.
    robin (the pairs of the "robin" axes, :func:`robin_pairs`; arith "exact" or
    "fma"): before the step the frame entry next to an owned point C on a Robin
    side is set to the ghost value a * C + b ("fma": fma(a, C, b)), then the
    unchanged update runs — with a Robin axis "fma" is the contracted update
    with a single rounding, fma(r, fma(-4, C, sum), C), as with a source.
    weights ((wS, wE, wN, wW, wC); "dirichlet" or "periodic" axes, arith "exact" or
    "fma", none of source / rmap / faces / gain / robin): the five-weight operator
    (:func:`_ftcs_step_weights`); ``r`` is then not used. None: today's function."""
    if weights is not None:
        if source is not None or rmap is not None or faces is not None or gain is not None or robin is not None:
            raise ValueError("weights together with source=, rmap=, faces=, a gain or robin= are not offered")
        return _ftcs_step_weights(T, arith, weights, bc_x, bc_y)
    has_robin = bc_x == "robin" or bc_y == "robin"
    if has_robin and arith not in ("exact", "fma"):
        raise ValueError("a Robin wall needs arith 'exact' or 'fma' (the scaled levels of jacobi / fast would need b scaled per level)")
    if gain is not None and source is None:
        raise ValueError("gain= scales a heat source: pass source=")
    if faces is not None:
        if rmap is not None or source is not None:
            raise ValueError("face coefficients together with rmap= or source= are not offered")
        if bc_x != "dirichlet" or bc_y != "dirichlet":
            raise ValueError("face coefficients need Dirichlet boundaries on both axes")
        return _ftcs_step_faces(T, arith, faces)
    if rmap is not None:
        # rmap (frame-inclusive, the per-point diffusion number; Dirichlet axes, arith "exact" or
        # "fma", no source): replaces r (:func:`_ftcs_step_rmap`). None: today's function.
        if bc_x != "dirichlet" or bc_y != "dirichlet":
            raise ValueError("a diffusivity map needs Dirichlet boundaries on both axes")
        if source is not None:
            raise ValueError("a diffusivity map and a heat source together are not offered")
        return _ftcs_step_rmap(T, arith, rmap)
    if source is not None:
        if bc_x != "dirichlet" or bc_y != "dirichlet":
            raise ValueError("a heat source needs Dirichlet boundaries on both axes")
        return _ftcs_step_source(T, r, arith, source, gain)
    T = wrap_frame(T, bc_x, bc_y, robin, arith if has_robin else "exact")
    r = T.dtype.type(r)
    four = T.dtype.type(4)
    c = T[1:-1, 1:-1]
    south = T[2:, 1:-1]   # x+1
    east = T[1:-1, 2:]    # y+1
    north = T[:-2, 1:-1]  # x-1
    west = T[1:-1, :-2]   # y-1
    out = T.copy()
    if arith == "jacobi":
        if r != 0.25:
            raise ValueError("arith 'jacobi' needs r == 1/4")
        out[1:-1, 1:-1] = r * (((south + east) + north) + west)
    elif has_robin and arith == "fma":
        total = ((south + east) + north) + west
        out[1:-1, 1:-1] = fma(np.broadcast_to(r, c.shape), fma(np.broadcast_to(-four, c.shape), c, total), c)
    else:
        out[1:-1, 1:-1] = c + r * ((((south + east) + north) + west) - four * c)
    return out


def ftcs(problem: Problem, nsteps: int | None = None, dtype=np.float64, T0: np.ndarray | None = None,
         arith: str = "exact", bc_x: str = "dirichlet", bc_y: str = "dirichlet",
         source: np.ndarray | None = None, rmap: np.ndarray | None = None, faces=None,
         source_gain=None, gain_start: int = 0, robin=None, weights=None) -> np.ndarray:
    """Run FTCS; returns the frame-inclusive field (frame entries on periodic
    / insulated axes: wrap / edge images of the returned owned points; on Robin
    axes their ghost values).
    robin: the pairs of the "robin" axes (:func:`ftcs_step`).
    source: a heat source added at every step (:func:`ftcs_step`).
    rmap: a diffusivity map in place of problem.r (:func:`ftcs_step`).
    faces: (RX, RY) per-face diffusion numbers, the conservative form (:func:`ftcs_step`).
    source_gain (with source=): a 1-D array G of per-step gains, the separable
    time-dependent source G[q] * S; step q of this run takes G[gain_start + q]
    (:func:`ftcs_step` gain=)."""
    T = initial_field(problem, dtype) if T0 is None else T0.astype(dtype)
    n = problem.ntime if nsteps is None else nsteps
    if weights is not None:  # the five-weight operator (:func:`ftcs_step`); problem.r is not used
        if source is not None or rmap is not None or faces is not None or source_gain is not None or robin is not None:
            raise ValueError("weights together with source=, rmap=, faces=, source_gain= or robin= are not offered")
        for _ in range(n):
            T = ftcs_step(T, problem.r, arith, bc_x, bc_y, weights=weights)
        return wrap_frame(T, bc_x, bc_y)
    if source_gain is not None:
        G = _gain_array(source_gain, T.dtype, source, gain_start, n)
        for q in range(n):
            T = ftcs_step(T, problem.r, arith, bc_x, bc_y, source, rmap, faces, gain=G[gain_start + q])
        return T
    if faces is not None:
        for _ in range(n):
            T = ftcs_step(T, problem.r, arith, bc_x, bc_y, source, rmap, faces)
        return T
    if rmap is not None:
        for _ in range(n):
            T = ftcs_step(T, problem.r, arith, bc_x, bc_y, source, rmap)
        return T
    if source is not None:
        for _ in range(n):
            T = ftcs_step(T, problem.r, arith, bc_x, bc_y, source)
        return T
    has_robin = bc_x == "robin" or bc_y == "robin"
    for _ in range(n):
        T = ftcs_step(T, problem.r, arith, bc_x, bc_y, robin=robin)
    return wrap_frame(T, bc_x, bc_y, robin, arith if has_robin else "exact")


def _gain_array(source_gain, dtype, source, start: int, nsteps: int) -> np.ndarray:
    """The schedule in the run's dtype, checked: 1-D, non-empty, finite, >= 0,
    with a source, and long enough for nsteps steps from ``start``."""
    if source is None:
        raise ValueError("source_gain= scales a heat source: pass source=")
    G = np.asarray(source_gain, dtype=dtype)
    if G.ndim != 1 or G.size == 0:
        raise ValueError("source_gain must be a non-empty 1-D array")
    if not (np.isfinite(G).all() and (G >= 0).all()):
        raise ValueError("source_gain entries must be finite and >= 0 (put the sign into the source)")
    if start < 0 or start + nsteps > G.size:
        raise ValueError(f"source_gain has {G.size} entries: steps {start}..{start + nsteps - 1} run past its end")
    return G


def probe_history(problem: Problem, nsteps: int, probes, dtype=np.float64, T0: np.ndarray | None = None,
                  arith: str = "exact", bc_x: str = "dirichlet", bc_y: str = "dirichlet",
                  source: np.ndarray | None = None, rmap: np.ndarray | None = None, faces=None,
                  source_gain=None, gain_start: int = 0, robin=None, weights=None) -> np.ndarray:
    """The golden of the solver's probe points: the (nsteps, P) array whose row
    q holds the values :func:`ftcs_step` leaves at ``probes`` after step q + 1.
    ``probes``: P owned points (i, j) in frame-inclusive indices, 1 <= i, j <= n,
    duplicates allowed. A thin loop over :func:`ftcs_step`, with its rules (and
    its refusals); the other arguments are :func:`ftcs`'s."""
    T = initial_field(problem, dtype) if T0 is None else T0.astype(dtype)
    p = np.asarray(probes)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError(f"probes must have shape (P, 2), got {p.shape}")
    if not np.issubdtype(p.dtype, np.integer):
        raise ValueError("probes must be integer points (i, j)")
    n, m = T.shape[0] - 2, T.shape[1] - 2
    if len(p) and (p.min() < 1 or p[:, 0].max() > n or p[:, 1].max() > m):
        raise ValueError(f"probes must be owned points (1..{n}, 1..{m})")
    H = np.empty((nsteps, len(p)), dtype=T.dtype)
    if weights is not None and source_gain is not None:
        raise ValueError("weights together with source_gain= are not offered")
    G = None if source_gain is None else _gain_array(source_gain, T.dtype, source, gain_start, nsteps)
    for q in range(nsteps):
        T = ftcs_step(T, problem.r, arith, bc_x, bc_y, source, rmap, faces,
                      gain=None if G is None else G[gain_start + q], robin=robin, weights=weights)
        H[q] = T[p[:, 0], p[:, 1]]
    return H


def fast_error_bound(nsteps: int, dtype, tmax: float) -> float:
    """Stated bound of the scaled-level arithmetic ("fast", the kernels' AR 3)
    against the reference rounding ("exact") after ``nsteps`` steps from a
    field with max |T0| = tmax, for r <= 1/4:

        max |T_fast - T_exact| <= 16 * nsteps * u * tmax,   u = eps / 2.

    Per step the reference form rounds ~6 times on values <= tmax (the sum,
    sum - 4c, r * (...), c + ...) and the scaled form ~5 times (sum, fma, and
    the rounded coefficient b = (1 - 4r) / r), plus 2 per pass for r^K and the
    unscaling multiply; FTCS with r <= 1/4 is non-expansive in the max norm, so
    per-step errors add up at most linearly (16 > 6 + 5 + 2 covers both)."""
    u = float(np.finfo(dtype).eps) / 2.0
    return 16.0 * nsteps * u * tmax


def owned(T: np.ndarray) -> np.ndarray:
    return T[1:-1, 1:-1]


def python_serial_demo(nx: int = 31, nt: int = 10, nu: float = 0.05, sigma: float = 0.25) -> np.ndarray:
    """python/serial/heat.py:8-58 verbatim semantics (without the plots)."""
    ny = nx
    dx = 2 / (nx - 1)
    dy = 2 / (ny - 1)
    dt = sigma * dx * dy / nu
    u = np.ones((ny, nx))
    u[int(.5 / dy):int(1 / dy + 1), int(.5 / dx):int(1 / dx + 1)] = 2
    for _ in range(nt + 1):
        un = u.copy()
        u[1:-1, 1:-1] = (un[1:-1, 1:-1] + nu * dt / dx ** 2 * (un[1:-1, 2:] - 2 * un[1:-1, 1:-1] + un[1:-1, 0:-2])
                         + nu * dt / dy ** 2 * (un[2:, 1:-1] - 2 * un[1:-1, 1:-1] + un[0:-2, 1:-1]))
        u[0, :] = 1
        u[-1, :] = 1
        u[:, 0] = 1
        u[:, -1] = 1
    return u


def eigen_factor(problem: Problem, kx: float = 1.0, ky: float = 1.0) -> float:
    """Per-step amplification g of the sine mode on the boundary-inclusive grid."""
    L = problem.x[-1] - problem.x[0]
    d = problem.delta
    return 1.0 - 4.0 * problem.r * (np.sin(kx * np.pi * d / (2 * L)) ** 2 + np.sin(ky * np.pi * d / (2 * L)) ** 2)


def periodic_eigen_factor(r: float, n: int, k: int = 1, l: int = 1) -> float:
    """Per-step amplification of the mode cos(2 pi k i / n) cos(2 pi l j / n)
    on the fully periodic n x n grid: g = 1 - 4r (sin^2(pi k / n) + sin^2(pi l / n))."""
    return 1.0 - 4.0 * r * (np.sin(np.pi * k / n) ** 2 + np.sin(np.pi * l / n) ** 2)


def periodic_eigenmode(r: float, n: int, nsteps: int, k: int = 1, l: int = 1) -> np.ndarray:
    """Closed-form FTCS solution (owned n x n points) from that mode: g^nsteps T_0."""
    i = np.arange(n)
    T0 = np.cos(2 * np.pi * k * i / n)[:, None] * np.cos(2 * np.pi * l * i / n)[None, :]
    return T0 * periodic_eigen_factor(r, n, k, l) ** nsteps


def insulated_eigen_factor(r: float, n: int, p: int = 1, q: int = 1) -> float:
    """Per-step amplification of the mode cos(p pi (i + 1/2) / n) cos(q pi (j + 1/2) / n)
    on the fully insulated n x n grid: g = 1 - 4r (sin^2(p pi / 2n) + sin^2(q pi / 2n))."""
    return 1.0 - 4.0 * r * (np.sin(np.pi * p / (2 * n)) ** 2 + np.sin(np.pi * q / (2 * n)) ** 2)


def insulated_eigenmode(r: float, n: int, nsteps: int, p: int = 1, q: int = 1) -> np.ndarray:
    """Closed-form FTCS solution (owned n x n points) from that mode: g^nsteps T_0."""
    i = np.arange(n) + 0.5
    T0 = np.cos(np.pi * p * i / n)[:, None] * np.cos(np.pi * q * i / n)[None, :]
    return T0 * insulated_eigen_factor(r, n, p, q) ** nsteps


def eigenmode(problem: Problem, nsteps: int) -> np.ndarray:
    """Closed-form FTCS solution for the `sine` IC (frame-inclusive)."""
    T0 = initial_field(problem, np.float64)
    return T0 * eigen_factor(problem, problem.ic.kx, problem.ic.ky) ** nsteps
