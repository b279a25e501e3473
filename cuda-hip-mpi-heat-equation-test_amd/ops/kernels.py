"""Raw kernel ops on PyTorch tensors (device or host), backed by the native engine.

A field is a flat 1-D tensor of ``layout.elems()`` elements laid out as
``csrc/include/heat2d/common.hpp`` describes (row-major, ``halo`` ghost rows
above/below, ``cpad`` padding columns on the left, 256-B aligned pitch). These
ops run on torch's current HIP stream, so they compose with torch code and with
stream capture. CUDA(HIP) tensors dispatch to the gfx950 kernels, CPU tensors to
the CPU twins — the results are bitwise identical.

Reference kernels replaced: ``heat_eqn`` (fortran/hip/heat_kernel.cpp:31-61) ->
:func:`tb_step`; ``swap_send`` / ``swap_recv1`` / ``swap_recv2`` (:63-150) ->
:func:`pack_rows` / :func:`unpack_rows`; the commented-out checksum
(fortran/hip/heat.F90:297-306) -> :func:`stats`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _native as N

TORCH_DTYPES = {N.F32: torch.float32, N.F64: torch.float64}


def dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return N.F32
    if t.dtype == torch.float64:
        return N.F64
    raise TypeError(f"unsupported dtype {t.dtype} (fp32 / fp64)")


def _stream(t: torch.Tensor):
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream) if t.is_cuda else None


def _check_field(t: torch.Tensor, layout: N.Layout) -> None:
    if t.dim() != 1 or not t.is_contiguous():
        raise ValueError("field must be a contiguous 1-D tensor")
    if t.numel() != layout.elems():
        raise ValueError(f"field has {t.numel()} elements, layout needs {layout.elems()}")


def make_layout(nrows: int, ncols: int, halo: int = 16, row0: int = 0,
                nrows_global: Optional[int] = None) -> N.Layout:
    return N.make_layout(nrows, ncols, halo, row0, nrows if nrows_global is None else nrows_global)


def empty_field(layout: N.Layout, dtype=torch.float64, device="cuda") -> torch.Tensor:
    return torch.empty(layout.elems(), dtype=dtype, device=device)


def view2d(field: torch.Tensor, layout: N.Layout) -> torch.Tensor:
    """(rows_alloc, pitch) view of a field (ghost rows / pad columns included)."""
    return field.view(layout.rows_alloc(), layout.pitch)


def owned(field: torch.Tensor, layout: N.Layout) -> torch.Tensor:
    """(nrows, ncols) view of the owned region."""
    v = view2d(field, layout)
    return v[layout.halo:layout.halo + layout.nrows, layout.cpad:layout.cpad + layout.ncols]


def init_field(field: torch.Tensor, layout: N.Layout, ic, xcoord: np.ndarray,
               ycoord: Optional[np.ndarray] = None) -> None:
    """Fill the whole allocation from an IC (utils.config.IcSpec). ``xcoord`` holds
    nrows_global+2 frame-inclusive x coordinates, ``ycoord`` ncols+2 (default: xcoord)."""
    _check_field(field, layout)
    ycoord = xcoord if ycoord is None else ycoord
    p = ic.to_native() if hasattr(ic, "to_native") else ic
    if field.is_cuda:
        xd = torch.as_tensor(np.ascontiguousarray(xcoord, np.float64), device=field.device)
        yd = torch.as_tensor(np.ascontiguousarray(ycoord, np.float64), device=field.device)
        N.call("heat2d_init_field", dtype_code(field), C.c_void_p(field.data_ptr()), C.byref(layout), C.byref(p),
               C.c_void_p(xd.data_ptr()), C.c_void_p(yd.data_ptr()), _stream(field))
        torch.cuda.current_stream(field.device).synchronize()  # keep xd/yd alive until done
    else:
        xh = np.ascontiguousarray(xcoord, np.float64)
        yh = np.ascontiguousarray(ycoord, np.float64)
        N.call("heat2d_cpu_init_field", dtype_code(field), C.c_void_p(field.data_ptr()), C.byref(layout),
               C.byref(p), xh.ctypes.data_as(C.c_void_p), yh.ctypes.data_as(C.c_void_p))


def _weights_args(weights, src, arith, bc_x, bc_y, others, what):
    """The raw ops' checks of ``weights=``: (5 doubles in src's dtype, arith code, bc bits)."""
    if any(o is not None for o in others):
        raise ValueError(f"{what}: weights together with source, rmap, faces, gain or robin: no kernel carries them")
    for name, bc in (("bc_x", bc_x), ("bc_y", bc_y)):
        if bc not in ("dirichlet", "periodic"):
            raise ValueError(f"{what}: weights need 'dirichlet' or 'periodic' axes, got {name}={bc!r}")
    if arith not in ("exact", "fma", "auto"):
        raise ValueError(f"{what}: weights need arith 'exact', 'fma' or 'auto' (jacobi / fast assume one r)")
    arr, _ = N.weights_array(weights, np.float32 if src.dtype == torch.float32 else np.float64)
    return arr, N.ARITH["exact"] if arith == "exact" else N.ARITH["fma"], N.bc_bits(bc_x, bc_y)


def tb_step(src: torch.Tensor, dst: torch.Tensor, layout: N.Layout, k: int, r: float,
            rows: Optional[tuple[int, int]] = None, tile_rows: int = 0, arith: str = "exact",
            bc_x: str = "dirichlet", bc_y: str = "dirichlet", source: Optional[torch.Tensor] = None,
            rmap: Optional[torch.Tensor] = None, faces: Optional[tuple] = None,
            gain: Optional[torch.Tensor] = None, gain_pos: int = 0, robin=None, weights=None) -> None:
    """dst[rows] = k FTCS steps of src (temporal-blocked kernel). The k ghost rows
    around ``rows`` must be valid in ``src``; Dirichlet rows/cols are kept.
    ``arith``: "exact" (reference rounding), "fma" (contracted update) or
    "jacobi" (r == 1/4: r * sum).
    ``bc_y="periodic"``: no column is pinned — ``src`` must hold wrap images in
    its ghost columns (:func:`wrap_cols`), and the ghost columns of the rows
    written are refreshed in ``dst``. ``bc_x="periodic"``: no row is pinned
    (the ghost rows hold wrap images: :func:`wrap_rows`). ``"insulated"`` on
    either axis: a point next to the wall takes its own value for the operand
    beyond it, at every level (``src``'s frame entries on that axis are not
    read by an owned point), and the frame images of the rows written are
    refreshed in ``dst``; not with arith "fast".
    ``source``: a heat source in the field's layout, dtype and device (the
    per-step increment, with -0.0 in every frame row / column and pad entry so
    that pinned points keep their bits: :func:`source_field`), added at every
    fused level as an operation of its own; Dirichlet axes, arith "exact" /
    "fma" / "auto"; on the device k is at most the source kernels' deepest pass
    (common.hpp ``kMaxTBSrc``, reported as ``HeatSolver.info()["source"]["max_tb"]``).
    ``rmap``: a diffusivity map in the field's layout, dtype and device (the
    per-point diffusion number, with +0.0 in every frame row / column, pad
    entry and row outside the grid — the pinning: :func:`rmap_field`), the
    multiplier of every point's update at every fused level; ``r`` is then not
    used. Dirichlet axes, arith "exact" / "fma" ("auto" is exact), no
    ``source``; on the device k is at most ``kMaxTBVar``
    (``HeatSolver.info()["rmap"]["max_tb"]``).
    ``faces``: ``(rx, ry)``, the per-face diffusion numbers of the conservative
    form div(k grad u) in the field's layout, dtype and device
    (:func:`faces_field`); ``r`` is then not used. Dirichlet axes, arith
    "exact" / "fma" ("auto" is exact), no ``source`` and no ``rmap``; on the
    device k is at most ``kMaxTBDiv`` (``HeatSolver.info()["faces"]["max_tb"]``).
    ``gain`` (with ``source``): a 1-D tensor of per-step gains in the field's
    dtype and device, finite and >= 0; level s of the pass adds
    ``gain[gain_pos + s - 1] * source`` — the product rounded, then the add;
    arith "fma": one fma (csrc/kernels/tb_impl.hpp ``tb_kernel_gain``). It must
    hold at least ``gain_pos + k`` entries.
    ``"robin"`` on either axis, with ``robin={"x_lo": (a, b), ...}`` for exactly
    the sides of the Robin axes: at a point next to a Robin wall the operand
    from beyond it is a * C + b of the point's own value C, at every fused
    level (arith "fma": fma(a, C, b)); the frame of the rows written gets the
    ghost values in ``dst``. Arith "exact" / "fma" / "auto", no ``source`` /
    ``rmap`` / ``faces``; on the device k is at most ``N.max_tb_rob()``
    (csrc/kernels/tb_impl.hpp ``tb_kernel_rob``).
    ``weights`` = (wS, wE, wN, wW, wC): the constant-coefficient five-point
    operator T' = wS*S + wE*E + wN*N + wW*W + wC*C at every fused level (operands
    S = T[i+1,j], E = T[i,j+1], N = T[i-1,j], W = T[i,j-1], C = T[i,j]; every
    product and sum rounded, arith "fma" / "auto": the first product, then four
    fmas); ``r`` is not used. "dirichlet" or "periodic" axes, none of ``source``
    / ``rmap`` / ``faces`` / ``gain`` / ``robin``; on the device k is at most
    ``N.max_tb_w5()`` (csrc/kernels/tb_impl.hpp ``tb_kernel_w5``)."""
    if weights is not None:
        w_arr, ar, bc = _weights_args(weights, src, arith, bc_x, bc_y, (source, rmap, faces, gain, robin), "tb_step")
        _check_field(src, layout)
        _check_field(dst, layout)
        if src.dtype != dst.dtype or src.device != dst.device:
            raise ValueError("src/dst dtype/device mismatch")
        if src.data_ptr() == dst.data_ptr():
            raise ValueError("tb_step is out-of-place (ping-pong fields)")
        rb, re = (0, layout.nrows) if rows is None else rows
        if src.is_cuda:
            N.call("heat2d_tb_w5", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, _stream(src), tile_rows, ar, bc, w_arr)
        else:
            N.call("heat2d_cpu_tb_w5", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, ar, bc, w_arr)
        return
    if gain is not None:
        if source is None:
            raise RuntimeError("gain= scales a heat source: pass source=")
        if gain.dim() != 1 or gain.dtype != src.dtype or gain.device != src.device or not gain.is_contiguous():
            raise ValueError("gain must be a contiguous 1-D tensor of the field's dtype and device")
        if gain_pos < 0 or gain_pos + k > gain.numel():
            raise ValueError(f"gain has {gain.numel()} entries: levels {gain_pos}..{gain_pos + k - 1} run past its end")
        if not bool((torch.isfinite(gain) & (gain >= 0)).all()):
            raise ValueError("gain entries must be finite and >= 0 (put the sign into the source)")
    _check_field(src, layout)
    _check_field(dst, layout)
    if faces is not None:
        rx, ry = faces
        for f in (rx, ry):
            _check_field(f, layout)
            if f.dtype != src.dtype or f.device != src.device:
                raise ValueError("faces dtype/device mismatch")
        if source is not None or rmap is not None:
            raise ValueError("face coefficients together with a heat source or a diffusivity map: no kernel carries them")
        if bc_x != "dirichlet" or bc_y != "dirichlet":
            raise ValueError("face coefficients need Dirichlet boundaries on both axes")
        if arith not in ("exact", "fma", "auto"):
            raise ValueError("face coefficients need arith 'exact', 'fma' or 'auto'")
        rb, re = (0, layout.nrows) if rows is None else rows
        ar = N.ARITH["fma"] if arith == "fma" else N.ARITH["exact"]
        if src.is_cuda:
            N.call("heat2d_tb_div", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, _stream(src), tile_rows, ar, C.c_void_p(rx.data_ptr()),
                   C.c_void_p(ry.data_ptr()))
        else:
            N.call("heat2d_cpu_tb_div", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, ar, C.c_void_p(rx.data_ptr()), C.c_void_p(ry.data_ptr()))
        return
    if rmap is not None:
        _check_field(rmap, layout)
        if rmap.dtype != src.dtype or rmap.device != src.device:
            raise ValueError("rmap dtype/device mismatch")
        if source is not None:
            raise ValueError("a diffusivity map and a heat source together: no kernel carries both")
        if bc_x != "dirichlet" or bc_y != "dirichlet":
            raise ValueError("a diffusivity map needs Dirichlet boundaries on both axes")
        if arith not in ("exact", "fma", "auto"):
            raise ValueError("a diffusivity map needs arith 'exact', 'fma' or 'auto'")
    if source is not None:
        _check_field(source, layout)
        if source.dtype != src.dtype or source.device != src.device:
            raise ValueError("source dtype/device mismatch")
        if bc_x != "dirichlet" or bc_y != "dirichlet":
            raise ValueError("a heat source needs Dirichlet boundaries on both axes")
        if arith not in ("exact", "fma", "auto"):
            raise ValueError("a heat source needs arith 'exact', 'fma' or 'auto'")
    if src.dtype != dst.dtype or src.device != dst.device:
        raise ValueError("src/dst dtype/device mismatch")
    if src.data_ptr() == dst.data_ptr():
        raise ValueError("tb_step is out-of-place (ping-pong fields)")
    has_robin = bc_x == "robin" or bc_y == "robin"
    if has_robin or robin is not None:
        rob_arr, _ = N.robin_array(robin, bc_x, bc_y, np.float32 if src.dtype == torch.float32 else np.float64)
    if has_robin and arith not in ("exact", "fma", "auto"):
        raise ValueError("Robin walls need arith 'exact', 'fma' or 'auto' (the scaled levels of jacobi / fast would need b "
                         "scaled per level)")
    rb, re = (0, layout.nrows) if rows is None else rows
    ar = N.arith_code(arith, r)
    bc = N.bc_bits(bc_x, bc_y)
    if rmap is not None:
        ar = N.ARITH["fma"] if arith == "fma" else N.ARITH["exact"]
        if src.is_cuda:
            N.call("heat2d_tb_var", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, _stream(src), tile_rows, ar, C.c_void_p(rmap.data_ptr()))
        else:
            N.call("heat2d_cpu_tb_var", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, ar, C.c_void_p(rmap.data_ptr()))
        return
    if source is not None and gain is not None:
        pos = torch.tensor([int(gain_pos)], dtype=torch.int64, device=src.device)
        if src.is_cuda:
            N.call("heat2d_tb_gain", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, r, _stream(src), tile_rows, ar, C.c_void_p(source.data_ptr()),
                   C.c_void_p(gain.data_ptr()), C.c_void_p(pos.data_ptr()))
            torch.cuda.current_stream(src.device).synchronize()  # keep pos alive until done
        else:
            N.call("heat2d_cpu_tb_gain", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, r, ar, C.c_void_p(source.data_ptr()), C.c_void_p(gain.data_ptr()),
                   C.c_void_p(pos.data_ptr()))
        return
    if source is not None:
        if src.is_cuda:
            N.call("heat2d_tb_src", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, r, _stream(src), tile_rows, ar, C.c_void_p(source.data_ptr()))
        else:
            N.call("heat2d_cpu_tb_src", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, r, ar, C.c_void_p(source.data_ptr()))
        return
    if has_robin:
        if src.is_cuda:
            N.call("heat2d_tb_rob", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, r, _stream(src), tile_rows, ar, bc, rob_arr)
        else:
            N.call("heat2d_cpu_tb_rob", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
                   C.byref(layout), rb, re, k, r, ar, bc, rob_arr)
        return
    if src.is_cuda:
        N.call("heat2d_tb_bc", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
               C.byref(layout), rb, re, k, r, _stream(src), tile_rows, ar, bc)
    else:
        N.call("heat2d_cpu_tb_bc", dtype_code(src), C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()),
               C.byref(layout), rb, re, k, r, ar, bc)


MAX_PROBES = 4096  # common.hpp kMaxProbes


def probe_points(points, nrows_global: int, ncols: int) -> np.ndarray:
    """``points`` as a (P, 2) int64 array of GLOBAL frame-inclusive indices
    (i, j), 1 <= i <= nrows_global, 1 <= j <= ncols — the checked form every
    probe entry point takes. ValueError: a shape other than (P, 2), a
    non-integer entry, a point off the owned grid, more than MAX_PROBES."""
    a = np.asarray(points)
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"probes must have shape (P, 2), got {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"probes must be integer points (i, j), got dtype {a.dtype}")
    a = np.ascontiguousarray(a, dtype=np.int64)
    if len(a) > MAX_PROBES:
        raise ValueError(f"at most {MAX_PROBES} probes, got {len(a)}")
    bad = (a[:, 0] < 1) | (a[:, 0] > nrows_global) | (a[:, 1] < 1) | (a[:, 1] > ncols)
    if bad.any():
        p = int(np.nonzero(bad)[0][0])
        raise ValueError(f"probe {p} = ({a[p, 0]}, {a[p, 1]}) is not an owned point "
                         f"(1..{nrows_global}, 1..{ncols})")
    return a


def probe_cone(src: torch.Tensor, layout: N.Layout, k: int, r: float, points, arith: str = "exact",
               bc_x: str = "dirichlet", bc_y: str = "dirichlet", source: Optional[torch.Tensor] = None,
               rmap: Optional[torch.Tensor] = None, faces: Optional[tuple] = None,
               gain: Optional[torch.Tensor] = None, robin=None, weights=None) -> torch.Tensor:
    """The probe-cone kernel alone (csrc/kernels/probe_cone.hip; CPU tensors:
    its twin): the values at ``points`` after each of the next k steps of
    ``src``, a (k, P) tensor of src's dtype and device — row s - 1 holds level
    s. ``points``: global frame-inclusive (i, j) whose rows this slab owns; the
    k ghost rows around them must be valid in ``src``. ``layout``, ``r``,
    ``arith`` ("exact" / "fma" / "jacobi"), ``bc_x`` / ``bc_y`` and the
    coefficient buffers are :func:`tb_step`'s. ``gain`` (with ``source``): the
    k gains of the levels, level s scaled by ``gain[s - 1]`` (``probe_cone_gain``).
    ``robin`` (with a "robin" axis, as :func:`tb_step`): the plain cone with the
    ghost value at the walls (``probe_cone_rob``), arith "exact" / "fma".
    ``weights`` (as :func:`tb_step`): the cone of the five-weight operator
    (``probe_cone_w5``), arith "exact" / "fma" / "auto"; ``r`` is not used.
    Nothing is written but the result."""
    if weights is not None:
        w_arr, ar, bc = _weights_args(weights, src, arith, bc_x, bc_y, (source, rmap, faces, gain, robin), "probe_cone")
        _check_field(src, layout)
        pts = probe_points(points, int(layout.nrows_global), int(layout.ncols))
        loc = pts - np.array([1 + layout.row0, 1], dtype=np.int64)
        if ((loc[:, 0] < 0) | (loc[:, 0] >= layout.nrows)).any():
            raise ValueError("probe_cone: a point's row is not an owned row of this slab")
        if not 1 <= k <= min(N.max_tb(), int(layout.halo)):
            raise ValueError(f"probe_cone: k must be in [1, {min(N.max_tb(), int(layout.halo))}]")
        out = torch.empty((k, len(pts)), dtype=src.dtype, device=src.device)
        if len(pts) == 0:
            return out
        dpts = torch.from_numpy(np.ascontiguousarray(loc)).to(src.device)
        N.call("heat2d_probe_cone_w5", dtype_code(src), C.c_void_p(src.data_ptr()), C.byref(layout), int(k), ar, bc, w_arr,
               C.c_void_p(dpts.data_ptr()), len(pts), C.c_void_p(out.data_ptr()), _stream(src), int(src.is_cuda))
        if src.is_cuda:
            torch.cuda.current_stream(src.device).synchronize()  # keep dpts alive until done
        return out
    if gain is not None:
        if source is None:
            raise RuntimeError("gain= scales a heat source: pass source=")
        if gain.dim() != 1 or gain.dtype != src.dtype or gain.device != src.device or not gain.is_contiguous():
            raise ValueError("gain must be a contiguous 1-D tensor of the field's dtype and device")
        if gain.numel() < k:
            raise ValueError(f"gain has {gain.numel()} entries for {k} levels")
        if not bool((torch.isfinite(gain) & (gain >= 0)).all()):
            raise ValueError("gain entries must be finite and >= 0 (put the sign into the source)")
    _check_field(src, layout)
    pts = probe_points(points, int(layout.nrows_global), int(layout.ncols))
    loc = pts - np.array([1 + layout.row0, 1], dtype=np.int64)
    if ((loc[:, 0] < 0) | (loc[:, 0] >= layout.nrows)).any():
        raise ValueError("probe_cone: a point's row is not an owned row of this slab")
    if not 1 <= k <= min(N.max_tb(), int(layout.halo)):
        raise ValueError(f"probe_cone: k must be in [1, {min(N.max_tb(), int(layout.halo))}]")
    if arith not in ("exact", "fma", "jacobi"):
        raise ValueError("probe_cone: arith 'exact', 'fma' or 'jacobi'")
    coefs = [source, rmap] + (list(faces) if faces is not None else [None, None])
    if (source is not None) + (rmap is not None) + (faces is not None) > 1:
        raise ValueError("probe_cone: at most one of source, rmap and faces")
    for f in coefs:
        if f is not None:
            _check_field(f, layout)
            if f.dtype != src.dtype or f.device != src.device:
                raise ValueError("coefficient buffer dtype/device mismatch")
    if any(f is not None for f in coefs):
        if bc_x != "dirichlet" or bc_y != "dirichlet":
            raise ValueError("a heat source, a diffusivity map and face coefficients need Dirichlet boundaries")
        if arith == "jacobi":
            raise ValueError("a heat source, a diffusivity map and face coefficients need arith 'exact' or 'fma'")
    has_robin = bc_x == "robin" or bc_y == "robin"
    if has_robin or robin is not None:
        rob_arr, _ = N.robin_array(robin, bc_x, bc_y, np.float32 if src.dtype == torch.float32 else np.float64)
    if has_robin and arith not in ("exact", "fma"):
        raise ValueError("probe_cone: Robin walls need arith 'exact' or 'fma'")
    ar = N.arith_code(arith, r)
    out = torch.empty((k, len(pts)), dtype=src.dtype, device=src.device)
    if len(pts) == 0:
        return out
    dpts = torch.from_numpy(np.ascontiguousarray(loc)).to(src.device)
    ptr = [C.c_void_p(f.data_ptr()) if f is not None else None for f in coefs]
    if gain is not None:
        N.call("heat2d_probe_cone_gain", dtype_code(src), C.c_void_p(src.data_ptr()), C.byref(layout), int(k), float(r),
               ar, ptr[0], C.c_void_p(gain.data_ptr()), C.c_void_p(dpts.data_ptr()), len(pts),
               C.c_void_p(out.data_ptr()), _stream(src), int(src.is_cuda))
        if src.is_cuda:
            torch.cuda.current_stream(src.device).synchronize()  # keep dpts alive until done
        return out
    if has_robin:
        N.call("heat2d_probe_cone_rob", dtype_code(src), C.c_void_p(src.data_ptr()), C.byref(layout), int(k), float(r),
               ar, N.bc_bits(bc_x, bc_y), rob_arr, C.c_void_p(dpts.data_ptr()), len(pts), C.c_void_p(out.data_ptr()),
               _stream(src), int(src.is_cuda))
        if src.is_cuda:
            torch.cuda.current_stream(src.device).synchronize()  # keep dpts alive until done
        return out
    N.call("heat2d_probe_cone", dtype_code(src), C.c_void_p(src.data_ptr()), C.byref(layout), int(k), float(r), ar,
           N.bc_bits(bc_x, bc_y), ptr[0], ptr[1], ptr[2], ptr[3], C.c_void_p(dpts.data_ptr()), len(pts),
           C.c_void_p(out.data_ptr()), _stream(src), int(src.is_cuda))
    if src.is_cuda:
        torch.cuda.current_stream(src.device).synchronize()  # keep dpts alive until done
    return out


def source_field(S: np.ndarray, layout: N.Layout, dtype: torch.dtype, device="cpu") -> torch.Tensor:
    """The heat-source buffer :func:`tb_step` takes, from the GLOBAL
    frame-inclusive array ``S`` ((nrows_global + 2) x (ncols + 2)): -0.0
    everywhere, then the owned points of every allocated row of the slab that
    is an owned row of the grid (ghost rows included)."""
    if S.shape != (layout.nrows_global + 2, layout.ncols + 2):
        raise ValueError(f"source must be {(layout.nrows_global + 2, layout.ncols + 2)}, got {S.shape}")
    f = torch.full((layout.rows_alloc(), layout.pitch), -0.0, dtype=dtype)
    Sd = torch.as_tensor(np.ascontiguousarray(S)).to(dtype)
    for i in range(-layout.halo, layout.nrows + layout.halo):
        g = layout.row0 + i
        if 0 <= g < layout.nrows_global:
            f[i + layout.halo, layout.cpad:layout.cpad + layout.ncols] = Sd[g + 1, 1:-1]
    return f.reshape(-1).to(device)


def rmap_field(R: np.ndarray, layout: N.Layout, dtype: torch.dtype, device="cpu") -> torch.Tensor:
    """The diffusivity-map buffer :func:`tb_step` takes, from the GLOBAL
    frame-inclusive array ``R`` ((nrows_global + 2) x (ncols + 2)): +0.0
    everywhere, then the owned points of every allocated row of the slab that
    is an owned row of the grid (ghost rows included)."""
    if R.shape != (layout.nrows_global + 2, layout.ncols + 2):
        raise ValueError(f"rmap must be {(layout.nrows_global + 2, layout.ncols + 2)}, got {R.shape}")
    f = torch.zeros((layout.rows_alloc(), layout.pitch), dtype=dtype)
    Rd = torch.as_tensor(np.ascontiguousarray(R)).to(dtype)
    for i in range(-layout.halo, layout.nrows + layout.halo):
        g = layout.row0 + i
        if 0 <= g < layout.nrows_global:
            f[i + layout.halo, layout.cpad:layout.cpad + layout.ncols] = Rd[g + 1, 1:-1]
    return f.reshape(-1).to(device)


def faces_field(RX: np.ndarray, RY: np.ndarray, layout: N.Layout, dtype: torch.dtype, device="cpu") -> tuple:
    """The two face-coefficient buffers :func:`tb_step` takes, from the GLOBAL
    frame-inclusive arrays ``RX``, ``RY`` ((nrows_global + 2) x (ncols + 2)):
    +0.0 everywhere, then the used faces of every allocated row of the slab —
    rx: the owned rows, columns -1 (the frame column's east face) .. ncols - 1;
    ry: rows -1 (the frame row's south face) .. nrows_global - 1, the owned
    columns."""
    out = []
    for w, A in enumerate((RX, RY)):
        if A.shape != (layout.nrows_global + 2, layout.ncols + 2):
            raise ValueError(f"faces must be {(layout.nrows_global + 2, layout.ncols + 2)}, got {A.shape}")
        f = torch.zeros((layout.rows_alloc(), layout.pitch), dtype=dtype)
        Ad = torch.as_tensor(np.ascontiguousarray(A)).to(dtype)
        c = layout.cpad
        for i in range(-layout.halo, layout.nrows + layout.halo):
            g = layout.row0 + i
            if w == 0 and 0 <= g < layout.nrows_global:
                f[i + layout.halo, c - 1:c + layout.ncols] = Ad[g + 1, 0:-1]
            if w == 1 and -1 <= g < layout.nrows_global:
                f[i + layout.halo, c:c + layout.ncols] = Ad[g + 1, 1:-1]
        out.append(f.reshape(-1).to(device))
    return tuple(out)


WRAP_COLS = 24  # ghost columns per side that wrap_cols fills (kernels.hpp kWrapCols)


def wrap_cols(field: torch.Tensor, layout: N.Layout, rows: Optional[tuple[int, int]] = None) -> None:
    """Periodic y: fill the WRAP_COLS ghost columns on each side of ``rows``
    (default: every allocated row, ghost rows included) with wrap images of the
    owned columns: column -1-j <- ncols-1-j, column ncols+j <- j."""
    _check_field(field, layout)
    r0, r1 = (-layout.halo, layout.nrows + layout.halo) if rows is None else rows
    N.call("heat2d_wrap_cols", dtype_code(field), C.c_void_p(field.data_ptr()), C.byref(layout), r0, r1,
           _stream(field) if field.is_cuda else None, int(field.is_cuda))


def wrap_rows(field: torch.Tensor, layout: N.Layout, k: int) -> None:
    """Periodic x on one slab: whole padded rows [nrows-k, nrows) -> ghost rows
    [-k, 0) and [0, k) -> [nrows, nrows+k) (k <= halo, k <= nrows)."""
    _check_field(field, layout)
    N.call("heat2d_wrap_rows", dtype_code(field), C.c_void_p(field.data_ptr()), C.byref(layout), k,
           _stream(field) if field.is_cuda else None, int(field.is_cuda))


def stats(field: torch.Tensor, layout: N.Layout, other: Optional[torch.Tensor] = None) -> dict:
    """sum, sum of squares, min, max (+ L2 / max-abs difference vs `other`) of the owned region."""
    _check_field(field, layout)
    optr = C.c_void_p(other.data_ptr()) if other is not None else None
    if field.is_cuda:
        work = torch.empty(int(N.lib().heat2d_stats_work_elems()) + 8, dtype=torch.float64, device=field.device)
        out = work[-8:]
        N.call("heat2d_stats", dtype_code(field), C.c_void_p(field.data_ptr()), optr, C.byref(layout),
               C.c_void_p(work.data_ptr()), C.c_void_p(out.data_ptr()), _stream(field))
        v = out[:6].cpu().tolist()
    else:
        o = (C.c_double * 6)()
        N.call("heat2d_cpu_stats", dtype_code(field), C.c_void_p(field.data_ptr()), optr, C.byref(layout), o)
        v = list(o)
    d = {"sum": v[0], "sum_sq": v[1], "min": v[2], "max": v[3]}
    if other is not None:
        d["diff_l2"] = float(np.sqrt(v[4]))
        d["diff_max"] = v[5]
    return d


def pack_rows(field: torch.Tensor, layout: N.Layout, row: int, nrows: int,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Copy owned columns of rows [row, row+nrows) into a contiguous (nrows*ncols) buffer."""
    _check_field(field, layout)
    if out is None:
        out = torch.empty(nrows * layout.ncols, dtype=field.dtype, device=field.device)
    if field.is_cuda:
        N.call("heat2d_pack_rows", dtype_code(field), C.c_void_p(field.data_ptr()), C.byref(layout), row, nrows,
               C.c_void_p(out.data_ptr()), _stream(field))
    else:
        out.view(nrows, layout.ncols).copy_(view2d(field, layout)[layout.halo + row:layout.halo + row + nrows,
                                                                   layout.cpad:layout.cpad + layout.ncols])
    return out


def unpack_rows(field: torch.Tensor, layout: N.Layout, row: int, nrows: int, buf: torch.Tensor) -> None:
    _check_field(field, layout)
    if field.is_cuda:
        N.call("heat2d_unpack_rows", dtype_code(field), C.c_void_p(field.data_ptr()), C.byref(layout), row, nrows,
               C.c_void_p(buf.data_ptr()), _stream(field))
    else:
        view2d(field, layout)[layout.halo + row:layout.halo + row + nrows,
                              layout.cpad:layout.cpad + layout.ncols].copy_(buf.view(nrows, layout.ncols))


def copy_(dst: torch.Tensor, src: torch.Tensor) -> None:
    """Vectorised 16-B streaming device copy (the copy-swap parity op)."""
    nbytes = src.numel() * src.element_size()
    if not (src.is_cuda and dst.is_cuda) or nbytes % 16:
        dst.copy_(src)
        return
    N.call("heat2d_copy", C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), nbytes, _stream(src), 0)
