"""The error surface of TbTerms::weights (kernels.hpp): what the raw C API can
express of the five-weight operator and no kernel carries is rejected before
anything is launched, each with its own message — by the device launchers in
stencil_tb.hip select_family (through heat2d_tb_w5) and by the CPU twin cpu::tb
(through heat2d_cpu_tb_w5). In the style of tests/test_terms_reject.py: a 64 x 64
fp64 slab at depth 2; the rejections need no GPU (without one the device
launcher's planning falls back to constants and select_family is reached all the
same), with one the module holds device buffers and belongs to the GPU suite.

No case for weights beside source / rmap / faces / gain, the fused statistics or
the wave-pair kernel: select_family rejects each with a message of its own, but
heat2d_tb_w5 takes none of those buffers and launches neither of those kernels,
so they cannot be expressed here (the solver and the Python layer refuse them
first: tests/test_weights.py).
"""
import ctypes as C

import pytest
import torch

from heat2d.ops import _native as N

HAS_GPU = torch.cuda.is_available()
pytestmark = [pytest.mark.gpu] if HAS_GPU else []

N_, K, HALO = 64, 2, 24
PX, PY, IX, IY, RX, RY = (N.BC_PERIODIC_X, N.BC_PERIODIC_Y, N.BC_INSULATED_X, N.BC_INSULATED_Y, N.BC_ROBIN_X,
                          N.BC_ROBIN_Y)
EXACT, FMA, JACOBI, FAST = 0, 1, 2, 3


class Slab:
    def __init__(self, device):
        self.L = N.make_layout(N_, N_, HALO)
        n = self.L.elems()
        self.src = torch.rand(n, dtype=torch.float64).to(device)
        self.dst = torch.full((n,), -7.0, dtype=torch.float64, device=device)  # (any launch would write over it)
        self.w = (C.c_double * 5)(0.11, 0.07, 0.23, 0.19, 0.37)
        self.nan = (C.c_double * 5)(0.11, 0.07, float("nan"), 0.19, 0.37)
        self.inf = (C.c_double * 5)(0.11, 0.07, 0.23, 0.19, float("inf"))
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None

    def head(self):
        return (N.F64, C.c_void_p(self.src.data_ptr()), C.c_void_p(self.dst.data_ptr()), C.byref(self.L), 0, N_)


@pytest.fixture(scope="module")
def dev(native):
    return Slab("cuda:0" if HAS_GPU else "cpu")


@pytest.fixture(scope="module")
def host(native):
    return Slab("cpu")


WALLS = "weights need Dirichlet or periodic axes: no insulated or Robin walls"
# heat2d_tb_w5(dtype, src, dst, L, rb, re, k, stream, tile_rows, arith, bc, weights)
DEVICE = {
    "no weights": (lambda s: (K, s.stream, 0, EXACT, 0, None), "heat2d_tb_w5 needs the five weights"),
    "arith 2": (lambda s: (K, s.stream, 0, JACOBI, 0, s.w), "weights need arith 0 (exact) or 1 (fma)"),
    "arith 3": (lambda s: (K, s.stream, 0, FAST, PX, s.w), "weights need arith 0 (exact) or 1 (fma)"),
    "insulated x": (lambda s: (K, s.stream, 0, EXACT, IX, s.w), WALLS),
    "insulated y": (lambda s: (K, s.stream, 0, FMA, IY | PX, s.w), WALLS),
    "Robin x": (lambda s: (K, s.stream, 0, EXACT, RX, s.w), WALLS),
    "Robin y": (lambda s: (K, s.stream, 0, EXACT, RY, s.w), WALLS),
    "x periodic and insulated": (lambda s: (K, s.stream, 0, EXACT, PX | IX, s.w), "an axis is periodic or insulated, not both"),
    "unknown bc bit": (lambda s: (K, s.stream, 0, EXACT, 64, s.w), "bc must be a set of"),
    "a NaN weight": (lambda s: (K, s.stream, 0, EXACT, 0, s.nan), "weights must be finite"),
    "an infinite weight": (lambda s: (K, s.stream, 0, FMA, PY, s.inf), "weights must be finite"),
}
# heat2d_cpu_tb_w5(dtype, src, dst, L, rb, re, k, arith, bc, weights)
CPU = {
    "no weights": (lambda s: (K, EXACT, 0, None), "heat2d_cpu_tb_w5 needs the five weights"),
    "arith 2": (lambda s: (K, JACOBI, 0, s.w), "arith 2 (jacobi) needs r == 1/4 exactly"),  # (r is not passed: 0)
    "arith 3": (lambda s: (K, FAST, 0, s.w), "weights need arith 0 (exact) or 1 (fma)"),
    "insulated x": (lambda s: (K, EXACT, IX, s.w), WALLS),
    "Robin y": (lambda s: (K, FMA, RY, s.w), "Robin walls need their pairs"),  # (the twin's Robin check comes first)
    "insulated y": (lambda s: (K, FMA, IY, s.w), WALLS),
    "a NaN weight": (lambda s: (K, EXACT, PX | PY, s.nan), "weights must be finite"),
}


def rejected(slab, entry, args, phrase):
    before = slab.dst.clone()
    with pytest.raises(N.NativeError) as e:
        N.call(entry, *slab.head(), *args(slab))
    assert phrase in str(e.value), str(e.value)
    if slab.dst.is_cuda:
        torch.cuda.synchronize()
    assert torch.equal(slab.dst, before)  # nothing ran


@pytest.mark.parametrize("case", sorted(DEVICE))
def test_device_launcher_rejects(dev, case):
    rejected(dev, "heat2d_tb_w5", *DEVICE[case])


@pytest.mark.parametrize("case", sorted(CPU))
def test_cpu_twin_rejects(host, case):
    rejected(host, "heat2d_cpu_tb_w5", *CPU[case])


def test_depth_limit_follows_the_constant(native):
    """kMaxTBW5 is the general kernels' own deepest pass here, so the launcher's depth check (check_layout)
    speaks before select_family's; the constant is what the solver and info() report."""
    assert N.max_tb_w5() == N.max_tb()
