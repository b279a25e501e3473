"""The error surface of the stencil launchers' terms (kernels.hpp TbTerms): every
combination of terms the raw C API can express and no kernel carries is rejected,
before anything is launched, with its own message.

The device launchers decide the kernel family of a launch and reject in one place
(stencil_tb.hip select_family); the CPU twin (cpu::tb) has its own checks. Both
run here through the entry points the Python layer uses, on a 64 x 64 fp64 slab
at depth 2 (the depth-limit cases: one level past the family's deepest pass).
The rejections need no GPU. A device launcher reaches select_family after
check_layout and plan_tb; without a GPU those run all the same (the CU count and
the occupancy queries fall back to constants), so this module is part of the
non-GPU suite there, and a change to check_layout or plan_tb that needs a device
shows here. With a GPU it holds device buffers and belongs to the GPU suite.

No case for source + rmap, faces + source, faces + rmap, or any of the three with
a non-zero bc: select_family rejects them, but no raw entry point takes two of
these buffers, or one of them beside a bc, so they cannot be expressed here (the
solver and the Python layer reject them with messages of their own first).
"""
import ctypes as C

import pytest
import torch

from heat2d.ops import _native as N

HAS_GPU = torch.cuda.is_available()
pytestmark = [pytest.mark.gpu] if HAS_GPU else []

N_, K, HALO = 64, 2, 24
R = 0.25  # (arith 2 is the r = 1/4 form: no case fails on r)
PX, PY, IX, IY, RX, RY = (N.BC_PERIODIC_X, N.BC_PERIODIC_Y, N.BC_INSULATED_X, N.BC_INSULATED_Y, N.BC_ROBIN_X,
                          N.BC_ROBIN_Y)
EXACT, JACOBI, FAST = 0, 2, 3


class Slab:
    """Buffers a launch could run on, were it not rejected: two fields, four
    term buffers in the field's layout, a gain array with its position word,
    and the Robin pairs (host memory on either side)."""

    def __init__(self, device):
        self.L = N.make_layout(N_, N_, HALO)
        n = self.L.elems()
        z = lambda: torch.zeros(n, dtype=torch.float64, device=device)
        self.q, self.m, self.fx, self.fy = z(), z(), z(), z()
        self.src = torch.rand(n, dtype=torch.float64).to(device)
        self.dst = torch.full((n,), -7.0, dtype=torch.float64, device=device)  # (any launch would write over it)
        self.gain = torch.ones(64, dtype=torch.float64, device=device)
        self.pos = torch.zeros(1, dtype=torch.int64, device=device)
        self.pairs = (C.c_double * 8)(*([0.5, 1.0] * 4))
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream) if device != "cpu" else None

    def head(self):
        return (N.F64, C.c_void_p(self.src.data_ptr()), C.c_void_p(self.dst.data_ptr()), C.byref(self.L), 0, N_)


@pytest.fixture(scope="module")
def dev(native):
    return Slab("cuda:0" if HAS_GPU else "cpu")


@pytest.fixture(scope="module")
def host(native):
    return Slab("cpu")


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# (entry point, the arguments after (dtype, src, dst, layout, rb, re) as a function of the slab, key phrase)
DEVICE = {
    "gain without source": ("heat2d_tb_gain", lambda s: (K, R, s.stream, 0, EXACT, None, p(s.gain), p(s.pos)),
                            "a gain schedule needs a heat source and its position word"),
    "gain without position word": ("heat2d_tb_gain", lambda s: (K, R, s.stream, 0, EXACT, p(s.q), p(s.gain), None),
                                   "a gain schedule needs a heat source and its position word"),
    "Robin x without pairs": ("heat2d_tb_bc", lambda s: (K, R, s.stream, 0, EXACT, RX),
                              "a Robin axis needs the walls' pairs"),
    "Robin y without pairs": ("heat2d_tb_bc", lambda s: (K, R, s.stream, 0, EXACT, RY | IX),
                              "a Robin axis needs the walls' pairs"),
    "insulated x, arith 3": ("heat2d_tb_bc", lambda s: (K, R, s.stream, 0, FAST, IX),
                             "insulated boundaries have no arith 3 (fast) kernels"),
    "insulated y, arith 3": ("heat2d_tb_bc", lambda s: (K, R, s.stream, 0, FAST, IY),
                             "insulated boundaries have no arith 3 (fast) kernels"),
    "Robin, arith 3": ("heat2d_tb_rob", lambda s: (K, R, s.stream, 0, FAST, RX | RY, s.pairs),
                       "insulated boundaries have no arith 3 (fast) kernels"),
    "source, arith 2": ("heat2d_tb_src", lambda s: (K, R, s.stream, 0, JACOBI, p(s.q)),
                        "a heat source needs arith 0 (exact) or 1 (fma)"),
    "gain, arith 2": ("heat2d_tb_gain", lambda s: (K, R, s.stream, 0, JACOBI, p(s.q), p(s.gain), p(s.pos)),
                      "a gain schedule needs arith 0 (exact) or 1 (fma)"),
    "map, arith 2": ("heat2d_tb_var", lambda s: (K, s.stream, 0, JACOBI, p(s.m)),
                     "a diffusivity map needs arith 0 (exact) or 1 (fma)"),
    "faces, arith 2": ("heat2d_tb_div", lambda s: (K, s.stream, 0, JACOBI, p(s.fx), p(s.fy)),
                       "face coefficients need arith 0 (exact) or 1 (fma)"),
    "Robin, arith 2": ("heat2d_tb_rob", lambda s: (K, R, s.stream, 0, JACOBI, RY, s.pairs),
                       "Robin walls need arith 0 (exact) or 1 (fma)"),
    "x periodic and insulated": ("heat2d_tb_bc", lambda s: (K, R, s.stream, 0, EXACT, PX | IX),
                                 "an axis is periodic or insulated, not both"),
    "y periodic and insulated": ("heat2d_tb_bc", lambda s: (K, R, s.stream, 0, EXACT, PY | IY),
                                 "an axis is periodic or insulated, not both"),
    "x Robin and periodic": ("heat2d_tb_rob", lambda s: (K, R, s.stream, 0, EXACT, RX | PX, s.pairs),
                             "an axis has one boundary kind: Robin, periodic or insulated"),
    "y Robin and insulated": ("heat2d_tb_rob", lambda s: (K, R, s.stream, 0, EXACT, RY | IY, s.pairs),
                              "an axis has one boundary kind: Robin, periodic or insulated"),
    "unknown bc bit": ("heat2d_tb_bc", lambda s: (K, R, s.stream, 0, EXACT, 64), "bc must be a set of"),
    "source past its deepest pass": ("heat2d_tb_src", lambda s: (17, R, s.stream, 0, EXACT, p(s.q)),
                                     "deepest pass (kMaxTBSrc)"),
    "gain past its deepest pass": ("heat2d_tb_gain",
                                   lambda s: (17, R, s.stream, 0, EXACT, p(s.q), p(s.gain), p(s.pos)),
                                   "deepest pass (kMaxTBSrc)"),
    "map past its deepest pass": ("heat2d_tb_var", lambda s: (17, s.stream, 0, EXACT, p(s.m)),
                                  "deepest pass (kMaxTBVar)"),
    "faces past their deepest pass": ("heat2d_tb_div", lambda s: (17, s.stream, 0, EXACT, p(s.fx), p(s.fy)),
                                      "deepest pass (kMaxTBDiv)"),
}

CPU = {
    "gain without source": ("heat2d_cpu_tb_gain", lambda s: (K, R, EXACT, None, p(s.gain), p(s.pos)),
                            "a gain schedule needs a heat source and its position word"),
    "insulated, arith 3": ("heat2d_cpu_tb_bc", lambda s: (K, R, FAST, IX | IY),
                           "insulated boundaries have no arith 3 (fast) kernels"),
    "Robin, arith 2": ("heat2d_cpu_tb_rob", lambda s: (K, R, JACOBI, RX, s.pairs),
                       "Robin walls need their pairs and arith 0 (exact) or 1 (fma)"),
    "Robin, arith 3": ("heat2d_cpu_tb_rob", lambda s: (K, R, FAST, RY, s.pairs),
                       "Robin walls need their pairs and arith 0 (exact) or 1 (fma)"),
    "source, arith 2": ("heat2d_cpu_tb_src", lambda s: (K, R, JACOBI, p(s.q)),
                        "a heat source needs arith 0 (exact) or 1 (fma)"),
    # (these two entry points pass r = 0, which arith 2 itself rejects: the scaled form stands for both)
    "map, arith 3": ("heat2d_cpu_tb_var", lambda s: (K, FAST, p(s.m)),
                     "a diffusivity map needs arith 0 (exact) or 1 (fma)"),
    "faces, arith 3": ("heat2d_cpu_tb_div", lambda s: (K, FAST, p(s.fx), p(s.fy)),
                       "face coefficients need arith 0 (exact) or 1 (fma)"),
    "x periodic and insulated": ("heat2d_cpu_tb_bc", lambda s: (K, R, EXACT, PX | IX),
                                 "an axis is periodic or insulated, not both"),
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
    rejected(dev, *DEVICE[case])


@pytest.mark.parametrize("case", sorted(CPU))
def test_cpu_twin_rejects(host, case):
    rejected(host, *CPU[case])
