"""The heat-source kernels (tb_kernel_src, csrc/kernels/tb_impl.hpp) in the
built library's gfx950 code objects (no GPU needed): one instance per dtype,
depth 1..D and arithmetic form (exact, fma; jacobi and "fast" have none), none
with scratch; D is the clamp a solver with a source reports. Registers, LDS
and occupancy are printed, not asserted."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_report  # noqa: E402
from source_worker import problem, rough_source  # noqa: E402

LIB = os.path.join(ROOT, "cuda-hip-mpi-heat-equation-test_amd", "_native", "libheat2d.so")
ARITH = ("exact", "fma")
# tb_kernel_src<T, NV, K, RING, AR>
_SRC = re.compile(r"tb_kernel_srcI([df])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")


def src_params(mangled):
    m = _SRC.search(mangled)
    return ("fp64" if m.group(1) == "d" else "fp32", int(m.group(2)), int(m.group(3)), int(m.group(4)),
            int(m.group(5))) if m else None


@pytest.fixture(scope="module")
def src(native):
    ks = [(src_params(k["name"]), k) for k in isa_report.kernels(LIB)]
    return [(p, k) for p, k in ks if p]


def depth_in_library(src):
    return max(p[2] for p, _ in src)


def test_src_instances_present(src):
    D = depth_in_library(src)
    assert D >= 16
    want = [(dt, 1, k, 4, ar) for dt in ("fp32", "fp64") for k in range(1, D + 1) for ar in range(2)]
    assert sorted(p for p, _ in src) == sorted(want)


def test_src_pattern_is_disjoint_from_the_other_kernels(src):
    """Neither tools/isa_report.py's tb_kernel / tb_kernel_pipe patterns nor
    tests/test_insulated_isa.py's may see the source kernel (their tests count
    their matches exactly)."""
    import test_insulated_isa
    assert src, "no tb_kernel_src instance in the library"
    assert all(isa_report.tb_params(k["name"]) is None and isa_report.pipe_params(k["name"]) is None and
               test_insulated_isa.ins_params(k["name"]) is None for _, k in src)


def test_src_no_scratch(src):
    assert src, "no tb_kernel_src instance in the library"
    for (dt, nv, depth, ring, ar), k in sorted(src, key=lambda x: x[0]):
        tag = (f"tb_kernel_src<{dt}, K={depth:2d}, {ARITH[ar]}>: vgpr {k['vgpr']:3d} agpr {k['agpr']:3d} "
               f"lds {k.get('lds', '?')} scratch {k['scratch']} waves/SIMD {k['waves_per_simd']}")
        print(tag)
        assert k["scratch"] == 0, tag


def test_clamp_is_the_depth_in_the_library(src):
    from heat2d.models.heat2d import HeatSolver
    D = depth_in_library(src)
    for dtype in ("fp64", "fp32"):
        s = HeatSolver(problem(301, 4), dtype=dtype, backend="cpu", source=rough_source(301, dtype))
        info = s.info()
        s.close()
        assert info["source"]["max_tb"] == D and info["tb"] <= D
