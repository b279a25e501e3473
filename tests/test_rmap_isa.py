"""The diffusivity-map kernels (tb_kernel_var, csrc/kernels/tb_impl.hpp) in the
built library's gfx950 code objects (no GPU needed): one instance per dtype,
depth 1..D and arithmetic form (exact, fma; jacobi and "fast" have none), none
with scratch; D is the clamp a solver with a map reports. Registers, LDS and
occupancy are printed, not asserted."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_report  # noqa: E402
from rmap_worker import problem, rough_map  # noqa: E402

LIB = os.path.join(ROOT, "cuda-hip-mpi-heat-equation-test_amd", "_native", "libheat2d.so")
ARITH = ("exact", "fma")
# tb_kernel_var<T, NV, K, RING, AR>
_VAR = re.compile(r"tb_kernel_varI([df])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")


def var_params(mangled):
    m = _VAR.search(mangled)
    return ("fp64" if m.group(1) == "d" else "fp32", int(m.group(2)), int(m.group(3)), int(m.group(4)),
            int(m.group(5))) if m else None


@pytest.fixture(scope="module")
def var(native):
    ks = [(var_params(k["name"]), k) for k in isa_report.kernels(LIB)]
    return [(p, k) for p, k in ks if p]


def depth_in_library(var):
    return max(p[2] for p, _ in var)


def test_var_instances_present(var):
    assert var, "no tb_kernel_var instance in the library"
    D = depth_in_library(var)
    assert D >= 8
    want = [(dt, 1, k, 4, ar) for dt in ("fp32", "fp64") for k in range(1, D + 1) for ar in range(2)]
    assert sorted(p for p, _ in var) == sorted(want)


def test_var_pattern_is_disjoint_from_the_other_kernels(var):
    """Neither tools/isa_report.py's tb_kernel / tb_kernel_pipe patterns nor the insulated and
    source tests' may see the map kernel (their tests count their matches exactly), nor this
    file's pattern theirs."""
    import test_insulated_isa
    import test_source_isa
    assert var, "no tb_kernel_var instance in the library"
    assert all(isa_report.tb_params(k["name"]) is None and isa_report.pipe_params(k["name"]) is None and
               test_insulated_isa.ins_params(k["name"]) is None and test_source_isa.src_params(k["name"]) is None
               for _, k in var)
    others = [k["name"] for k in isa_report.kernels(LIB)
              if isa_report.tb_params(k["name"]) or isa_report.pipe_params(k["name"]) or
              test_insulated_isa.ins_params(k["name"]) or test_source_isa.src_params(k["name"])]
    assert others and all(var_params(nm) is None for nm in others)


def test_var_no_scratch(var):
    assert var, "no tb_kernel_var instance in the library"
    for (dt, nv, depth, ring, ar), k in sorted(var, key=lambda x: x[0]):
        tag = (f"tb_kernel_var<{dt}, K={depth:2d}, {ARITH[ar]}>: vgpr {k['vgpr']:3d} agpr {k['agpr']:3d} "
               f"lds {k.get('lds', '?')} scratch {k['scratch']} waves/SIMD {k['waves_per_simd']}")
        print(tag)
        assert k["scratch"] == 0, tag


def test_clamp_is_the_depth_in_the_library(var):
    from heat2d.models.heat2d import HeatSolver
    assert var, "no tb_kernel_var instance in the library"
    D = depth_in_library(var)
    assert D >= 8
    for dtype in ("fp64", "fp32"):
        s = HeatSolver(problem(301, 4), dtype=dtype, backend="cpu", tb=24, rmap=rough_map(301, dtype))
        info = s.info()
        s.close()
        assert info["rmap"]["max_tb"] == D and info["tb"] == D
