"""The insulated-edge kernels (tb_kernel_ins, csrc/kernels/tb_impl.hpp) in the
built library's gfx950 code objects (no GPU needed): one instance per dtype,
depth 1..24 and arithmetic form (exact, fma, jacobi; "fast" has none), none
with scratch. Occupancy is printed, not asserted."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_report  # noqa: E402

LIB = os.path.join(ROOT, "cuda-hip-mpi-heat-equation-test_amd", "_native", "libheat2d.so")
ARITH = ("exact", "fma", "jacobi")
# tb_kernel_ins<T, NV, K, RING, AR>
_INS = re.compile(r"tb_kernel_insI([df])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")


def ins_params(mangled):
    m = _INS.search(mangled)
    return ("fp64" if m.group(1) == "d" else "fp32", int(m.group(2)), int(m.group(3)), int(m.group(4)),
            int(m.group(5))) if m else None


@pytest.fixture(scope="module")
def ins(native):
    ks = [(ins_params(k["name"]), k) for k in isa_report.kernels(LIB)]
    return [(p, k) for p, k in ks if p]


def test_ins_instances_present(ins):
    want = [(dt, 1, k, 4, ar) for dt in ("fp32", "fp64") for k in range(1, 25) for ar in range(3)]
    assert sorted(p for p, _ in ins) == sorted(want)


def test_ins_pattern_is_disjoint_from_tb_kernel(ins):
    """tools/isa_report.py's tb_kernel pattern must not see the insulated
    kernel (tests/test_isa.py counts its matches exactly)."""
    assert all(isa_report.tb_params(k["name"]) is None and isa_report.pipe_params(k["name"]) is None for _, k in ins)


def test_ins_no_scratch(ins):
    for (dt, nv, depth, ring, ar), k in sorted(ins, key=lambda x: x[0]):
        tag = (f"tb_kernel_ins<{dt}, K={depth:2d}, {ARITH[ar]}>: vgpr {k['vgpr']:3d} agpr {k['agpr']:3d} "
               f"scratch {k['scratch']} waves/SIMD {k['waves_per_simd']}")
        print(tag)
        assert k["scratch"] == 0, tag
