"""The conservative-form kernels (tb_kernel_div, csrc/kernels/tb_impl.hpp) in the
built library's gfx950 code objects (no GPU needed): exactly one instance per
dtype, depth 1..D and arithmetic form (exact, fma), none with scratch, static LDS
at most 40 KiB each (four one-wave workgroups fit a CU's 160 KiB); D is the
clamp a solver with faces reports. Registers and occupancy are printed, not
asserted."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_report  # noqa: E402
from faces_worker import problem, rough_faces  # noqa: E402

LIB = os.path.join(ROOT, "cuda-hip-mpi-heat-equation-test_amd", "_native", "libheat2d.so")
ARITH = ("exact", "fma")
# tb_kernel_div<T, NV, K, RING, AR>
_DIV = re.compile(r"tb_kernel_divI([df])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")


def div_params(mangled):
    m = _DIV.search(mangled)
    return ("fp64" if m.group(1) == "d" else "fp32", int(m.group(2)), int(m.group(3)), int(m.group(4)),
            int(m.group(5))) if m else None


@pytest.fixture(scope="module")
def div(native):
    ks = [(div_params(k["name"]), k) for k in isa_report.kernels(LIB)]
    return [(p, k) for p, k in ks if p]


def depth_in_library(div):
    return max(p[2] for p, _ in div)


def test_div_instances_present(div):
    """Exactly 2 dtypes x 2 forms x D instances."""
    assert div, "no tb_kernel_div instance in the library"
    D = depth_in_library(div)
    assert D >= 8
    want = [(dt, 1, k, 4, ar) for dt in ("fp32", "fp64") for k in range(1, D + 1) for ar in range(2)]
    assert sorted(p for p, _ in div) == sorted(want) and len(div) == 2 * 2 * D


def test_div_pattern_is_disjoint_from_the_other_kernels(div):
    """None of the existing patterns (tools/isa_report.py's tb_kernel / tb_kernel_pipe, the
    insulated, source and map tests') sees the new kernel — their tests count their matches
    exactly — nor this file's pattern theirs."""
    import test_insulated_isa
    import test_rmap_isa
    import test_source_isa
    assert div, "no tb_kernel_div instance in the library"
    others_see = (isa_report.tb_params, isa_report.pipe_params, test_insulated_isa.ins_params, test_source_isa.src_params,
                  test_rmap_isa.var_params)
    assert all(f(k["name"]) is None for _, k in div for f in others_see)
    others = [k["name"] for k in isa_report.kernels(LIB) if any(f(k["name"]) for f in others_see)]
    assert others and all(div_params(nm) is None for nm in others)


def test_div_no_scratch_and_lds_fits_four_per_cu(div):
    assert div, "no tb_kernel_div instance in the library"
    for (dt, nv, depth, ring, ar), k in sorted(div, key=lambda x: x[0]):
        tag = (f"tb_kernel_div<{dt}, K={depth:2d}, {ARITH[ar]}>: vgpr {k['vgpr']:3d} agpr {k['agpr']:3d} "
               f"lds {k.get('lds', '?')} scratch {k['scratch']} waves/SIMD {k['waves_per_simd']}")
        print(tag)
        assert k["scratch"] == 0, tag
        assert k["lds"] == 2 * depth * 1024 and k["lds"] <= 40 * 1024, tag  # the two rings of K face rows


def test_clamp_is_the_depth_in_the_library(div):
    from heat2d.models.heat2d import HeatSolver
    assert div, "no tb_kernel_div instance in the library"
    D = depth_in_library(div)
    assert D >= 8
    for dtype in ("fp64", "fp32"):
        s = HeatSolver(problem(301, 4), dtype=dtype, backend="cpu", tb=24, faces=rough_faces(301, dtype))
        info = s.info()
        s.close()
        assert info["faces"]["max_tb"] == D and info["tb"] == D


def test_committed_isa_diff_shows_added_instances_only():
    """profiles/r11/faces/isa_diff.txt: the sorted one-line-per-instance report of every
    tb_kernel* instance, parent against this change — added lines only, all of them the new kernel."""
    lines = open(os.path.join(ROOT, "profiles", "r11", "faces", "isa_diff.txt")).read().splitlines()
    added = [ln for ln in lines if ln.startswith(">")]
    assert not [ln for ln in lines if ln.startswith("<")]
    assert len(added) == 64 and all(div_params(ln) for ln in added)
