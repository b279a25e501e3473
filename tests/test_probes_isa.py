"""The probe-cone kernel (probe_cone<T, MODE, AR>, csrc/kernels/probe_cone.hip) in the
built library's gfx950 code objects (no GPU needed): exactly the expected
instances, none with scratch, static LDS at most 64 KiB (two planes of 49 x 49
elements), a name pattern disjoint from the stencil kernels', and the committed
report that every tb_kernel* instance kept its registers, scratch and LDS.
Registers and occupancy are printed, not asserted."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_report  # noqa: E402

LIB = os.path.join(ROOT, "cuda-hip-mpi-heat-equation-test_amd", "_native", "libheat2d.so")
MODES = ("plain", "source", "map", "faces")
ARITH = ("exact", "fma", "jacobi")
# probe_cone<T, MODE, AR>
_CONE = re.compile(r"probe_coneI([df])Li(\d+)ELi(\d+)E")


def cone_params(mangled):
    m = _CONE.search(mangled)
    return ("fp64" if m.group(1) == "d" else "fp32", int(m.group(2)), int(m.group(3))) if m else None


@pytest.fixture(scope="module")
def cone(native):
    ks = [(cone_params(k["name"]), k) for k in isa_report.kernels(LIB)]
    return [(p, k) for p, k in ks if p]


def test_cone_instances_present(cone):
    """2 dtypes x (plain x {exact, fma, jacobi} + {source, map, faces} x {exact, fma}) = 18."""
    want = [(dt, mode, ar) for dt in ("fp32", "fp64") for mode in range(4) for ar in range(3 if mode == 0 else 2)]
    assert sorted(p for p, _ in cone) == sorted(want) and len(cone) == 18
    assert sum("probe_advance" in k["name"] for k in isa_report.kernels(LIB)) == 1


def test_cone_pattern_is_disjoint_from_the_stencil_kernels(cone):
    import test_faces_isa
    import test_insulated_isa
    import test_rmap_isa
    import test_source_isa
    assert cone, "no probe_cone instance in the library"
    others_see = (isa_report.tb_params, isa_report.pipe_params, test_insulated_isa.ins_params, test_source_isa.src_params,
                  test_rmap_isa.var_params, test_faces_isa.div_params)
    assert all(f(k["name"]) is None for _, k in cone for f in others_see)
    assert all("tb_kernel" not in k["name"] for _, k in cone)  # (tools/isa_report.py's default filter)
    others = [k["name"] for k in isa_report.kernels(LIB) if any(f(k["name"]) for f in others_see)]
    assert others and all(cone_params(nm) is None for nm in others)


def test_cone_no_scratch_and_lds_within_64k(cone):
    assert cone, "no probe_cone instance in the library"
    for (dt, mode, ar), k in sorted(cone, key=lambda x: x[0]):
        tag = (f"probe_cone<{dt}, {MODES[mode]}, {ARITH[ar]}>: vgpr {k['vgpr']:3d} agpr {k['agpr']:3d} sgpr {k['sgpr']:3d} "
               f"lds {k['lds']} scratch {k['scratch']} waves/SIMD {k['waves_per_simd']}")
        print(tag)
        assert k["scratch"] == 0, tag
        assert k["lds"] == 2 * 49 * 49 * (8 if dt == "fp64" else 4) and k["lds"] <= 64 * 1024, tag


def test_committed_isa_diff_is_empty():
    """profiles/r12/probes/isa_diff.txt: the diff of the sorted one-line-per-instance reports of
    every tb_kernel* instance (registers, scratch, LDS), parent against this change — no line:
    all 1332 instances keep their bytes."""
    assert open(os.path.join(ROOT, "profiles", "r12", "probes", "isa_diff.txt")).read().strip() == ""
