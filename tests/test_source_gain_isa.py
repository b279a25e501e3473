"""The gain-schedule kernels (tb_kernel_gain, csrc/kernels/tb_impl.hpp; probe_cone_gain,
csrc/kernels/probe_cone.hip) in the built library's gfx950 code objects (no GPU needed):
exactly 64 tb_kernel_gain instances (2 dtypes x depths 1..16 x exact / fma, ring 4), none with
scratch, each with the LDS of the tb_kernel_src instance of the same dtype, depth and form; a
name pattern disjoint from every other kernel's; 4 probe_cone_gain instances; and the committed
report that every tb_kernel* instance of the parent kept its registers, scratch and LDS.
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
ARITH = ("exact", "fma")
# tb_kernel_gain<T, NV, K, RING, AR>
_GAIN = re.compile(r"tb_kernel_gainI([df])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")
# probe_cone_gain<T, AR>
_CONE = re.compile(r"probe_cone_gainI([df])Li(\d+)E")


def gain_params(mangled):
    m = _GAIN.search(mangled)
    return ("fp64" if m.group(1) == "d" else "fp32", int(m.group(2)), int(m.group(3)), int(m.group(4)),
            int(m.group(5))) if m else None


def cone_gain_params(mangled):
    m = _CONE.search(mangled)
    return ("fp64" if m.group(1) == "d" else "fp32", int(m.group(2))) if m else None


@pytest.fixture(scope="module")
def kernels(native):
    return isa_report.kernels(LIB)


@pytest.fixture(scope="module")
def gain(kernels):
    return [(gain_params(k["name"]), k) for k in kernels if gain_params(k["name"])]


def others_see():
    import test_faces_isa
    import test_insulated_isa
    import test_probes_isa
    import test_rmap_isa
    import test_source_isa
    return (isa_report.tb_params, isa_report.pipe_params, test_insulated_isa.ins_params, test_source_isa.src_params,
            test_rmap_isa.var_params, test_faces_isa.div_params, test_probes_isa.cone_params)


def test_gain_instances_present(gain):
    want = [(dt, 1, k, 4, ar) for dt in ("fp32", "fp64") for k in range(1, 17) for ar in range(2)]
    assert sorted(p for p, _ in gain) == sorted(want) and len(gain) == 64


def test_gain_no_scratch_and_the_source_kernels_lds(gain, kernels):
    import test_source_isa
    src = {test_source_isa.src_params(k["name"]): k for k in kernels if test_source_isa.src_params(k["name"])}
    assert gain, "no tb_kernel_gain instance in the library"
    for p, k in sorted(gain, key=lambda x: x[0]):
        dt, nv, depth, ring, ar = p
        tag = (f"tb_kernel_gain<{dt}, K={depth:2d}, {ARITH[ar]}>: vgpr {k['vgpr']:3d} agpr {k['agpr']:3d} sgpr {k['sgpr']:3d} "
               f"lds {k['lds']} scratch {k['scratch']} waves/SIMD {k['waves_per_simd']} "
               f"(tb_kernel_src: vgpr {src[p]['vgpr']} agpr {src[p]['agpr']} waves/SIMD {src[p]['waves_per_simd']})")
        print(tag)
        assert k["scratch"] == 0, tag
        assert k["lds"] == src[p]["lds"] == max(depth, 1) * 1024, tag


def test_patterns_are_mutually_disjoint(gain, kernels):
    """The new patterns see none of the existing kernels and no existing pattern sees the new
    kernels (several ISA tests count their matches exactly)."""
    assert gain, "no tb_kernel_gain instance in the library"
    cones = [k for k in kernels if cone_gain_params(k["name"])]
    for k in [k for _, k in gain] + cones:
        assert all(f(k["name"]) is None for f in others_see()), k["name"]
    assert all(cone_gain_params(k["name"]) is None for _, k in gain)
    assert all(gain_params(k["name"]) is None for k in cones)
    old = [k["name"] for k in kernels if any(f(k["name"]) for f in others_see())]
    assert len(old) >= 1332 and all(gain_params(nm) is None and cone_gain_params(nm) is None for nm in old)
    assert sum("probe_advance" in k["name"] for k in kernels) == 1
    assert sum("gain_step" in k["name"] for k in kernels) == 1


def test_cone_gain_instances(kernels):
    cones = [(cone_gain_params(k["name"]), k) for k in kernels if cone_gain_params(k["name"])]
    assert sorted(p for p, _ in cones) == sorted((dt, ar) for dt in ("fp32", "fp64") for ar in range(2))
    for (dt, ar), k in sorted(cones, key=lambda x: x[0]):
        tag = (f"probe_cone_gain<{dt}, {ARITH[ar]}>: vgpr {k['vgpr']:3d} agpr {k['agpr']:3d} sgpr {k['sgpr']:3d} "
               f"lds {k['lds']} scratch {k['scratch']} waves/SIMD {k['waves_per_simd']}")
        print(tag)
        assert k["scratch"] == 0, tag
        assert k["lds"] == 2 * 49 * 49 * (8 if dt == "fp64" else 4) and k["lds"] <= 64 * 1024, tag


def test_committed_isa_diff_adds_only_the_new_kernels():
    """profiles/r13/gain/isa_diff.txt: the diff of the sorted one-line-per-instance reports of every
    tb_kernel* instance (registers, scratch), parent against this change: 64 added lines, all of
    them tb_kernel_gain, none removed or changed — a solver without a gain launches what it did."""
    lines = open(os.path.join(ROOT, "profiles", "r13", "gain", "isa_diff.txt")).read().splitlines()
    added = [ln for ln in lines if ln.startswith(">")]
    assert not [ln for ln in lines if ln.startswith("<")]
    assert len(added) == 64 and all(gain_params(ln) for ln in added)
    assert all(re.fullmatch(r"\d+a\d+(,\d+)?", ln) for ln in lines if not ln.startswith(">"))
