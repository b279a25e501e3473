"""The five-weight kernels (tb_kernel_w5, csrc/kernels/tb_impl.hpp; probe_cone_w5,
csrc/kernels/probe_cone.hip) in the built library's gfx950 code objects (no GPU needed):
exactly 2 dtypes x 2 forms (exact, fma) x kMaxTBW5 tb_kernel_w5 instances, ring 4, none with
scratch, none with LDS; name patterns disjoint both ways from every other kernel's; 4
probe_cone_w5 instances without scratch, the other cone counts unchanged; and the committed
report that every tb_kernel* / probe_cone* instance of the parent kept its registers, scratch
and LDS. Registers and occupancy are printed, not asserted."""
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
# tb_kernel_w5<T, NV, K, RING, AR>
_W5 = re.compile(r"tb_kernel_w5I([df])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E")
# probe_cone_w5<T, AR>
_CONE = re.compile(r"probe_cone_w5I([df])Li(\d+)E")
DIFF = os.path.join(ROOT, "profiles", "r16", "weights", "isa_diff.txt")


def w5_params(mangled):
    m = _W5.search(mangled)
    return ("fp64" if m.group(1) == "d" else "fp32", int(m.group(2)), int(m.group(3)), int(m.group(4)),
            int(m.group(5))) if m else None


def cone_params(mangled):
    m = _CONE.search(mangled)
    return ("fp64" if m.group(1) == "d" else "fp32", int(m.group(2))) if m else None


@pytest.fixture(scope="module")
def kernels(native):
    return isa_report.kernels(LIB)


@pytest.fixture(scope="module")
def w5(kernels):
    return [(w5_params(k["name"]), k) for k in kernels if w5_params(k["name"])]


def test_w5_instances_present(w5):
    """Exactly 2 dtypes x 2 forms x kMaxTBW5 instances: every depth the clamp allows."""
    from heat2d.ops import _native as N
    assert w5, "no tb_kernel_w5 instance in the library"
    D = N.max_tb_w5()
    want = [(dt, 1, k, 4, ar) for dt in ("fp32", "fp64") for k in range(1, D + 1) for ar in range(2)]
    assert sorted(p for p, _ in w5) == sorted(want) and len(w5) == 2 * 2 * D


def test_w5_no_scratch_no_lds(w5):
    assert w5, "no tb_kernel_w5 instance in the library"
    for p, k in sorted(w5, key=lambda x: x[0]):
        dt, nv, depth, ring, ar = p
        tag = (f"tb_kernel_w5<{dt}, K={depth:2d}, {ARITH[ar]}>: vgpr {k['vgpr']:3d} agpr {k['agpr']:3d} sgpr {k['sgpr']:3d} "
               f"lds {k['lds']} scratch {k['scratch']} waves/SIMD {k['waves_per_simd']}")
        print(tag)
        assert k["scratch"] == 0, tag
        assert k["lds"] == 0, tag


def test_w5_patterns_are_disjoint_from_the_other_kernels(w5, kernels):
    """None of the existing patterns sees the new kernels — their tests count their matches exactly — nor
    these patterns theirs."""
    import test_faces_isa
    import test_insulated_isa
    import test_probes_isa
    import test_rmap_isa
    import test_robin_isa
    import test_source_gain_isa
    import test_source_isa
    assert w5, "no tb_kernel_w5 instance in the library"
    others_see = (isa_report.tb_params, isa_report.pipe_params, test_insulated_isa.ins_params, test_source_isa.src_params,
                  test_rmap_isa.var_params, test_faces_isa.div_params, test_source_gain_isa._GAIN.search,
                  test_source_gain_isa._CONE.search, test_probes_isa._CONE.search, test_robin_isa.rob_params,
                  test_robin_isa.cone_params)
    new = [k["name"] for _, k in w5] + [k["name"] for k in kernels if cone_params(k["name"])]
    assert len(new) == len(w5) + 4
    assert all(not f(nm) for nm in new for f in others_see)
    assert all("gain_step" not in nm and "probe_advance" not in nm for nm in new)
    others = [k["name"] for k in kernels if any(f(k["name"]) for f in others_see)]
    assert others and all(w5_params(nm) is None and cone_params(nm) is None for nm in others)


def test_probe_cone_w5_instances(kernels):
    """2 dtypes x exact / fma, no scratch; the other cone kernels keep their counts."""
    import test_probes_isa
    import test_robin_isa
    import test_source_gain_isa
    cone = [(cone_params(k["name"]), k) for k in kernels if cone_params(k["name"])]
    assert sorted(p for p, _ in cone) == [(dt, ar) for dt in ("fp32", "fp64") for ar in range(2)]
    for (dt, ar), k in cone:
        tag = f"probe_cone_w5<{dt}, {ARITH[ar]}>: vgpr {k['vgpr']} sgpr {k['sgpr']} lds {k['lds']} scratch {k['scratch']}"
        print(tag)
        assert k["scratch"] == 0, tag
    assert sum(1 for k in kernels if test_source_gain_isa._CONE.search(k["name"])) == 4
    assert sum(1 for k in kernels if test_robin_isa._CONE.search(k["name"])) == 4
    assert sum(1 for k in kernels if test_probes_isa._CONE.search(k["name"])) == 18  # 2 dtypes x (plain: 3 forms, 3 modes: 2 each)


def test_committed_isa_diff_shows_added_instances_only():
    """profiles/r16/weights/isa_diff.txt: the sorted one-line-per-instance report of every tb_kernel* and
    probe_cone* instance (name, registers, scratch, LDS), parent against this change — added lines only, all of
    them tb_kernel_w5 or probe_cone_w5."""
    from heat2d.ops import _native as N
    lines = open(DIFF).read().splitlines()
    added = [ln for ln in lines if ln.startswith(">")]
    assert not [ln for ln in lines if ln.startswith("<")]
    assert len(added) == 4 * N.max_tb_w5() + 4 and all(w5_params(ln) or cone_params(ln) for ln in added)
    assert all(re.fullmatch(r"\d+a\d+(,\d+)?", ln) for ln in lines if not ln.startswith(">"))
