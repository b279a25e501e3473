"""The wave-pair interior kernels (tb_kernel_pipe, csrc/kernels/
tb_pipe_impl.hpp) in the built library's gfx950 code objects (no GPU needed):
every instance must keep 2 waves per SIMD without scratch, and its static LDS
(two pairs' row FIFOs) must leave room for 2 workgroups per CU — a depth that
does not is not shipped."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_report  # noqa: E402

LIB = os.path.join(ROOT, "cuda-hip-mpi-heat-equation-test_amd", "_native", "libheat2d.so")
LDS_PER_CU = 160 * 1024  # gfx950
ARITH = ("exact", "fma", "jacobi", "fast")


@pytest.fixture(scope="module")
def pipes(native):
    ks = [(isa_report.pipe_params(k["name"]), k) for k in isa_report.kernels(LIB)]
    return [(p, k) for p, k in ks if p]


def test_pipe_instances_present(pipes):
    """fp64, depths 16..24, all four arithmetic forms: one instance each."""
    assert sorted(p for p, _ in pipes) == [(k, ar) for k in range(16, 25) for ar in range(4)]


def test_pipe_pattern_is_disjoint_from_tb_kernel(pipes):
    """tools/isa_report.py's tb_kernel pattern must not see the pair kernel
    (tests/test_isa.py counts its matches exactly)."""
    assert all(isa_report.tb_params(k["name"]) is None for _, k in pipes)


def test_pipe_two_waves_per_simd_no_scratch(pipes):
    for (depth, ar), k in pipes:
        tag = f"tb_kernel_pipe<K={depth}, {ARITH[ar]}>: vgpr {k['vgpr']} agpr {k['agpr']} scratch {k['scratch']}"
        assert k["scratch"] == 0, tag
        assert k["vgpr"] <= 256 and k["waves_per_simd"] >= 2, tag  # .vgpr_count is the total (VGPRs + AGPRs)


def test_pipe_lds_allows_two_workgroups_per_cu(pipes):
    for (depth, ar), k in pipes:
        assert 0 < k["lds"] <= 64 * 1024, (depth, k["lds"])  # static LDS limit of one workgroup
        assert 2 * k["lds"] <= LDS_PER_CU, (depth, k["lds"])
