"""bench.py --dump-outputs: the field the timed steps left, written as
DIR/field.npy — whole when it fits the dump budget, else a fixed sample of
whole rows that only depends on the field's shape."""
import importlib.util
import os

import numpy as np
import pytest

import heat2d
from heat2d.models import reference as R
from test_bench_contract import run_plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_driver", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_sample_rows(bench):
    assert np.array_equal(bench.sample_rows(100, 800), np.arange(100))
    assert np.array_equal(bench.sample_rows(12, 1 << 20, budget=12 << 20), np.arange(12))
    row_bytes = 32768 * 8
    rows = bench.sample_rows(32768, row_bytes)
    assert len(rows) == bench.DUMP_BYTES // row_bytes == 192 and len(rows) * row_bytes <= 64 * 10**6
    assert np.all(np.diff(rows) > 0) and rows[0] == 0 and rows[-1] == 32767
    # the frame's neighbourhood on both sides, the rest spread over the middle
    assert np.array_equal(rows[:48], np.arange(48)) and np.array_equal(rows[-48:], np.arange(32768 - 48, 32768))
    assert np.array_equal(rows, bench.sample_rows(32768, row_bytes))
    assert len(bench.sample_rows(13, 10, budget=80)) == 8  # one row over the budget: sampled


@pytest.mark.parametrize("nproc,dtype", [(1, "fp64"), (3, "fp32")])
def test_bench_dump_outputs_cpu(tmp_path, nproc, dtype):
    """The dumped field is the golden model's after warmup + steps steps,
    bitwise, whatever the rank count (rank 0 writes every rank's rows)."""
    out = tmp_path / "dump"
    d = run_plain("--backend", "cpu", "--gpus", str(nproc), "--grid", "100", "--steps", "12", "--warmup", "3", "--tb",
                  "4", "--dtype", dtype, "--dump-outputs", str(out))
    assert d["steps"] == 12 and d["verified"] is None and d["timed_field_check"] is None  # a plain run
    assert sorted(os.listdir(out)) == ["field.npy"]
    got = np.load(out / "field.npy")
    npdt = np.float64 if dtype == "fp64" else np.float32
    inp = heat2d.InputDat(n=100, sigma=0.25, nu=0.05, dom_len=1.0, ntime=15, soln=0, nfields=6)
    ref = R.owned(R.ftcs(heat2d.make_problem(inp, "ghost", "uniform"), dtype=npdt))
    assert got.dtype == npdt and got.shape == (100, 100) and np.array_equal(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp64", "fp32"])
def test_slab_rows_gpu(gpu, bench, dtype):
    """The sampled rows of a device field (runs of consecutive rows packed on
    the device) are those rows of the whole download."""
    from heat2d.models.heat2d import HeatSolver
    prob = heat2d.make_problem(heat2d.parse_input_text("700 0.25 0.05 1.0 9 0"), "ghost", "hat")
    with HeatSolver(prob, dtype=dtype, backend="hip", tb=4, device=gpu) as s:
        s.step(9)
        whole = s.download()
        for rows in ([0], [699], [0, 1, 2, 100, 300, 301, 698, 699], list(range(5, 699, 7))):
            rows = np.array(rows, dtype=np.int64)
            got = bench.slab_rows(s, rows, gpu)
            assert got.dtype == whole.dtype and np.array_equal(got, whole[rows]), rows
        assert np.array_equal(bench.slab_rows(s, np.arange(700), gpu), whole)
