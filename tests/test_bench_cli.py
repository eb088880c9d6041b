"""CPU: bench.py's command line and its output dump (no GPU): a plain run is the headline alone (``--full`` off by
default), ``--dump-outputs`` writes float32 / float64 ``.npy`` files within the size limit, and the dumped sample of a
large output is the same rows on every run."""

import numpy as np
import pytest

import bench


def test_plain_run_is_the_default_and_full_is_opt_in():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    b = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert b.full and b.dump_outputs == "somewhere"


def test_sample_rows_is_fixed_sorted_and_within_budget():
    assert bench._sample_rows(5, 100, 1000).tolist() == [0, 1, 2, 3, 4]  # everything fits: every row
    r1 = bench._sample_rows(4096, 1000, 64000)
    r2 = bench._sample_rows(4096, 1000, 64000)
    assert r1.tolist() == r2.tolist()  # the same rows on every run
    assert len(r1) == 64 and len(set(r1.tolist())) == 64
    assert (np.diff(r1) > 0).all() and r1.min() >= 0 and r1.max() < 4096
    assert len(bench._sample_rows(10, 1 << 30, 1)) == 1  # never empty


def test_dump_outputs_writes_npy_and_enforces_dtype_and_size(tmp_path):
    arrays = {"a": np.arange(6, dtype=np.float32).reshape(2, 3), "b": np.asarray([1.5, 2.5])}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    for name, ref in arrays.items():
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype == ref.dtype and np.array_equal(got, ref)
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path / "bad"), {"t": np.arange(3, dtype=np.int32)})
    too_big = np.lib.stride_tricks.as_strided(np.zeros(1, dtype=np.float32), shape=(bench.DUMP_LIMIT // 4 + 1,),
                                              strides=(0,))
    with pytest.raises(RuntimeError):
        bench.dump_outputs(str(tmp_path / "big"), {"t": too_big})
    assert not (tmp_path / "big").exists()
