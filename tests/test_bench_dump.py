"""bench.py --dump-outputs: the writer of the last timed step's result (CPU tensors suffice)."""
import os

import numpy as np
import torch

import bench


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_results_are_written_whole(tmp_path):
    a = torch.arange(7, dtype=torch.float32) - 3
    b = torch.tensor([2 ** 40 + 1, -5], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path), (a, [b]))
    got = _load(tmp_path)
    assert sorted(got) == ["output0", "output1"]
    assert got["output0"].dtype == np.float32 and np.array_equal(got["output0"], a.numpy())
    assert got["output1"].dtype == np.float64 and np.array_equal(got["output1"], b.numpy().astype(np.float64))


def test_large_result_is_sampled_with_its_nonzeros(tmp_path, monkeypatch):
    n = 100003
    monkeypatch.setattr(bench, "DUMP_BUDGET", 48 * 1000)      # 2000 sampled entries, at most 2000 non-zeros
    x = torch.zeros(n)
    nz = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:1500].sort().values
    x[nz] = torch.randn(1500, generator=torch.Generator().manual_seed(4)) + 10
    d1, d2 = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(d1), x)
    bench.dump_outputs(str(d2), x.clone())
    got, again = _load(d1), _load(d2)
    assert sorted(got) == ["output_nonzero_index", "output_nonzero_value", "output_sample", "output_sample_index"]
    idx = got["output_sample_index"].astype(np.int64)
    assert idx.size == 2000 and np.all(np.diff(idx) >= 0) and idx.min() >= 0 and idx.max() < n
    assert np.array_equal(got["output_sample"], x.numpy()[idx])
    assert np.array_equal(got["output_nonzero_index"].astype(np.int64), nz.numpy())
    assert np.array_equal(got["output_nonzero_value"], x.numpy()[nz.numpy()])
    assert sum(v.nbytes for v in got.values()) <= 48 * 1000
    for k in got:                                             # the same positions from run to run
        assert got[k].tobytes() == again[k].tobytes()


def test_dense_large_result_writes_the_sample_only(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 48 * 1000)
    bench.dump_outputs(str(tmp_path), torch.ones(100003, dtype=torch.float64))
    got = _load(tmp_path)
    assert sorted(got) == ["output_sample", "output_sample_index"]
    assert got["output_sample"].dtype == np.float64 and got["output_sample"].size == 48 * 1000 // 32
