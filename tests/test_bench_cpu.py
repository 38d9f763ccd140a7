"""bench.py --dump-outputs on the host: which arrays of a step's output are written, in which types, and the seeded sample
that keeps a large output under the size limit."""
import os
from unittest import mock

import numpy as np
import torch

with mock.patch.dict(os.environ):  # (bench sets HIP_FORCE_DEV_KERNARG for its own process at import: not for this one)
    import bench
from mssvt_amd.mssvt_utils import SparseTensor


def test_output_arrays_skip_the_inputs_and_convert_types():
    feats, idx = torch.randn(5, 3), torch.arange(20, dtype=torch.int32).view(5, 4)
    sp = SparseTensor.__new__(SparseTensor)
    sp.features, sp.indices = feats, idx
    out = dict(voxel_features=torch.zeros(2), voxel_coords=torch.zeros(2, dtype=torch.int32), batch_size=1,
               encoded_spconv_tensor=sp, encoded_spconv_tensor_stride=1, loss=torch.tensor(2.5, dtype=torch.float64),
               half=torch.ones(3, dtype=torch.float16))
    arrays = bench.output_arrays(out, {"voxel_features", "voxel_coords", "batch_size"})
    assert sorted(arrays) == ["encoded_spconv_tensor.features", "encoded_spconv_tensor.indices", "half", "loss"]
    assert arrays["encoded_spconv_tensor.features"].dtype == np.float32
    np.testing.assert_array_equal(arrays["encoded_spconv_tensor.features"], feats.numpy())
    assert arrays["encoded_spconv_tensor.indices"].dtype == np.float64
    np.testing.assert_array_equal(arrays["encoded_spconv_tensor.indices"], idx.numpy())
    assert arrays["loss"].dtype == np.float64 and arrays["half"].dtype == np.float32


def test_dump_outputs_whole_and_sampled(tmp_path):
    rng = np.random.default_rng(3)
    arrays = {"a": rng.standard_normal((1000, 16)).astype(np.float32), "b": rng.standard_normal((1000, 16))}
    bench.dump_outputs(arrays, str(tmp_path / "whole"))
    assert sorted(os.listdir(tmp_path / "whole")) == ["a.npy", "b.npy"]
    for k, v in arrays.items():
        np.testing.assert_array_equal(np.load(tmp_path / "whole" / (k + ".npy")), v)
    limit = 60000
    for d in ("s1", "s2"):
        bench.dump_outputs(arrays, str(tmp_path / d), limit=limit)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == ["a.index.npy", "a.npy", "b.index.npy", "b.npy"]
    assert sum(os.path.getsize(tmp_path / "s1" / f) for f in files) <= limit + 4 * 256  # (+ the .npy headers)
    for k, v in arrays.items():
        pos = np.load(tmp_path / "s1" / (k + ".index.npy"))
        got = np.load(tmp_path / "s1" / (k + ".npy"))
        assert got.dtype == v.dtype and 0 < got.size < v.size and pos.dtype == np.float64
        np.testing.assert_array_equal(got, v.reshape(-1)[pos.astype(np.int64)])
        np.testing.assert_array_equal(pos, np.load(tmp_path / "s2" / (k + ".index.npy")))  # a fixed, seeded sample
    np.testing.assert_array_equal(np.load(tmp_path / "s1" / "a.index.npy"), np.load(tmp_path / "s1" / "b.index.npy"))
