"""``DynamicVFE.fused_train`` without a GPU: on CPU tensors the module takes the torch branch and still reproduces the
reference's training step; every entry point of csrc/vfe_train.hip is declared in the header with its argument types (the
ABI tests of tests/test_abi_cpu.py then hold export and call sites to the header); the Python constants mirror the header."""
import ctypes
import os
import re

import numpy as np
import torch

from tests.test_vfe_train_cpu import _check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ENTRY_POINTS = {
    "mssvt_vfe_group_workspace_bytes": (ctypes.c_longlong, [ctypes.c_longlong, ctypes.c_int]),
    "mssvt_vfe_group": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int] + [ctypes.c_void_p] * 6 +
                        [ctypes.c_longlong, ctypes.c_void_p]),
    "mssvt_vfe_augment": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong] + [ctypes.c_void_p] * 3 +
                          [ctypes.c_int] * 2 + [ctypes.c_void_p] * 3 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3),
    "mssvt_vfe_run_parts_floats": (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int]),
    "mssvt_vfe_run_max_forward": (ctypes.c_int, [ctypes.c_void_p] * 2 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3),
    "mssvt_vfe_run_max_backward": (ctypes.c_int, [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3),
}


def test_fused_flag_on_cpu_tensors_takes_the_torch_branch(golden_dir, monkeypatch):
    from mssvt_amd.dynamic_vfe import DynamicVFE

    def never(self, batch_dict):
        raise AssertionError("the fused step needs the GPU")

    monkeypatch.setattr(DynamicVFE, "_forward_train_fused", never)
    d = np.load(os.path.join(golden_dir, "dynamic_vfe_train_32_64.npz"))
    cfg = dict(NUM_FILTERS=d["num_filters"].tolist(), WITH_CLUSTER_CENTER=True, WITH_VOXEL_CENTER=True, FUSED_TRAIN=True)
    vfe = DynamicVFE(cfg, 5, d["voxel_size"].tolist(), d["grid_size"].tolist(), d["point_cloud_range"].tolist())
    assert vfe.fused_train is True
    vfe.load_state_dict({k[3:]: torch.from_numpy(d[k]) for k in d.files if k.startswith("sd.")}, strict=True)  # same keys
    vfe.train()
    out = vfe(dict(points=torch.from_numpy(d["points"]), batch_size=int(d["batch_size"])))
    (out["voxel_features"] * torch.from_numpy(d["weight_of_the_loss"])).sum().backward()
    _check(d, vfe, out)


def test_every_new_entry_point_is_declared_with_its_argument_types():
    from mssvt_amd import _lib
    lib = _lib.lib()
    src = open(os.path.join(ROOT, "include", "mssvt_hip.h")).read()
    declared = set(re.findall(r"\b(mssvt_vfe_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))
    assert declared == set(ENTRY_POINTS), declared ^ set(ENTRY_POINTS)
    for name, (ret, args) in ENTRY_POINTS.items():
        fn = getattr(lib, name)
        assert fn.restype is ret, name
        assert list(fn.argtypes) == args, (name, fn.argtypes)


def test_python_constants_mirror_the_header_and_sizes_are_plain_arithmetic():
    from mssvt_amd import _lib, vfe_train
    src = open(os.path.join(ROOT, "include", "mssvt_hip.h")).read()
    from tests import vfe_train_ref
    assert int(re.search(r"#define MSSVT_VFE_TRAIN_CHUNK (\d+)", src).group(1)) == vfe_train.CHUNK == vfe_train_ref.CHUNK
    lib = _lib.lib()
    for rows in (0, 1, vfe_train.CHUNK, vfe_train.CHUNK + 1, 160000):
        windows = (rows + vfe_train.CHUNK - 1) // vfe_train.CHUNK
        assert lib.mssvt_vfe_run_parts_floats(rows, 64) == 2 * windows * 2 * 64 + 4
    assert lib.mssvt_vfe_run_parts_floats(-1, 64) == 0
    assert [vfe_train.supported_width(F) for F in (0, 4, 30, 64, 256, 260)] == [False, True, False, True, True, False]


def test_argument_errors_are_status_codes():
    from mssvt_amd import _lib
    lib = _lib.lib()
    assert lib.mssvt_vfe_run_max_forward(None, None, 8, 1, 30, 0, None, None, None) == -1  # width no multiple of 4
    assert lib.mssvt_vfe_run_max_forward(None, None, 8, 1, 260, 1, None, None, None) == -1
    assert lib.mssvt_vfe_run_max_forward(None, None, -1, 1, 64, 1, None, None, None) == -1
    assert lib.mssvt_vfe_run_max_forward(None, None, 8, 1, 64, 1, None, None, None) == -1  # null tables
    assert lib.mssvt_vfe_run_max_backward(None, None, None, None, 8, 1, 64, 1, None, None, None) == -1
    assert lib.mssvt_vfe_group(None, -1, 0, None, None, None, None, None, None, 0, None) == -1
    assert lib.mssvt_vfe_augment(None, 3, 10, None, None, None, 10, 1, None, None, None, 5, 1, 1, 0, None, None, None) == -1
    assert lib.mssvt_vfe_run_max_forward(None, None, 0, 0, 64, 1, None, None, None) == 0  # nothing to do
