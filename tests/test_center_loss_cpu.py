"""The host side of the fused CenterHead loss (csrc/center_loss.hip; mssvt_amd/center_head.py: center_loss,
CenterHead.fused_loss): the entry points are declared and exported, the constants mirrored in Python and in the tests are
the header's, argument errors are status codes before any launch, CPU tensors raise, and the default path is untouched."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import center_loss_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "mssvt_hip.h")) as f:
        return f.read()


def _define(name):
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, _header()).group(1))


def test_header_declares_and_library_exports_the_three_entry_points():
    from mssvt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = _lib.lib()
    for ret, name, params in (("long long", "mssvt_center_loss_workspace_bytes", 6), ("int", "mssvt_center_loss_forward", 29),
                              ("int", "mssvt_center_loss_backward", 37)):
        m = re.search(r"\b%s\s+%s\s*\(([^;{]*?)\)\s*;" % (ret, name), src, flags=re.S)
        assert m is not None, name
        assert m.group(1).count(",") + 1 == params, name
        assert m.group(1).strip().endswith("void *stream") or name.endswith("bytes"), name  # the stream goes last
        fn = getattr(lib, name)
        assert len(fn.argtypes) == params
        assert fn.restype is (ctypes.c_longlong if ret == "long long" else ctypes.c_int)
    assert lib.mssvt_hip_abi_version() == 100  # an additive change


def test_python_and_test_constants_are_the_headers():
    from mssvt_amd import center_head
    assert center_head.CENTER_LOSS_SWEEP == cases.SWEEP == _define("MSSVT_CENTER_LOSS_SWEEP")
    assert center_head.CENTER_LOSS_MAX_BLOCKS == cases.MAX_BLOCKS == _define("MSSVT_CENTER_LOSS_MAX_BLOCKS")
    assert center_head.CENTER_LOSS_MAX_OBJS == _define("MSSVT_CENTER_LOSS_MAX_OBJS")
    assert center_head.CENTER_LOSS_MAX_CODE == _define("MSSVT_CENTER_LOSS_MAX_CODE")


def test_workspace_query_follows_the_grid_and_refuses_shapes_beyond_the_limits():
    from mssvt_amd import _lib
    q = _lib.lib().mssvt_center_loss_workspace_bytes
    per_block = 3 * 8  # pos, neg, num_pos as doubles
    assert q(1, 1, 1, 1, 1, 8) == per_block
    assert q(1, 1, 32, 32, 8, 8) == per_block and q(1, 1, 25, 41, 8, 8) == 2 * per_block
    assert q(1, 1, 12, 174763, 8, 8) == cases.MAX_BLOCKS * per_block == q(4, 3, 470, 470, 500, 8)  # capped
    assert q(1, 1, 4, 4, 4096, 16) > 0
    for shape in ((1, 1, 4, 4, 4097, 8), (1, 1, 4, 4, 4, 17), (2, 1, 32768, 32768, 4, 8), (0, 1, 4, 4, 4, 8), (1, 1, 4, 4, 0, 8),
                  (1, 1, 4, 4, 4, 0), (1, -1, 4, 4, 4, 8)):
        assert q(*shape) <= 0, shape


def test_argument_errors_are_status_codes_before_any_launch():
    """the raw library, as tests/test_abi_cpu.py::test_argument_errors_are_status_codes_not_exits calls it: no GPU here, so
    a status can only come from the checks in front of the first HIP call"""
    from mssvt_amd import build
    lib = ctypes.CDLL(build.build())
    null, i, f = ctypes.c_void_p(0), ctypes.c_int, ctypes.c_float
    buf = ctypes.create_string_buffer(64)
    some = ctypes.c_void_p(ctypes.addressof(buf))  # never dereferenced on the host
    dims = [i(1), i(1), i(4), i(4), i(4), i(8), i(9)]
    no_maps = [null, i(0)] * 6
    maps = [some, i(2), some, i(1), some, i(3), some, i(2), null, i(0), null, i(0)]
    fwd, bwd = lib.mssvt_center_loss_forward, lib.mssvt_center_loss_backward
    assert fwd(*dims, null, null, *no_maps, null, null, null, null, f(1.0), null, null, null) == -1
    assert bwd(*dims, null, null, *no_maps, null, null, null, null, f(1.0), null, null, null, null, *([null] * 6), null) == -1
    for hole in range(8):  # each required pointer on its own
        ptrs = [some] * 8
        ptrs[hole] = null
        hm, heatmap, tb, inds, masks, cw, ws, out = ptrs
        assert fwd(*dims, hm, heatmap, *maps, tb, inds, masks, cw, f(1.0), ws, out, null) == -1, hole
    # sizes: the channels do not add up to code_size, a map with channels and no pointer, target rows shorter than the code
    bad_sum = [some, i(2), some, i(1), some, i(3), some, i(1), null, i(0), null, i(0)]
    no_ptr = [some, i(2), null, i(1), some, i(3), some, i(2), null, i(0), null, i(0)]
    assert fwd(*dims, some, some, *bad_sum, some, some, some, some, f(1.0), some, some, null) == -1
    assert fwd(*dims, some, some, *no_ptr, some, some, some, some, f(1.0), some, some, null) == -1
    short = dims[:6] + [i(7)]
    assert fwd(*short, some, some, *maps, some, some, some, some, f(1.0), some, some, null) == -1
    empty = [i(1), i(1), i(4), i(4), i(0), i(8), i(9)]
    assert fwd(*empty, some, some, *maps, some, some, some, some, f(1.0), some, some, null) == -1
    # limits are a status of their own
    many = [i(1), i(1), i(4), i(4), i(4097), i(8), i(9)]
    assert fwd(*many, some, some, *maps, some, some, some, some, f(1.0), some, some, null) == -2
    assert bwd(*many, some, some, *maps, some, some, some, some, f(1.0), some, null, null, null, *([null] * 6), null) == -2


def test_center_loss_refuses_cpu_tensors():
    from mssvt_amd import _lib, center_head
    c = cases.make_case("tail_only")
    with pytest.raises(_lib.MssvtHipError, match="no CPU path"):
        center_head.center_loss(torch.from_numpy(c["hm"]), [torch.from_numpy(m) for m in c["maps"]], torch.from_numpy(c["heatmap"]),
                                torch.from_numpy(c["target_boxes"]), torch.from_numpy(c["inds"]), torch.from_numpy(c["masks"]),
                                c["code_weights"], c["loc_weight"])


def test_fused_loss_is_off_by_default_and_cpu_predictions_keep_the_torch_path(golden_dir):
    from tests.test_head_train_cpu import _step
    d, head = _step(golden_dir, "cpu")
    assert head.fused_loss is False
    want, want_tb = head.get_loss()
    head.fused_loss = True  # predictions on the CPU: the existing expressions, floats in tb_dict
    loss, tb = head.get_loss()
    assert torch.equal(loss, want) and tb == want_tb and all(isinstance(v, float) for v in tb.values())
    assert abs(float(loss.detach()) - float(d["loss"])) <= 1e-5 * float(d["loss"])
    assert set(tb) == set(json.loads(str(d["tb_json"])))


def test_detector_returns_the_loss_as_a_tensor_with_fused_loss():
    """CenterPoint.forward: loss_rpn is loss.detach() with the attribute set and loss.item() without it"""
    from mssvt_amd.centerpoint import CenterPoint

    class Head(torch.nn.Module):
        fused_loss = False

        def get_loss(self):
            return torch.tensor(2.5, requires_grad=True) * 2, {"rpn_loss": 5.0}

    det = CenterPoint.__new__(CenterPoint)
    torch.nn.Module.__init__(det)
    det.module_list, det.dense_head = [], Head()
    det.train()
    ret, tb, _ = det(dict())
    assert isinstance(tb["loss_rpn"], float) and tb["loss_rpn"] == 5.0 and ret["loss"].requires_grad
    det.dense_head.fused_loss = True
    ret, tb, _ = det(dict())
    assert torch.is_tensor(tb["loss_rpn"]) and not tb["loss_rpn"].requires_grad and float(tb["loss_rpn"]) == 5.0
    assert np.isclose(float(ret["loss"]), 5.0)
