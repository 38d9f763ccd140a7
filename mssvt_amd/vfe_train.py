"""DynamicVFE's training step on HIP run kernels (csrc/vfe_train.hip): points GROUPED BY VOXEL, a voxel's points a contiguous
run of rows; no float atomics, every sum in a fixed order -- values and gradients are bit-identical run to run.

    g = group_points(point_voxel, num_voxels)     order / run_off / sizes [N, P'] / row_voxel, nothing read back
    x = augment(points, g, rows, N, ...)          the (P', in_channels) PFN input, forward only
    y = run_max_concat(x, run_off)                (P', F) -> (P', 2F): [x ; max over the row's run]   (PFNLayerV2's max + concat)
    m = run_max(x, run_off)                       (P', F) -> (N, F)                                   (the voxel features)

(ref pcdet/models/backbones_3d/vfe/dynamic_vfe.py:71-131; the gradient of a maximum is split equally between the rows that
attain it exactly, as ``scatter_reduce("amax")`` and oracle/gen_golden_vfe.py do.)  None of these calls waits for the host.
"""
import collections
import functools

import torch

from . import _lib

CHUNK = 128      # MSSVT_VFE_TRAIN_CHUNK: a run of more rows is reduced in pieces by separate lane groups
MAX_WIDTH = 256  # F: a multiple of 4 up to this

Groups = collections.namedtuple("Groups", "order run_off sizes row_voxel")


def supported_width(F):
    return 4 <= F <= MAX_WIDTH and F % 4 == 0


@functools.lru_cache(maxsize=64)
def _group_workspace_bytes(P, cap):
    n = int(_lib.lib().mssvt_vfe_group_workspace_bytes(P, cap))
    if n <= 0:
        raise _lib.MssvtHipError("mssvt_vfe_group_workspace_bytes(%d, %d) refused the size" % (P, cap))
    return n


def group_points(point_voxel, num_voxels):
    """point_voxel (P,) int32 from the voxelizer (-1: outside the grid); num_voxels: an int, or the 1-element int32 device
    tensor the voxelizer left (then the tables have room for P voxels and N stays on the device).

    Returns Groups(order (P,), run_off (capacity + 1,), sizes (2,) = [N, P'], row_voxel (P,)), all int32 on the device:
    ``order[:P']`` the original index of every kept point sorted by voxel and, inside a voxel, by ascending point index;
    rows ``run_off[v]:run_off[v + 1]`` are voxel v's (an id no point carries: an empty run); ``row_voxel[:P']`` the voxel of
    every row.  ``sizes`` is what a training step reads back, once, to size its tensors."""
    assert point_voxel.is_cuda and point_voxel.dtype == torch.int32 and point_voxel.dim() == 1
    point_voxel = point_voxel.contiguous()
    P, dev = point_voxel.shape[0], point_voxel.device
    n_dev = None
    if torch.is_tensor(num_voxels):
        assert num_voxels.is_cuda and num_voxels.dtype == torch.int32 and num_voxels.numel() == 1
        n_dev, cap = num_voxels, P
    else:
        cap = int(num_voxels)
    order = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    row_voxel = torch.empty(max(P, 1), dtype=torch.int32, device=dev)
    run_off = torch.empty(cap + 1, dtype=torch.int32, device=dev)
    sizes = torch.empty(2, dtype=torch.int32, device=dev)
    nbytes = _group_workspace_bytes(P, cap)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("mssvt_vfe_group", _lib.ptr(point_voxel), P, cap, _lib.ptr(n_dev), _lib.ptr(order), _lib.ptr(row_voxel),
              _lib.ptr(run_off), _lib.ptr(sizes), _lib.ptr(ws), nbytes, _lib.stream())
    return Groups(order[:P], run_off, sizes, row_voxel[:P])


def augment(points, groups, num_rows, num_voxels, voxel_coords, voxel_size, offset, num_point_features,
            with_cluster_center=True, with_voxel_center=True, with_distance=False):
    """The PFN input of the grouped rows (ref dynamic_vfe.py:96-112), (num_rows, in_channels) f32: row r is point
    ``groups.order[r]``: [its features, xyz - cluster centre, xyz - voxel centre, |xyz|].  voxel_coords (>= num_voxels, 4)
    int32 [b, z, y, x]; offset = voxel_size / 2 + range_min.  Forward only: points carry no gradient."""
    assert points.is_cuda and points.dtype == torch.float32 and points.is_contiguous() and not points.requires_grad
    P, stride = points.shape
    C = num_point_features + (3 if with_cluster_center else 0) + (3 if with_voxel_center else 0) + (1 if with_distance else 0)
    out = torch.empty((num_rows, C), dtype=torch.float32, device=points.device)
    mean3 = torch.empty((max(num_voxels, 1), 3), dtype=torch.float32, device=points.device) if with_cluster_center else None
    _lib.call("mssvt_vfe_augment", _lib.ptr(points), stride, P, _lib.ptr(groups.order), _lib.ptr(groups.row_voxel),
              _lib.ptr(groups.run_off), num_rows, num_voxels, _lib.ptr(voxel_coords), _lib.f3(voxel_size), _lib.f3(offset),
              num_point_features, int(bool(with_cluster_center)), int(bool(with_voxel_center)), int(bool(with_distance)),
              _lib.ptr(mean3), _lib.ptr(out), _lib.stream())
    return out


def _rows(x):
    """a contiguous float32 device matrix whose rows sit on 16-byte boundaries"""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2):
        raise _lib.MssvtHipError("the run kernels take float32 matrices on the GPU")
    x = x.contiguous()
    return x.clone() if x.data_ptr() % 16 else x


def _parts(rows, F, dev):
    return torch.empty(int(_lib.lib().mssvt_vfe_run_parts_floats(rows, F)), dtype=torch.float32, device=dev)


def _forward(x, run_off, concat):
    x = _rows(x.detach())
    assert run_off.is_cuda and run_off.dtype == torch.int32 and run_off.dim() == 1 and run_off.numel() >= 1
    run_off = run_off.contiguous()
    rows, F = x.shape
    N = run_off.numel() - 1
    out = torch.empty((rows, 2 * F) if concat else (N, F), dtype=torch.float32, device=x.device)
    _lib.call("mssvt_vfe_run_max_forward", _lib.ptr(x), _lib.ptr(run_off), rows, N, F, int(concat),
              _lib.ptr(_parts(rows, F, x.device)), _lib.ptr(out), _lib.stream())
    return x, run_off, out


def _backward(saved, maxima, grad_out, run_off, rows, F, concat):
    grad_out = _rows(grad_out)
    gx = torch.empty((rows, F), dtype=torch.float32, device=grad_out.device)
    _lib.call("mssvt_vfe_run_max_backward", _lib.ptr(saved), _lib.ptr(maxima), _lib.ptr(grad_out), _lib.ptr(run_off), rows,
              run_off.numel() - 1, F, int(concat), _lib.ptr(_parts(rows, F, gx.device)), _lib.ptr(gx), _lib.stream())
    return gx


class RunMaxConcat(torch.autograd.Function):
    """(P', F) -> (P', 2F): [x ; max over the row's run of x].  The output holds both x and the broadcast maximum: it is all the
    backward needs."""

    @staticmethod
    def forward(ctx, x, run_off):
        _, run_off, out = _forward(x, run_off, True)
        ctx.save_for_backward(out, run_off)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        out, run_off = ctx.saved_tensors
        rows, F = out.shape[0], out.shape[1] // 2
        return _backward(out, None, grad_out, run_off, rows, F, True), None


class RunMax(torch.autograd.Function):
    """(P', F) -> (N, F): the maximum over every run; an empty run gives a zero row and no gradient."""

    @staticmethod
    def forward(ctx, x, run_off):
        x, run_off, out = _forward(x, run_off, False)
        ctx.save_for_backward(x, out, run_off)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, out, run_off = ctx.saved_tensors
        return _backward(x, out, grad_out, run_off, x.shape[0], x.shape[1], False), None


def run_max_concat(x, run_off):
    return RunMaxConcat.apply(x, run_off)


def run_max(x, run_off):
    return RunMax.apply(x, run_off)
