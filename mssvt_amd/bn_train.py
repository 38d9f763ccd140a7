"""BatchNorm2d in TRAINING mode with the ReLU behind it on HIP kernels (csrc/bn_train.hip): the layer that follows every
convolution of HeightCompression and BaseBEVBackbone.

``BnReluFunction`` is ``y = relu(batch_norm(x))`` (the ReLU optional) on channels-last fp32 GPU tensors with a hand-written
backward: three launches forward (per-piece statistics with one read of x, their merge in piece order, normalise + ReLU) and
three backward (per-piece sums of g and g xhat, their merge, dx).  The backward recomputes the ReLU mask from x with the
forward's own expression, so y is neither saved nor read.  There are no float atomics: the results are bit-identical from
step to step.  The running buffers are updated by the forward's merge launch, in place.

``ROUTED_BN`` lists the channel counts the modules send here when ``fused_train`` and ``fused_bn`` are both on: exactly those
whose slowest forward + backward beat the library's fastest, over NCHW and channels-last, at every timed shape of that width
and at B = 1 and B = 4 in tools/time_bev_bn_train.py (profiles/bev_bn_train_times.json, DESIGN section 5.5's rule).  Every
covered width stays reachable through the Function.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, bev_conv
from ._lib import MssvtHipError

CHANNELS = (32, 64, 128, 256)
# channel counts that cleared the routing rule on an MI355X (profiles/bev_bn_train_times.json): 128 did at (128, 470 x 470),
# B = 1 and B = 4; 256 cleared it at four of its five timed points and lost at (256, 235 x 235), B = 1 (0.114 .. 0.253 ms
# against the library's fastest 0.114 ms), so it stays out and reachable through the Function
ROUTED_BN = frozenset({128})
# the narrow widths exist for small module tests: never timed, routed whenever the switch is on
NARROW_CHANNELS = frozenset({32, 64})


def piece_rows(C):
    """Rows per piece of the statistics / reduction kernels for this width (0: not covered)."""
    return int(_lib.lib().mssvt_bn_train_piece_rows(C))


def workspace_bytes(P, C):
    n = int(_lib.lib().mssvt_bn_train_workspace_bytes(P, C))
    if n <= 0:
        raise MssvtHipError("mssvt_bn_train_workspace_bytes(%d, %d) refused the size" % (P, C))
    return n


def _nhwc(t):
    return t if bev_conv.is_channels_last(t) else t.contiguous(memory_format=torch.channels_last)


class BnReluFunction(torch.autograd.Function):
    """``BnReluFunction.apply(x, weight, bias, running_mean, running_var, eps, momentum, relu)``: x (B, C, H, W) fp32 on the
    GPU (made channels-last); returns ``(y, running_mean, running_var)``, the two buffers updated in place (declared dirty,
    not differentiable)."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, momentum, relu):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            raise MssvtHipError("bn_train.BnReluFunction needs a 4-D fp32 GPU tensor (no CPU path)")
        x = _nhwc(x)
        B, C, H, W = x.shape
        P = B * H * W
        vectors = [weight.detach(), bias.detach(), running_mean, running_var]
        for v in vectors:
            if not (v.is_cuda and v.device == x.device and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == C):
                raise MssvtHipError("bn_train.BnReluFunction: weight, bias and the running buffers must be contiguous fp32 (%d,) on %s" % (C, x.device))
        y = torch.empty_like(x)  # channels-last, as x
        save_mean = torch.empty(C, dtype=torch.float32, device=x.device)
        save_invstd = torch.empty(C, dtype=torch.float32, device=x.device)
        workspace = torch.empty(workspace_bytes(P, C), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call("mssvt_bn_train_fwd", x.data_ptr(), P, C, vectors[0].data_ptr(), vectors[1].data_ptr(), float(eps),
                      float(momentum), running_mean.data_ptr(), running_var.data_ptr(), int(bool(relu)), y.data_ptr(),
                      save_mean.data_ptr(), save_invstd.data_ptr(), workspace.data_ptr(), _lib.stream())
        ctx.mark_dirty(running_mean, running_var)
        ctx.mark_non_differentiable(running_mean, running_var)
        ctx.save_for_backward(x, weight, bias, save_mean, save_invstd)
        ctx.relu = bool(relu)
        return y, running_mean, running_var

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, _drm, _drv):
        x, weight, bias, save_mean, save_invstd = ctx.saved_tensors
        B, C, H, W = x.shape
        P = B * H * W
        dy = _nhwc(dy)
        dx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        workspace = torch.empty(workspace_bytes(P, C), dtype=torch.uint8, device=x.device)
        with torch.cuda.device(x.device):
            _lib.call("mssvt_bn_train_bwd", x.data_ptr(), dy.data_ptr(), P, C, weight.data_ptr(), bias.data_ptr(),
                      save_mean.data_ptr(), save_invstd.data_ptr(), int(ctx.relu), dx.data_ptr(), dgamma.data_ptr(),
                      dbeta.data_ptr(), workspace.data_ptr(), _lib.stream())
        return dx, dgamma, dbeta, None, None, None, None, None


def bn_supported(bn):
    """True if `bn` is a layer the Function covers: exactly ``nn.BatchNorm2d`` (a SyncBatchNorm stays a torch module), affine,
    tracking its running statistics with a momentum, fp32 on the GPU, a covered width."""
    if type(bn) is not nn.BatchNorm2d or not bn.affine or not bn.track_running_stats or bn.momentum is None:
        return False
    if bn.running_mean is None or bn.running_var is None or bn.weight.dtype != torch.float32 or not bn.weight.is_cuda:
        return False
    return bool(_lib.lib().mssvt_bn_train_supported(bn.num_features))


def bn_routed(bn):
    """True if the modules send this layer to the Function when `fused_train` and `fused_bn` are on."""
    return bn_supported(bn) and (bn.num_features in ROUTED_BN or bn.num_features in NARROW_CHANNELS)


def bn_relu(bn, x, relu):
    """A `bn_supported` BatchNorm2d in training mode (and the ReLU behind it if `relu`) through the Function; the step counter
    is advanced on the device as the module does."""
    y = BnReluFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, relu)[0]
    if bn.num_batches_tracked is not None:
        with torch.no_grad():
            bn.num_batches_tracked += 1
    return y
