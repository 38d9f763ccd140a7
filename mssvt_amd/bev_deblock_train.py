"""The transposed BEV deblocks in TRAINING mode on split-fp16 matrix instructions (csrc/bev_conv.hip).

``DeblockFunction`` is ``y = conv_transpose2d(x, w, stride=s)`` for a ``ConvTranspose2d`` whose kernel equals its stride
s in {1, 2} (no padding, no bias) on channels-last fp32 GPU tensors with a hand-written backward.  x (B, cin, H, W),
w (cin, cout, s, s) as the module holds it, y and dY (B, cout, s H, s W):

    forward   the inference kernels on a weight-only blob (scale 1, shift 0, no activation): ``mssvt_bev_conv`` with the
              transposed 1 x 1 pack for s = 1, ``mssvt_bev_up2`` for s = 2;
    dX        ``deblock_dgrad``: mssvt_bev_deblock_dgrad, the convolution kernel over dY with the weight tensor read as the
              Conv2d weight (out = cin, in = cout, ky, kx) it already is -- s x s taps at stride s; skipped when the input
              needs no gradient;
    dW        ``deblock_wgrad``: mssvt_bev_deblock_wgrad, ``bev_conv_train.conv_wgrad``'s GEMM over pixels with the phases
              (dy, dx) as taps -- slices added in slice order, no atomics, bit-identical from step to step.

The weights are repacked on every call (they change every step).  BatchNorm + ReLU behind the deblock and ``torch.cat``
stay what they are (``bev_conv_train.run_layers_train``).

``ROUTED_DEBLOCK_TRAIN`` lists the product shapes (stride, cin, cout) the modules send here when ``fused_train`` and
``fused_train_deblocks`` are both on: exactly those whose slowest forward + backward beat the library's fastest at B = 1 and
B = 4 in tools/time_bev_deblock_train.py (profiles/bev_deblock_train_times.json, DESIGN section 5.5's rule).  Every covered
shape stays reachable through the Function.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, bev_conv
from ._lib import MssvtHipError

# (stride, cin, cout)
SHAPES = ((1, 128, 256), (2, 256, 256), (1, 32, 64), (2, 64, 32))
# the product shapes that cleared the routing rule on an MI355X (profiles/bev_deblock_train_times.json: slowest forward +
# backward against the library's fastest, 0.518 / 0.625 ms (B = 1) and 2.119 / 2.201 ms (B = 4) for the 1 x 1 deblock at 470 x 470,
# 0.752 / 0.822 ms and 2.460 / 4.537 ms for the up-2 deblock at 235 x 235 -> 470 x 470: both cleared it)
ROUTED_DEBLOCK_TRAIN = frozenset({(1, 128, 256), (2, 256, 256)})
# the narrow shapes exist for small module tests: never timed, routed whenever the switch is on
NARROW_SHAPES = frozenset({(1, 32, 64), (2, 64, 32)})


def slice_pixels(stride, cin, cout):
    """Input pixels per slice of the weight-gradient kernel for this shape (0: not covered)."""
    return int(_lib.lib().mssvt_bev_deblock_wgrad_slice_pixels(stride, cin, cout))


def wgrad_workspace_bytes(B, H, W, stride, cin, cout):
    n = int(_lib.lib().mssvt_bev_deblock_wgrad_workspace_bytes(B, H, W, stride, cin, cout))
    if n <= 0:
        raise MssvtHipError("mssvt_bev_deblock_wgrad_workspace_bytes(%d, %d, %d, %d, %d, %d) refused the size"
                            % (B, H, W, stride, cin, cout))
    return n


def dgrad_workspace_bytes(B, H, W, stride, cin, cout):
    n = int(_lib.lib().mssvt_bev_deblock_dgrad_workspace_bytes(B, H, W, stride, cin, cout))
    if n <= 0:
        raise MssvtHipError("mssvt_bev_deblock_dgrad_workspace_bytes(%d, %d, %d, %d, %d, %d) refused the size"
                            % (B, H, W, stride, cin, cout))
    return n


def _nhwc(t):
    return t if bev_conv.is_channels_last(t) else t.contiguous(memory_format=torch.channels_last)


def _check(who, *tensors):
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and bev_conv.is_channels_last(t)):
            raise MssvtHipError("bev_deblock_train.%s needs 4-D fp32 GPU tensors that are channels-last in memory (no CPU path)" % who)


def _workspace(who, workspace, nbytes, device):
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    if not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.device == device
            and workspace.dtype == torch.uint8 and workspace.numel() >= nbytes):
        raise MssvtHipError("bev_deblock_train.%s: workspace must hold %d bytes on %s" % (who, nbytes, device))
    return workspace


def deblock_wgrad(x, dy, stride, workspace=None):
    """x (B, cin, H, W), dy (B, cout, s H, s W): fp32 on the GPU, channels-last in memory -> dw (cin, cout, s, s), contiguous.
    `workspace`: a uint8 tensor of ``wgrad_workspace_bytes`` (allocated here if None; its contents do not matter)."""
    _check("deblock_wgrad", x, dy)
    s = int(stride)
    B, cin, H, W = x.shape
    cout = dy.shape[1]
    if tuple(dy.shape) != (B, cout, s * H, s * W) or dy.device != x.device or min(B, H, W) < 1:
        raise MssvtHipError("bev_deblock_train.deblock_wgrad: x is %s, dy is %s, stride %d" % (tuple(x.shape), tuple(dy.shape), s))
    workspace = _workspace("deblock_wgrad", workspace, wgrad_workspace_bytes(B, H, W, s, cin, cout), x.device)
    dw = torch.empty((cin, cout, s, s), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("mssvt_bev_deblock_wgrad", x.data_ptr(), dy.data_ptr(), B, H, W, cin, cout, s, dw.data_ptr(),
                  workspace.data_ptr(), _lib.stream())
    return dw


def deblock_dgrad(dy, w, stride, workspace=None):
    """dy (B, cout, s H, s W) fp32 on the GPU, channels-last in memory, w (cin, cout, s, s) -> dx (B, cin, H, W), channels-last.
    `workspace`: a uint8 tensor of ``dgrad_workspace_bytes`` (allocated here if None; its contents do not matter)."""
    _check("deblock_dgrad", dy)
    s = int(stride)
    if not (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and w.device == dy.device):
        raise MssvtHipError("bev_deblock_train.deblock_dgrad needs an fp32 weight tensor on the gradient's GPU")
    B, cout, Hs, Ws = dy.shape
    cin = int(w.shape[0])
    if tuple(w.shape) != (cin, cout, s, s) or s < 1 or Hs % s or Ws % s or min(B, Hs, Ws) < 1:
        raise MssvtHipError("bev_deblock_train.deblock_dgrad: dy is %s, w is %s, stride %d" % (tuple(dy.shape), tuple(w.shape), s))
    H, W = Hs // s, Ws // s
    workspace = _workspace("deblock_dgrad", workspace, dgrad_workspace_bytes(B, H, W, s, cin, cout), dy.device)
    w = w.detach().contiguous()
    dx = torch.empty((B, H, W, cin), dtype=torch.float32, device=dy.device)
    with torch.cuda.device(dy.device):
        _lib.call("mssvt_bev_deblock_dgrad", dy.data_ptr(), w.data_ptr(), B, H, W, cin, cout, s, dx.data_ptr(),
                  workspace.data_ptr(), _lib.stream())
    return dx.permute(0, 3, 1, 2)


@torch.no_grad()
def _pack_forward(w, stride, cin, cout):
    """The weight-only blob of the forward kernel (scale 1, shift 0), never cached.  No host read."""
    lib = _lib.lib()
    w = w.detach().contiguous()
    if stride == 1:
        blob = torch.empty(lib.mssvt_bev_conv_pack_bytes(1, cin, cout), dtype=torch.uint8, device=w.device)
        _lib.call("mssvt_bev_conv_pack", _lib.ptr(w), 1, None, None, None, None, None, 0.0, 1, cin, cout, _lib.ptr(blob),
                  _lib.stream())
        return bev_conv.Packed(blob, (1, cin, cout, 1, 1, True))
    blob = torch.empty(lib.mssvt_bev_up2_pack_bytes(cin, cout), dtype=torch.uint8, device=w.device)
    _lib.call("mssvt_bev_up2_pack", _lib.ptr(w), None, None, None, None, None, 0.0, cin, cout, _lib.ptr(blob), _lib.stream())
    return bev_conv.PackedUp2(blob, (cin, cout))


class DeblockFunction(torch.autograd.Function):
    """``DeblockFunction.apply(x, w, stride)``: x (B, cin, H, W) fp32 on the GPU (made channels-last), w (cin, cout, s, s)."""

    @staticmethod
    def forward(ctx, x, w, stride):
        s, cin, cout = int(stride), int(w.shape[0]), int(w.shape[1])
        if tuple(w.shape) != (cin, cout, s, s) or not _lib.lib().mssvt_bev_deblock_train_supported(s, cin, cout):
            raise MssvtHipError("bev_deblock_train.DeblockFunction: shape not covered (stride %d, weight %s)" % (s, tuple(w.shape)))
        x = _nhwc(x)
        with torch.cuda.device(x.device):
            packed = _pack_forward(w, s, cin, cout)
            y = bev_conv.conv_bn_act(x, packed, relu=False) if s == 1 else bev_conv.up2_bn_act(x, packed, relu=False)
        ctx.save_for_backward(x, w)
        ctx.stride = s
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _nhwc(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = deblock_dgrad(dy, w, ctx.stride)
        if ctx.needs_input_grad[1]:
            dw = deblock_wgrad(x, dy, ctx.stride)
        return dx, dw, None


def deblock_shape(conv):
    """(stride, cin, cout) of a ConvTranspose2d with kernel = stride in {1, 2} and nothing else (no padding, output padding,
    dilation, groups or bias), else None."""
    if not isinstance(conv, nn.ConvTranspose2d) or conv.groups != 1 or conv.bias is not None:
        return None
    k, s = bev_conv._pair(conv.kernel_size), bev_conv._pair(conv.stride)
    if k != s or k[0] != k[1] or k[0] not in (1, 2) or bev_conv._pair(conv.dilation) != (1, 1):
        return None
    if isinstance(conv.padding, str) or bev_conv._pair(conv.padding) != (0, 0) or bev_conv._pair(conv.output_padding) != (0, 0):
        return None
    return (s[0], int(conv.in_channels), int(conv.out_channels))


def deblock_train_supported(conv):
    """True if `conv` is a deblock the Function covers: ``deblock_shape``, a covered shape, fp32 weights on the GPU."""
    shape = deblock_shape(conv)
    if shape is None or conv.weight.dtype != torch.float32 or not conv.weight.is_cuda:
        return False
    return bool(_lib.lib().mssvt_bev_deblock_train_supported(*shape))


def deblock_train_routed(conv):
    """True if the modules send this deblock to the Function when `fused_train` and `fused_train_deblocks` are on."""
    if not deblock_train_supported(conv):
        return False
    shape = deblock_shape(conv)
    return shape in ROUTED_DEBLOCK_TRAIN or shape in NARROW_SHAPES


def deblock(conv, x):
    """A `deblock_train_supported` deblock through the Function."""
    return DeblockFunction.apply(x, conv.weight, bev_conv._pair(conv.stride)[0])
