"""The stride-2 3 x 3 BEV convolution in TRAINING mode on split-fp16 matrix instructions (csrc/bev_conv.hip).

``DownFunction`` is ``y = conv2d(x, w, stride=2, padding=1)`` (3 x 3, dilation 1, no bias) on channels-last fp32 GPU tensors
with a hand-written backward.  x (B, cin, H, W), w (cout, cin, 3, 3) as the module holds it, y and dY (B, cout, Ho, Wo) with
Ho = (H - 1) // 2 + 1, Wo = (W - 1) // 2 + 1:

    forward   ``bev_conv.conv_bn_act(x, bev_conv.pack_weight(w, 3, cin, cout, 2, 1), relu=False)`` -- the inference kernel,
              scale 1 / shift 0;
    dX        ``down_dgrad``: mssvt_bev_down_dgrad, the convolution kernel over dY as the four parity phases of dX in one
              launch (1, 2, 2 and 4 taps: the 9 taps of w each used once, no zero-stuffed dY); skipped when the input needs no
              gradient;
    dW        ``down_wgrad``: mssvt_bev_down_wgrad, ``bev_conv_train.conv_wgrad``'s GEMM over the OUTPUT pixels with x read at
              (2 oy + ky - 1, 2 ox + kx - 1) -- slices added in slice order, no atomics, bit-identical from step to step.

The weights are repacked on every call (they change every step).

``ROUTED_DOWN_TRAIN`` lists the product shapes (cin, cout) the modules send here when ``fused_train`` and
``fused_train_down`` are both on: exactly those whose slowest forward + backward beat the library's fastest at B = 1 and B = 4
in tools/time_bev_down_train.py (profiles/bev_down_train_times.json, DESIGN section 5.5's rule).  Every covered shape stays
reachable through the Function.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, bev_conv
from ._lib import MssvtHipError

# (cin, cout)
SHAPES = ((128, 256), (32, 64))
# the product shapes that cleared the routing rule on an MI355X (profiles/bev_down_train_times.json: slowest forward + backward
# against the library's fastest at 470 x 470 -> 235 x 235, 0.810 / 0.971 ms (B = 1) and 2.460 / 4.394 ms (B = 4): cleared)
ROUTED_DOWN_TRAIN = frozenset({(128, 256)})
# the narrow shape exists for small module tests: never timed, routed whenever the switch is on
NARROW_SHAPES = frozenset({(32, 64)})


def out_size(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def slice_pixels(cin, cout):
    """Output pixels per slice of the weight-gradient kernel for this shape (0: not covered)."""
    return int(_lib.lib().mssvt_bev_down_wgrad_slice_pixels(cin, cout))


def wgrad_workspace_bytes(B, H, W, cin, cout):
    n = int(_lib.lib().mssvt_bev_down_wgrad_workspace_bytes(B, H, W, cin, cout))
    if n <= 0:
        raise MssvtHipError("mssvt_bev_down_wgrad_workspace_bytes(%d, %d, %d, %d, %d) refused the size" % (B, H, W, cin, cout))
    return n


def dgrad_workspace_bytes(B, H, W, cin, cout):
    n = int(_lib.lib().mssvt_bev_down_dgrad_workspace_bytes(B, H, W, cin, cout))
    if n <= 0:
        raise MssvtHipError("mssvt_bev_down_dgrad_workspace_bytes(%d, %d, %d, %d, %d) refused the size" % (B, H, W, cin, cout))
    return n


def _nhwc(t):
    return t if bev_conv.is_channels_last(t) else t.contiguous(memory_format=torch.channels_last)


def _check(who, *tensors):
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and bev_conv.is_channels_last(t)):
            raise MssvtHipError("bev_down_train.%s needs 4-D fp32 GPU tensors that are channels-last in memory (no CPU path)" % who)


def _workspace(who, workspace, nbytes, device):
    if workspace is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    if not (isinstance(workspace, torch.Tensor) and workspace.is_cuda and workspace.device == device
            and workspace.dtype == torch.uint8 and workspace.numel() >= nbytes):
        raise MssvtHipError("bev_down_train.%s: workspace must hold %d bytes on %s" % (who, nbytes, device))
    return workspace


def down_wgrad(x, dy, workspace=None):
    """x (B, cin, H, W), dy (B, cout, Ho, Wo): fp32 on the GPU, channels-last in memory -> dw (cout, cin, 3, 3), contiguous.
    `workspace`: a uint8 tensor of ``wgrad_workspace_bytes`` (allocated here if None; its contents do not matter)."""
    _check("down_wgrad", x, dy)
    B, cin, H, W = x.shape
    cout = dy.shape[1]
    if min(B, H, W) < 1 or tuple(dy.shape) != (B, cout) + out_size(H, W) or dy.device != x.device:
        raise MssvtHipError("bev_down_train.down_wgrad: x is %s, dy is %s" % (tuple(x.shape), tuple(dy.shape)))
    workspace = _workspace("down_wgrad", workspace, wgrad_workspace_bytes(B, H, W, cin, cout), x.device)
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("mssvt_bev_down_wgrad", x.data_ptr(), dy.data_ptr(), B, H, W, cin, cout, dw.data_ptr(), workspace.data_ptr(),
                  _lib.stream())
    return dw


def down_dgrad(dy, w, H, W, workspace=None):
    """dy (B, cout, Ho, Wo) fp32 on the GPU, channels-last in memory, w (cout, cin, 3, 3), (H, W) the layer's input size
    (two sizes share one output size) -> dx (B, cin, H, W), channels-last.
    `workspace`: a uint8 tensor of ``dgrad_workspace_bytes`` (allocated here if None; its contents do not matter)."""
    _check("down_dgrad", dy)
    if not (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and w.dim() == 4 and w.device == dy.device):
        raise MssvtHipError("bev_down_train.down_dgrad needs an fp32 weight tensor on the gradient's GPU")
    B, cout = dy.shape[:2]
    cin, H, W = int(w.shape[1]), int(H), int(W)
    if tuple(w.shape) != (cout, cin, 3, 3) or min(B, H, W) < 1 or tuple(dy.shape[2:]) != out_size(H, W):
        raise MssvtHipError("bev_down_train.down_dgrad: dy is %s, w is %s, input size (%d, %d)"
                            % (tuple(dy.shape), tuple(w.shape), H, W))
    workspace = _workspace("down_dgrad", workspace, dgrad_workspace_bytes(B, H, W, cin, cout), dy.device)
    w = w.detach().contiguous()
    dx = torch.empty((B, H, W, cin), dtype=torch.float32, device=dy.device)
    with torch.cuda.device(dy.device):
        _lib.call("mssvt_bev_down_dgrad", dy.data_ptr(), w.data_ptr(), B, H, W, cin, cout, dx.data_ptr(), workspace.data_ptr(),
                  _lib.stream())
    return dx.permute(0, 3, 1, 2)


class DownFunction(torch.autograd.Function):
    """``DownFunction.apply(x, w)``: x (B, cin, H, W) fp32 on the GPU (made channels-last), w (cout, cin, 3, 3)."""

    @staticmethod
    def forward(ctx, x, w):
        cout, cin = int(w.shape[0]), int(w.shape[1])
        if tuple(w.shape) != (cout, cin, 3, 3) or not _lib.lib().mssvt_bev_down_train_supported(cin, cout):
            raise MssvtHipError("bev_down_train.DownFunction: shape not covered (weight %s)" % (tuple(w.shape),))
        x = _nhwc(x)
        with torch.cuda.device(x.device):
            y = bev_conv.conv_bn_act(x, bev_conv.pack_weight(w, 3, cin, cout, 2, 1), relu=False)
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = _nhwc(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = down_dgrad(dy, w, x.shape[2], x.shape[3])
        if ctx.needs_input_grad[1]:
            dw = down_wgrad(x, dy)
        return dx, dw


def down_shape(conv, pad=None):
    """(cin, cout) of a Conv2d with a 3 x 3 kernel at stride 2, dilation 1, zero padding 1 (its own, or `pad` = 1 from a
    ZeroPad2d(1) in front of a padding-0 convolution) and nothing else (no groups, no bias), else None."""
    if not isinstance(conv, nn.Conv2d) or conv.groups != 1 or conv.bias is not None or conv.padding_mode != "zeros":
        return None
    if isinstance(conv.padding, str) or bev_conv._pair(conv.kernel_size) != (3, 3) or bev_conv._pair(conv.stride) != (2, 2):
        return None
    p = bev_conv._pair(conv.padding) if pad is None else bev_conv._pair(pad)
    if bev_conv._pair(conv.dilation) != (1, 1) or p != (1, 1):
        return None
    return (int(conv.in_channels), int(conv.out_channels))


def down_train_supported(conv, pad=None):
    """True if `conv` is a layer the Function covers: ``down_shape``, a covered shape, fp32 weights on the GPU."""
    shape = down_shape(conv, pad)
    if shape is None or conv.weight.dtype != torch.float32 or not conv.weight.is_cuda:
        return False
    lib = _lib.lib()
    return bool(lib.mssvt_bev_down_train_supported(*shape)) and bool(lib.mssvt_bev_conv_supported(3, shape[0], shape[1], 2, 1))


def down_train_routed(conv, pad=None):
    """True if the modules send this layer to the Function when `fused_train` and `fused_train_down` are on."""
    if not down_train_supported(conv, pad):
        return False
    shape = down_shape(conv, pad)
    return shape in ROUTED_DOWN_TRAIN or shape in NARROW_SHAPES


def down(conv, x):
    """A `down_train_supported` convolution through the Function."""
    return DownFunction.apply(x, conv.weight)
