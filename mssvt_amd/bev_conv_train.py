"""The stride-1 3 x 3 BEV convolutions in TRAINING mode on split-fp16 matrix instructions (csrc/bev_conv.hip).

``Conv3x3Function`` is ``y = conv(x, w)`` (3 x 3, stride 1, dilation d in {1, 2}, zero padding d, no bias, cin = cout) on
channels-last fp32 GPU tensors with a hand-written backward:

    forward   ``bev_conv.conv_bn_act(x, bev_conv.pack_weight(w), relu=False)`` -- the inference kernel, scale 1 / shift 0;
    dX        the same call on dY with the weights rotated by 180 degrees and the channel axes swapped
              (``w.flip(2, 3).transpose(0, 1)``), skipped when the input needs no gradient;
    dW        ``conv_wgrad``: mssvt_bev_conv_wgrad, a GEMM over pixels cut into slices whose partial slabs are added in slice
              order -- no atomics, bit-identical from step to step.

The weights are repacked on every call (they change every step).  Every layer the kernel does not cover (the stride-2 layer,
the 1 x 1 deblock, the transposed deblock) stays a torch module: ``run_layers_train`` runs a stack on channels-last tensors and
sends the ``train_routed`` convolutions through the Function.  With ``fused_deblocks=True`` the transposed deblocks that
``bev_deblock_train.deblock_train_routed`` accepts run through ``bev_deblock_train.DeblockFunction`` (the same kernels with
other tap sets).  The stride-2 layer stays a module unless ``fused_down=True`` and ``bev_down_train.down_train_routed`` accepts
it: then it runs through ``bev_down_train.DownFunction`` (never through ``conv3x3``).  BatchNorm in training mode and ReLU stay torch modules too
unless the modules' second switch, ``fused_bn``, is on: then ``run_layers_train(..., fused_bn=True)`` sends every BatchNorm2d
that ``bn_train.bn_routed`` accepts, with the ReLU behind it, through ``bn_train.BnReluFunction`` (csrc/bn_train.hip).

``ROUTED_TRAIN`` lists the product layer shapes the modules send here when their ``fused_train`` switch is on: exactly those
whose slowest forward + backward beat the library's fastest at B = 1 and B = 4 in tools/time_bev_conv_train.py
(profiles/bev_conv_train_times.json, DESIGN section 5.5's rule).  Every covered shape stays reachable through the Function.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib, bev_conv
from ._lib import MssvtHipError

CHANNEL_SHAPES = ((128, 128), (256, 256), (32, 32), (64, 64))
# (ksize, cin, cout, stride, dilation) of the product layers that cleared the routing rule on an MI355X
# (profiles/bev_conv_train_times.json: all three covered shapes of the configuration cleared it, at B = 1 and B = 4)
ROUTED_TRAIN = frozenset({(3, 128, 128, 1, 1), (3, 128, 128, 1, 2), (3, 256, 256, 1, 1)})
# the narrow shapes exist for small module tests: never timed, routed whenever the switch is on
NARROW_CHANNELS = frozenset({(32, 32), (64, 64)})


def slice_pixels(cin, cout):
    """Pixels per slice of the weight-gradient kernel for this channel shape (0: not covered)."""
    return int(_lib.lib().mssvt_bev_conv_wgrad_slice_pixels(cin, cout))


def workspace_bytes(B, H, W, cin, cout):
    n = int(_lib.lib().mssvt_bev_conv_wgrad_workspace_bytes(B, H, W, 3, cin, cout))
    if n <= 0:
        raise MssvtHipError("mssvt_bev_conv_wgrad_workspace_bytes(%d, %d, %d, 3, %d, %d) refused the size" % (B, H, W, cin, cout))
    return n


def _nhwc(t):
    return t if bev_conv.is_channels_last(t) else t.contiguous(memory_format=torch.channels_last)


def conv_wgrad(x, dy, dilation=1, workspace=None):
    """x (B, cin, H, W), dy (B, cout, H, W): fp32 on the GPU, channels-last in memory -> dw (cout, cin, 3, 3), contiguous.
    `workspace`: a uint8 tensor of ``workspace_bytes`` (allocated here if None; its contents do not matter)."""
    for t in (x, dy):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and bev_conv.is_channels_last(t)):
            raise MssvtHipError("bev_conv_train.conv_wgrad needs 4-D fp32 GPU tensors that are channels-last in memory (no CPU path)")
    B, cin, H, W = x.shape
    cout = dy.shape[1]
    if tuple(dy.shape) != (B, cout, H, W) or dy.device != x.device or min(B, H, W) < 1:
        raise MssvtHipError("bev_conv_train.conv_wgrad: x is %s, dy is %s" % (tuple(x.shape), tuple(dy.shape)))
    nbytes = workspace_bytes(B, H, W, cin, cout)
    if workspace is None:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    elif not (workspace.is_cuda and workspace.device == x.device and workspace.dtype == torch.uint8 and workspace.numel() >= nbytes):
        raise MssvtHipError("bev_conv_train.conv_wgrad: workspace must hold %d bytes on %s" % (nbytes, x.device))
    dw = torch.empty((cout, cin, 3, 3), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.call("mssvt_bev_conv_wgrad", x.data_ptr(), dy.data_ptr(), B, H, W, cin, cout, 3, int(dilation), dw.data_ptr(),
                  workspace.data_ptr(), _lib.stream())
    return dw


class Conv3x3Function(torch.autograd.Function):
    """``Conv3x3Function.apply(x, w, dilation)``: x (B, cin, H, W) fp32 on the GPU (made channels-last), w (cout, cin, 3, 3)."""

    @staticmethod
    def forward(ctx, x, w, dilation=1):
        cout, cin = int(w.shape[0]), int(w.shape[1])
        x = _nhwc(x)
        with torch.cuda.device(x.device):
            y = bev_conv.conv_bn_act(x, bev_conv.pack_weight(w, 3, cin, cout, 1, int(dilation)), relu=False)
        ctx.save_for_backward(x, w)
        ctx.dilation = int(dilation)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        cout, cin = int(w.shape[0]), int(w.shape[1])
        dy = _nhwc(dy)
        dx = dw = None
        with torch.cuda.device(x.device):
            if ctx.needs_input_grad[0]:
                rot = w.flip(2, 3).transpose(0, 1).contiguous()  # (cin, cout, 3, 3): a convolution cout -> cin
                dx = bev_conv.conv_bn_act(dy, bev_conv.pack_weight(rot, 3, cout, cin, 1, ctx.dilation), relu=False)
            if ctx.needs_input_grad[1]:
                dw = conv_wgrad(x, dy, ctx.dilation)
        return dx, dw, None


def train_supported(conv, pad=None):
    """True if `conv` is a layer the Function covers: Conv2d, 3 x 3, stride 1, bias=False, padding = dilation (or `pad` = 1
    from a ZeroPad2d(1) in front of a padding-0 convolution), a covered channel shape, fp32 on the GPU."""
    if not isinstance(conv, nn.Conv2d) or conv.bias is not None:
        return False
    shape = bev_conv.layer_shape(conv, pad)
    if shape is None or shape[5] or conv.weight.dtype != torch.float32 or not conv.weight.is_cuda:
        return False
    return bool(_lib.lib().mssvt_bev_conv_wgrad_supported(*shape[:5])) and bool(_lib.lib().mssvt_bev_conv_supported(*shape[:5]))


def train_routed(conv, pad=None):
    """True if the modules send this layer to the Function when `fused_train` is on."""
    if not train_supported(conv, pad):
        return False
    shape = bev_conv.layer_shape(conv, pad)
    return shape[:5] in ROUTED_TRAIN or shape[1:3] in NARROW_CHANNELS


def switch_applies(module, x):
    """The conditions under which a module's `fused_train` takes effect: on, training mode, autograd on, fp32 on the GPU, no AMP."""
    return bool(getattr(module, "fused_train", False)) and module.training and torch.is_grad_enabled() \
        and not getattr(module, "use_amp", False) and x.is_cuda and x.dtype == torch.float32


def conv3x3(conv, x):
    """A `train_supported` convolution through the Function."""
    return Conv3x3Function.apply(x, conv.weight, bev_conv._pair(conv.dilation)[0])


def run_layers_train(layers, x, fused_bn=False, fused_deblocks=False, fused_down=False):
    """A Conv / BatchNorm / ReLU stack (`layers`: the modules in order) on a channels-last tensor with autograd on: every
    routed convolution through ``Conv3x3Function``, every other module (BatchNorm2d / SyncBatchNorm in training mode and ReLU
    included) as the torch module it is, on the same channels-last tensors.  With `fused_bn`, a BatchNorm2d that
    ``bn_train.bn_routed`` accepts runs through ``bn_train.bn_relu`` together with the ``nn.ReLU`` behind it (in place or not;
    without one: ``relu=False``); every other BatchNorm and ReLU stays a module.  With `fused_deblocks`, a ConvTranspose2d that
    ``bev_deblock_train.deblock_train_routed`` accepts runs through ``bev_deblock_train.DeblockFunction``; every other one
    stays a module.  With `fused_down`, a 3 x 3 stride-2 Conv2d with padding 1 (or a ZeroPad2d(1) + padding-0 pair) that
    ``bev_down_train.down_train_routed`` accepts runs through ``bev_down_train.DownFunction``."""
    layers = list(layers)
    i, n = 0, len(layers)
    if fused_bn:
        from . import bn_train
    if fused_deblocks:
        from . import bev_deblock_train
    if fused_down:
        from . import bev_down_train
    while i < n:
        m = layers[i]
        if fused_bn and bn_train.bn_routed(m):
            relu = i + 1 < n and type(layers[i + 1]) is nn.ReLU
            x = bn_train.bn_relu(m, x, relu)
            i += 2 if relu else 1
        elif isinstance(m, nn.ZeroPad2d) and tuple(m.padding) == (1, 1, 1, 1) and i + 1 < n \
                and isinstance(layers[i + 1], nn.Conv2d) and bev_conv._pair(layers[i + 1].padding) == (0, 0) \
                and train_routed(layers[i + 1], 1):
            x = conv3x3(layers[i + 1], x)
            i += 2
        elif isinstance(m, nn.Conv2d) and train_routed(m):
            x = conv3x3(m, x)
            i += 1
        elif fused_down and isinstance(m, nn.ZeroPad2d) and tuple(m.padding) == (1, 1, 1, 1) and i + 1 < n \
                and isinstance(layers[i + 1], nn.Conv2d) and bev_conv._pair(layers[i + 1].padding) == (0, 0) \
                and bev_down_train.down_train_routed(layers[i + 1], 1):
            x = bev_down_train.down(layers[i + 1], x)
            i += 2
        elif fused_down and isinstance(m, nn.Conv2d) and bev_down_train.down_train_routed(m):
            x = bev_down_train.down(m, x)
            i += 1
        elif fused_deblocks and isinstance(m, nn.ConvTranspose2d) and bev_deblock_train.deblock_train_routed(m):
            x = bev_deblock_train.deblock(m, x)
            i += 1
        else:
            x = m(x)
            i += 1
    return x
