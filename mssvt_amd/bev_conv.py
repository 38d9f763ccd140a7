"""Dense BEV convolutions on split-fp16 matrix instructions (csrc/bev_conv.hip): ``y = act(scale * conv(x, w) + shift)``
on channels-last fp32 tensors, inference only.

Stands for the Conv2d + BatchNorm2d + ReLU triples of the reference's ``HeightCompression.compress_layers``
(pcdet/models/backbones_2d/map_to_bev/height_compression.py:20-39) and ``BaseBEVBackbone`` blocks / 1x1 deblocks
(pcdet/models/backbones_2d/base_bev_backbone.py:30-78) in eval mode.  A layer is turned into one packed blob on the
device (fp16 hi / lo weight images + the folded BatchNorm as fp32 scale / shift) by ``pack``; ``conv_bn_act`` runs it.
There is no CPU path.

``ROUTED`` lists the product layer shapes the modules send here when their ``fused_convs`` switch is on: exactly those
whose slowest run beat the library's fastest in tools/time_bev_conv.py (profiles/bev_conv_times.json, DESIGN section
5.5's rule).  Every covered shape stays reachable through ``conv_bn_act``.

The 2 x 2 stride-2 transposed deblock (``ConvTranspose2d(cin, cout, 2, stride=2)`` + BN + ReLU) is a family of its own:
``up2_shape`` / ``up2_supported`` / ``pack_up2`` / ``up2_bn_act``, routed by ``ROUTED_UP2`` (tools/time_bev_deblocks.py,
profiles/bev_deblock_times.json, the same rule).  ``conv_bn_act`` and ``up2_bn_act`` take ``out=, channel=``: the layer
then writes its channel slice of a wider channels-last tensor (``BaseBEVBackbone``'s ``fused_deblocks``: no ``torch.cat``).
"""
import weakref

import torch
from torch import nn

from . import _lib
from ._lib import MssvtHipError

# the kernel's tiles (include/mssvt_hip.h: MSSVT_BEV_CONV_WAVE_PIXELS / MSSVT_BEV_CONV_BLOCK_PIXELS)
WAVE_PIXELS = 32
BLOCK_PIXELS = 256

CHANNEL_SHAPES = ((128, 128), (128, 256), (256, 256), (32, 32), (32, 64), (64, 64))
# (ksize, cin, cout, stride, dilation) of the product layers (mssvt.yaml) that cleared the routing rule on an MI355X
# (profiles/bev_conv_times.json: all five covered shapes of the configuration cleared it, at B = 1 and B = 4)
ROUTED = frozenset({
    (3, 128, 128, 1, 1), (3, 128, 128, 1, 2), (3, 128, 256, 2, 1), (3, 256, 256, 1, 1), (1, 128, 256, 1, 1),
})
# the narrow shapes exist so that the reference-run goldens (32 / 64 channels) pass through the kernel: no product
# configuration has them, they are not timed, and the modules route them whenever the switch is on
GOLDEN_CHANNELS = frozenset({(32, 32), (32, 64), (64, 64)})
# (cin, cout) of the 2 x 2 stride-2 transposed deblocks: covered; routed by the modules' `fused_deblocks` (the rule above on
# profiles/bev_deblock_times.json: 0.19 / 0.70 ms against the library's 0.47 / 1.85 ms at B = 1 / 4); the reference-run golden's
# shape (det_bev_head.npz), never timed
UP2_CHANNEL_SHAPES = ((256, 256), (64, 32))
ROUTED_UP2 = frozenset({(256, 256)})
GOLDEN_UP2 = frozenset({(64, 32)})


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def layer_shape(conv, pad=None):
    """(ksize, cin, cout, stride, dilation, transposed) of a layer the kernel's tap sets can express, else None.  `pad`
    overrides the convolution's own padding (a ZeroPad2d(1) in front of a padding-0 convolution: pad = 1)."""
    transposed = isinstance(conv, nn.ConvTranspose2d)
    if not isinstance(conv, (nn.Conv2d, nn.ConvTranspose2d)) or conv.groups != 1:
        return None
    if not transposed and conv.padding_mode != "zeros":
        return None
    k, s, d = _pair(conv.kernel_size), _pair(conv.stride), _pair(conv.dilation)
    if isinstance(conv.padding, str) or k[0] != k[1] or s[0] != s[1] or d[0] != d[1]:
        return None
    p = _pair(conv.padding) if pad is None else _pair(pad)
    if p[0] != p[1]:
        return None
    if transposed and (k[0] != 1 or s[0] != 1 or _pair(conv.output_padding) != (0, 0)):
        return None
    if p[0] != (d[0] if k[0] == 3 else 0):
        return None
    return (k[0], int(conv.in_channels), int(conv.out_channels), s[0], d[0], transposed)


def supported(conv, bn=None, pad=None):
    """True if `conv` (+ an eval-mode BatchNorm2d `bn`) is a layer ``pack`` / ``conv_bn_act`` cover."""
    shape = layer_shape(conv, pad)
    if shape is None or conv.weight.dtype != torch.float32 or not conv.weight.is_cuda:
        return False
    if bn is not None and not (isinstance(bn, nn.BatchNorm2d) and bn.running_mean is not None and bn.running_var is not None
                               and bn.num_features == shape[2]):
        return False
    return bool(_lib.lib().mssvt_bev_conv_supported(*shape[:5]))


def routed(conv, bn=None, pad=None):
    """True if the modules send this layer to the kernel when their switch is on."""
    if not supported(conv, bn, pad):
        return False
    shape = layer_shape(conv, pad)
    return shape[:5] in ROUTED or shape[1:3] in GOLDEN_CHANNELS


def up2_shape(conv):
    """(cin, cout) of a ConvTranspose2d with kernel 2 and stride 2 and nothing else (no padding, output padding, dilation or
    groups), else None."""
    if not isinstance(conv, nn.ConvTranspose2d) or conv.groups != 1:
        return None
    if _pair(conv.kernel_size) != (2, 2) or _pair(conv.stride) != (2, 2) or _pair(conv.dilation) != (1, 1):
        return None
    if isinstance(conv.padding, str) or _pair(conv.padding) != (0, 0) or _pair(conv.output_padding) != (0, 0):
        return None
    return (int(conv.in_channels), int(conv.out_channels))


def up2_supported(conv, bn=None):
    """True if `conv` (+ an eval-mode BatchNorm2d `bn`) is a layer ``pack_up2`` / ``up2_bn_act`` cover."""
    shape = up2_shape(conv)
    if shape is None or conv.weight.dtype != torch.float32 or not conv.weight.is_cuda:
        return False
    if bn is not None and not (isinstance(bn, nn.BatchNorm2d) and bn.running_mean is not None and bn.running_var is not None
                               and bn.num_features == shape[1]):
        return False
    return bool(_lib.lib().mssvt_bev_up2_supported(*shape))


def up2_routed(conv, bn=None):
    """True if the modules send this deblock to the kernel when `fused_deblocks` is on."""
    return up2_supported(conv, bn) and (up2_shape(conv) in ROUTED_UP2 or up2_shape(conv) in GOLDEN_UP2)


class Packed(object):
    """One layer as the kernel reads it: `blob` (uint8, device) and the layer's geometry."""
    __slots__ = ("blob", "ksize", "cin", "cout", "stride", "dilation", "transposed")

    def __init__(self, blob, shape):
        self.blob = blob
        self.ksize, self.cin, self.cout, self.stride, self.dilation, self.transposed = shape

    def out_size(self, h, w):
        return (h - 1) // self.stride + 1, (w - 1) // self.stride + 1


class PackedUp2(object):
    """One 2 x 2 stride-2 transposed layer as the kernel reads it."""
    __slots__ = ("blob", "cin", "cout")

    def __init__(self, blob, shape):
        self.blob = blob
        self.cin, self.cout = shape

    def out_size(self, h, w):
        return 2 * h, 2 * w


_cache = weakref.WeakKeyDictionary()  # conv module -> (key, Packed or PackedUp2)


def _tensors(conv, bn):
    return [conv.weight, conv.bias] + ([None] * 4 if bn is None else [bn.weight, bn.bias, bn.running_mean, bn.running_var])


def params(conv, bn, who="bev_conv.pack"):
    """[weight, bias, bn weight, bn bias, running mean, running var] of (conv, bn), checked fp32 on one GPU, detached and
    contiguous (None where the layer has none)."""
    ts = _tensors(conv, bn)
    for t in ts:
        if t is not None and not (t.is_cuda and t.dtype == torch.float32 and t.device == conv.weight.device):
            raise MssvtHipError("%s: parameters must be fp32 tensors on one GPU (no CPU path)" % who)
    return [None if t is None else t.detach().contiguous() for t in ts]


def pair_key(conv, bn):
    """The cache-key element of (conv, bn): the modules' identity and every tensor's identity, storage and version
    (load_state_dict and an optimizer step write in place: version; .to() and a re-assigned parameter change the identity
    or the storage)."""
    return (id(conv), id(bn), None if bn is None else float(bn.eps)) + tuple(
        None if t is None else (id(t), t.data_ptr(), t._version, str(t.device)) for t in _tensors(conv, bn))


def _key(conv, bn, pad):
    return (pair_key(conv, bn), pad)


@torch.no_grad()
def pack(conv, bn=None, pad=None):
    """The packed blob of a layer (cached per `conv` module; rebuilt when a parameter or running statistic changed).
    Runs on the device on the current stream, no host read."""
    key = _key(conv, bn, pad)
    hit = _cache.get(conv)
    if hit is not None and hit[0] == key:
        return hit[1]
    if not supported(conv, bn, pad):
        raise MssvtHipError("bev_conv.pack: layer not covered (%r, %r)" % (conv, bn))
    shape = layer_shape(conv, pad)
    ksize, cin, cout = shape[:3]
    w, bias, bn_w, bn_b, bn_m, bn_v = params(conv, bn)
    nbytes = _lib.lib().mssvt_bev_conv_pack_bytes(ksize, cin, cout)
    blob = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("mssvt_bev_conv_pack", _lib.ptr(w), int(shape[5]), _lib.ptr(bias), _lib.ptr(bn_w), _lib.ptr(bn_b),
                  _lib.ptr(bn_m), _lib.ptr(bn_v), 0.0 if bn is None else float(bn.eps), ksize, cin, cout, _lib.ptr(blob),
                  _lib.stream())
    packed = Packed(blob, shape)
    _cache[conv] = (key, packed)
    return packed


@torch.no_grad()
def pack_weight(w, ksize, cin, cout, stride=1, dilation=1):
    """A plain weight tensor `w` (cout, cin, ksize, ksize) with no bias and no BatchNorm (scale 1, shift 0) as a ``Packed``
    layer of that stride / dilation, never cached: the training path (bev_conv_train.py) repacks every step.  No host read."""
    if not (isinstance(w, torch.Tensor) and w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == (cout, cin, ksize, ksize)):
        raise MssvtHipError("bev_conv.pack_weight needs an fp32 GPU tensor of shape (%d, %d, %d, %d)" % (cout, cin, ksize, ksize))
    nbytes = _lib.lib().mssvt_bev_conv_pack_bytes(ksize, cin, cout)
    if nbytes <= 0:
        raise MssvtHipError("bev_conv.pack_weight: shape not covered (%d, %d, %d)" % (ksize, cin, cout))
    w = w.detach().contiguous()
    blob = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("mssvt_bev_conv_pack", _lib.ptr(w), 0, None, None, None, None, None, 0.0, ksize, cin, cout, _lib.ptr(blob),
                  _lib.stream())
    return Packed(blob, (ksize, cin, cout, stride, dilation, False))


@torch.no_grad()
def pack_up2(conv, bn=None):
    """The packed blob of a 2 x 2 stride-2 transposed layer: `pack`'s cache and key (rebuilt when a tensor changed)."""
    key = _key(conv, bn, "up2")
    hit = _cache.get(conv)
    if hit is not None and hit[0] == key:
        return hit[1]
    if not up2_supported(conv, bn):
        raise MssvtHipError("bev_conv.pack_up2: layer not covered (%r, %r)" % (conv, bn))
    cin, cout = up2_shape(conv)
    w, bias, bn_w, bn_b, bn_m, bn_v = params(conv, bn, "bev_conv.pack_up2")
    blob = torch.empty(_lib.lib().mssvt_bev_up2_pack_bytes(cin, cout), dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        _lib.call("mssvt_bev_up2_pack", _lib.ptr(w), _lib.ptr(bias), _lib.ptr(bn_w), _lib.ptr(bn_b), _lib.ptr(bn_m), _lib.ptr(bn_v),
                  0.0 if bn is None else float(bn.eps), cin, cout, _lib.ptr(blob), _lib.stream())
    packed = PackedUp2(blob, (cin, cout))
    _cache[conv] = (key, packed)
    return packed


def is_channels_last(x):
    """4-D and NHWC in memory (the logical shape stays (B, C, H, W))."""
    return x.dim() == 4 and x.permute(0, 2, 3, 1).is_contiguous()


def _input(x, packed, who):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and is_channels_last(x)):
        raise MssvtHipError("bev_conv.%s needs a 4-D fp32 GPU tensor that is channels-last in memory (no CPU path)" % who)
    if x.requires_grad and torch.is_grad_enabled():
        raise MssvtHipError("bev_conv.%s is inference only (autograd is on for this input)" % who)
    B, C, H, W = x.shape
    if C != packed.cin or packed.blob.device != x.device:
        raise MssvtHipError("bev_conv.%s: input has %d channels on %s, the layer takes %d on %s"
                            % (who, C, x.device, packed.cin, packed.blob.device))
    if min(B, H, W) < 1 or x.data_ptr() % 16:
        raise MssvtHipError("bev_conv.%s: empty or unaligned input" % who)
    return B, C, H, W


def _output(out, channel, x, B, ho, wo, cout, who):
    """(y, ystride): `out` checked -- a (B, C, ho, wo) fp32 tensor on x's device, channels-last and dense (pixel stride C),
    16-byte aligned, channel % 4 == 0 and channel + cout <= C -- or a new (B, ho, wo, cout) tensor."""
    if out is None:
        if channel != 0:
            raise MssvtHipError("bev_conv.%s: channel = %r without out" % (who, channel))
        return torch.empty((B, ho, wo, cout), dtype=torch.float32, device=x.device), cout
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == x.device and out.dtype == torch.float32
            and is_channels_last(out)):
        raise MssvtHipError("bev_conv.%s: out must be a dense channels-last 4-D fp32 tensor on the input's device" % who)
    C = out.shape[1]
    if tuple(out.shape) != (B, C, ho, wo) or out.data_ptr() % 16:
        raise MssvtHipError("bev_conv.%s: out is %s (16-byte aligned: %s), the layer writes (%d, C, %d, %d)"
                            % (who, tuple(out.shape), out.data_ptr() % 16 == 0, B, ho, wo))
    if not isinstance(channel, int) or isinstance(channel, bool) or channel < 0 or channel % 4 or channel + cout > C or C % 4:
        raise MssvtHipError("bev_conv.%s: channel = %r must be a multiple of 4 with channel + %d <= %d (a multiple of 4)"
                            % (who, channel, cout, C))
    if out.requires_grad and torch.is_grad_enabled():
        raise MssvtHipError("bev_conv.%s is inference only (autograd is on for out)" % who)
    return out, C


def conv_bn_act(x, packed, relu=True, out=None, channel=0):
    """`x` (B, cin, H, W) fp32 on the GPU, channels-last in memory -> (B, cout, Ho, Wo) of the same kind.  With `out`
    (B, C, Ho, Wo), channels-last: the layer writes channels [channel, channel + cout) of it and returns that view."""
    B, C, H, W = _input(x, packed, "conv_bn_act")
    ho, wo = packed.out_size(H, W)
    y, ystride = _output(out, channel, x, B, ho, wo, packed.cout, "conv_bn_act")
    emap = torch.empty(B * H * W, dtype=torch.int32, device=x.device)
    if out is None:
        _lib.call("mssvt_bev_conv", x.data_ptr(), B, H, W, C, packed.blob.data_ptr(), packed.ksize, packed.cout, packed.stride,
                  packed.dilation, int(bool(relu)), emap.data_ptr(), y.data_ptr(), _lib.stream())
        return y.permute(0, 3, 1, 2)
    _lib.call("mssvt_bev_conv_into", x.data_ptr(), B, H, W, C, packed.blob.data_ptr(), packed.ksize, packed.cout, packed.stride,
              packed.dilation, int(bool(relu)), emap.data_ptr(), y.data_ptr(), ystride, channel, _lib.stream())
    return out[:, channel:channel + packed.cout]


def up2_bn_act(x, packed, relu=True, out=None, channel=0):
    """`x` (B, cin, H, W) fp32 on the GPU, channels-last in memory -> (B, cout, 2H, 2W) of the same kind through a
    ``pack_up2`` blob; `out` / `channel` as in ``conv_bn_act``."""
    if not isinstance(packed, PackedUp2):
        raise MssvtHipError("bev_conv.up2_bn_act needs a pack_up2 blob")
    B, C, H, W = _input(x, packed, "up2_bn_act")
    y, ystride = _output(out, channel, x, B, 2 * H, 2 * W, packed.cout, "up2_bn_act")
    emap = torch.empty(B * H * W, dtype=torch.int32, device=x.device)
    _lib.call("mssvt_bev_up2", x.data_ptr(), B, H, W, C, packed.blob.data_ptr(), packed.cout, int(bool(relu)), emap.data_ptr(),
              y.data_ptr(), ystride, channel, _lib.stream())
    return y.permute(0, 3, 1, 2) if out is None else out[:, channel:channel + packed.cout]


def switch_applies(module, x):
    """The conditions under which a module's `fused_convs` takes effect: on, eval mode, autograd off, fp32 on the GPU, no AMP."""
    return bool(getattr(module, "fused_convs", False)) and not module.training and not torch.is_grad_enabled() \
        and not getattr(module, "use_amp", False) and x.is_cuda and x.dtype == torch.float32


def run_layers(layers, x):
    """A Conv / BatchNorm / ReLU stack (`layers`: the modules in order) on a channels-last tensor: every routed
    Conv + BN (+ ReLU) triple through the kernel, every other module through the library on the same tensors."""
    layers = list(layers)
    i, n = 0, len(layers)
    while i < n:
        m, pad, ci = layers[i], None, i
        if isinstance(m, nn.ZeroPad2d) and tuple(m.padding) == (1, 1, 1, 1) and i + 1 < n \
                and isinstance(layers[i + 1], nn.Conv2d) and _pair(layers[i + 1].padding) == (0, 0):
            pad, ci = 1, i + 1
        conv = layers[ci]
        bn = layers[ci + 1] if ci + 1 < n and isinstance(layers[ci + 1], nn.BatchNorm2d) else None
        if isinstance(conv, (nn.Conv2d, nn.ConvTranspose2d)) and bn is not None and routed(conv, bn, pad):
            relu = ci + 2 < n and isinstance(layers[ci + 2], nn.ReLU)
            x = conv_bn_act(x, pack(conv, bn, pad), relu)
            i = ci + (3 if relu else 2)
        else:
            x = m(x)
            i += 1
    return x
