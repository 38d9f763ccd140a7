"""``CenterHead``'s convolutions on split-fp16 matrix instructions (csrc/head_conv.hip), inference only.

Stands for the reference's ``shared_conv`` and ``SeparateHead`` stacks (pcdet/models/dense_heads/center_head.py:11-46, :76-84,
forward :350-360) in eval mode, as three stages on channels-last fp32 tensors:

* ``shared``: the 3x3 Cin -> S Conv + BatchNorm + ReLU;
* ``trunk``:  the first 3x3 S -> S Conv + BatchNorm + ReLU of every branch of every head as ONE convolution S -> nb S;
* ``finals``: the last 3x3 S -> k_b convolution (bias, no activation) of every branch in one launch, each branch on its own
  S-channel slice of the trunk tensor and normalised on that slice alone, written planar: one buffer
  ``[branch][B][k_b][H][W]`` of which every map is a contiguous ``(B, k_b, H, W)`` view -- the layout ``center_decode`` reads.

Coverage is all or nothing for a module (``supported``): every branch has ``num_conv == 2`` and at most 16 maps, Cin in
{64, 256, 384, 512}, S in {32, 64}, every normalisation a ``BatchNorm2d`` with running statistics.  Any other head runs the
library path as if its ``fused_convs`` switch were off.  ``pack`` turns a head into three blobs on the device (cached per
module, rebuilt when a parameter or running statistic changes); ``forward`` produces the ``pred_dicts``.  No CPU path.

``ROUTED`` lists the stages the module sends to the kernels when its switch is on: those whose slowest run beat the library's
fastest in tools/time_head_conv.py (profiles/head_conv_times.json, DESIGN section 5.7's rule); ``routed_stages(x)`` is that
set for given features (the shared layer is taken only where it causes no layout conversion, ``SHARED_FROM_NCHW``).  A stage
outside it runs through the library on the same tensors; every stage stays callable through ``run_shared`` / ``run_trunk`` /
``run_finals``.
"""
import weakref

import torch
from torch import nn

from . import _lib
from ._lib import MssvtHipError
from .bev_conv import is_channels_last, pair_key, params, switch_applies

STAGES = ("shared", "trunk", "finals")
# the stages that cleared the routing rule on an MI355X at the mssvt.yaml head shape (profiles/head_conv_times.json: all
# three, at B = 1 and B = 4) ...
ROUTED = frozenset({"shared", "trunk", "finals"})
# ... the shared layer on features that ARRIVE channels-last only (the backbone's switch on): behind the layout conversion that
# NCHW features need, its slowest run (1.42 ms at B = 1) does not beat the library's fastest (1.18 ms), so NCHW features take
# the library's shared layer and only its S-channel output is made channels-last
SHARED_FROM_NCHW = False

CIN = (64, 256, 384, 512)  # the channel counts mssvt_head_conv_supported accepts (include/mssvt_hip.h)
S = (32, 64)


def _plain3x3(conv, bias=None):
    return isinstance(conv, nn.Conv2d) and tuple(conv.kernel_size) == (3, 3) and tuple(conv.stride) == (1, 1) \
        and conv.padding in ((1, 1), 1) and tuple(conv.dilation) == (1, 1) and conv.groups == 1 \
        and conv.padding_mode == "zeros" and conv.weight.dtype == torch.float32 \
        and (bias is None or (conv.bias is not None) == bias)


def _bn_ok(bn, channels):
    return isinstance(bn, nn.BatchNorm2d) and bn.running_mean is not None and bn.running_var is not None \
        and bn.num_features == channels


def _triple(seq, cin, cout):
    """(conv, bn) of a Sequential(Conv2d 3x3, BatchNorm2d, ReLU) with these channel counts, else None."""
    if not (isinstance(seq, nn.Sequential) and len(seq) == 3 and _plain3x3(seq[0]) and _bn_ok(seq[1], cout)
            and isinstance(seq[2], nn.ReLU)):
        return None
    if (seq[0].in_channels, seq[0].out_channels) != (cin, cout):
        return None
    return seq[0], seq[1]


def branches(head):
    """[(head index, name, Sequential)] in ``heads_list`` order, inside a head in ``sep_head_dict`` order."""
    return [(i, name, getattr(sep, name)) for i, sep in enumerate(head.heads_list) for name in sep.sep_head_dict]


def layers(head):
    """(shared (conv, bn), [trunk (conv, bn) per branch], [final conv per branch]) of a head with the covered STRUCTURE, else
    None (the sizes are ``mssvt_head_conv_supported``'s to judge)."""
    sc = getattr(head, "shared_conv", None)
    if not (isinstance(sc, nn.Sequential) and len(sc) == 3 and _plain3x3(sc[0])):
        return None
    cin, s = int(sc[0].in_channels), int(sc[0].out_channels)
    shared = _triple(sc, cin, s)
    if shared is None:
        return None
    trunk, finals = [], []
    for _, _, seq in branches(head):
        if not (isinstance(seq, nn.Sequential) and len(seq) == 2):  # num_conv == 2
            return None
        first, last = _triple(seq[0], s, s), seq[1]
        if first is None or not _plain3x3(last, bias=True) or last.in_channels != s:
            return None
        trunk.append(first)
        finals.append(last)
    return (shared, trunk, finals) if trunk else None


def supported(head):
    """The coverage rule of the module docstring (structure and sizes; where the parameters live is ``forward``'s concern)."""
    found = layers(head)
    if found is None:
        return False
    shared, trunk, finals = found
    return bool(_lib.lib().mssvt_head_conv_supported(int(shared[0].in_channels), int(shared[0].out_channels), len(trunk),
                                                     max(int(c.out_channels) for c in finals)))


class Packed(object):
    """One stage as the kernel reads it: `blob` (uint8, device), the input channels `cin` (shared only), `s`, the branch
    count `nb` and, for the finals, every branch's map count `ks` and the maps before it `kbase`."""
    __slots__ = ("stage", "blob", "cin", "s", "nb", "ks", "kbase")

    def __init__(self, stage, blob, cin, s, nb, ks=()):
        self.stage, self.blob, self.cin, self.s, self.nb = stage, blob, cin, s, nb
        self.ks = tuple(int(k) for k in ks)
        self.kbase = tuple(sum(self.ks[:i]) for i in range(len(self.ks)))


def _params(conv, bn):
    return params(conv, bn, "head_conv")


def _blob(nbytes, device):
    if nbytes <= 0:
        raise MssvtHipError("head_conv: sizes not covered by the kernels")
    return torch.zeros(int(nbytes), dtype=torch.uint8, device=device)  # (the header's padding stays defined)


@torch.no_grad()
def pack_shared(conv, bn):
    cin, s = int(conv.in_channels), int(conv.out_channels)
    w, bias, bn_w, bn_b, bn_m, bn_v = _params(conv, bn)
    blob = _blob(_lib.lib().mssvt_head_conv_shared_pack_bytes(cin, s), w.device)
    with torch.cuda.device(w.device):
        _lib.call("mssvt_head_conv_shared_pack", _lib.ptr(w), _lib.ptr(bias), _lib.ptr(bn_w), _lib.ptr(bn_b), _lib.ptr(bn_m),
                  _lib.ptr(bn_v), 0.0 if bn is None else float(bn.eps), cin, s, _lib.ptr(blob), _lib.stream())
    return Packed("shared", blob, cin, s, 1)


@torch.no_grad()
def pack_trunk(pairs):
    """`pairs`: [(conv S -> S, bn)] per branch."""
    s, nb = int(pairs[0][0].in_channels), len(pairs)
    dev = pairs[0][0].weight.device
    blob = _blob(_lib.lib().mssvt_head_conv_trunk_pack_bytes(s, nb), dev)
    with torch.cuda.device(dev):
        for b, (conv, bn) in enumerate(pairs):
            w, bias, bn_w, bn_b, bn_m, bn_v = _params(conv, bn)
            if tuple(w.shape) != (s, s, 3, 3) or w.device != dev:
                raise MssvtHipError("head_conv.pack_trunk: every branch must be a 3x3 %d -> %d convolution on one GPU" % (s, s))
            _lib.call("mssvt_head_conv_trunk_pack", _lib.ptr(w), _lib.ptr(bias), _lib.ptr(bn_w), _lib.ptr(bn_b), _lib.ptr(bn_m),
                      _lib.ptr(bn_v), 0.0 if bn is None else float(bn.eps), s, nb, b, _lib.ptr(blob), _lib.stream())
    return Packed("trunk", blob, s, s, nb)


@torch.no_grad()
def pack_finals(convs):
    """`convs`: the last convolution S -> k_b (with bias) per branch."""
    s, nb = int(convs[0].in_channels), len(convs)
    dev = convs[0].weight.device
    blob = _blob(_lib.lib().mssvt_head_conv_finals_pack_bytes(s, nb), dev)
    packed = Packed("finals", blob, s, s, nb, [c.out_channels for c in convs])
    with torch.cuda.device(dev):
        for b, conv in enumerate(convs):
            w, bias = _params(conv, None)[:2]
            if tuple(w.shape) != (packed.ks[b], s, 3, 3) or w.device != dev:
                raise MssvtHipError("head_conv.pack_finals: every branch must be a 3x3 %d -> k convolution on one GPU" % s)
            _lib.call("mssvt_head_conv_finals_pack", _lib.ptr(w), _lib.ptr(bias), s, nb, b, packed.ks[b], packed.kbase[b],
                      _lib.ptr(blob), _lib.stream())
    return packed


_cache = weakref.WeakKeyDictionary()  # CenterHead -> (key, {stage: Packed})


def _key(found):
    shared, trunk, finals = found
    return tuple(pair_key(conv, bn) for conv, bn in [shared] + list(trunk) + [(c, None) for c in finals])


@torch.no_grad()
def pack(head):
    """{stage: Packed} of a covered head (cached per module; rebuilt when a parameter or running statistic changed).  Runs on
    the device on the current stream, no host read."""
    found = layers(head)
    if found is None or not supported(head):
        raise MssvtHipError("head_conv.pack: head not covered (%r)" % (head,))
    key = _key(found)
    hit = _cache.get(head)
    if hit is not None and hit[0] == key:
        return hit[1]
    shared, trunk, finals = found
    packs = dict(shared=pack_shared(*shared), trunk=pack_trunk(trunk), finals=pack_finals(finals))
    _cache[head] = (key, packs)
    return packs


def _check_rows(x, channels, what):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()
            and x.shape[3] == channels and min(x.shape) >= 1 and x.data_ptr() % 16 == 0):
        raise MssvtHipError("head_conv.%s needs a contiguous (B, H, W, %d) fp32 GPU tensor (no CPU path)" % (what, channels))
    if x.requires_grad and torch.is_grad_enabled():
        raise MssvtHipError("head_conv.%s is inference only (autograd is on for this input)" % what)


def expmap(x, channels):
    """The exponent words of a contiguous fp32 tensor read as rows of `channels` floats: int32, one per row."""
    rows = x.numel() // channels
    e = torch.empty(rows, dtype=torch.int32, device=x.device)
    _lib.call("mssvt_head_conv_expmap", x.data_ptr(), rows, channels, e.data_ptr(), _lib.stream())
    return e


def run_shared(packed, x):
    """x (B, H, W, cin) -> (y (B, H, W, S), y's exponent words (B H W))."""
    _check_rows(x, packed.cin, "run_shared")
    B, H, W, _ = x.shape
    y = torch.empty((B, H, W, packed.s), dtype=torch.float32, device=x.device)
    ws = torch.empty(B * H * W, dtype=torch.int32, device=x.device)
    e = torch.empty(B * H * W, dtype=torch.int32, device=x.device)
    _lib.call("mssvt_head_conv_shared", x.data_ptr(), B, H, W, packed.cin, packed.s, packed.blob.data_ptr(), ws.data_ptr(),
              y.data_ptr(), e.data_ptr(), _lib.stream())
    return y, e


def run_trunk(packed, x, e):
    """x (B, H, W, S) with its exponent words -> (t (B, H, W, nb S), words (B H W, nb): one per pixel and branch)."""
    _check_rows(x, packed.s, "run_trunk")
    B, H, W, _ = x.shape
    t = torch.empty((B, H, W, packed.nb * packed.s), dtype=torch.float32, device=x.device)
    e2 = torch.empty(B * H * W * packed.nb, dtype=torch.int32, device=x.device)
    _lib.call("mssvt_head_conv_trunk", x.data_ptr(), B, H, W, packed.s, packed.nb, packed.blob.data_ptr(), e.data_ptr(),
              t.data_ptr(), e2.data_ptr(), _lib.stream())
    return t, e2


def run_finals(packed, t, e2):
    """t (B, H, W, nb S) with words (B H W, nb) -> the branches' maps, each a contiguous (B, k_b, H, W) view of one buffer."""
    _check_rows(t, packed.nb * packed.s, "run_finals")
    B, H, W, _ = t.shape
    out = torch.empty(B * H * W * sum(packed.ks), dtype=torch.float32, device=t.device)
    _lib.call("mssvt_head_conv_finals", t.data_ptr(), B, H, W, packed.s, packed.nb, packed.blob.data_ptr(), e2.data_ptr(),
              out.data_ptr(), _lib.stream())
    n = B * H * W
    return [out[n * kb:n * (kb + k)].view(B, k, H, W) for k, kb in zip(packed.ks, packed.kbase)]


def applies(head, x):
    """True where ``CenterHead.forward`` sends its convolutions here: ``bev_conv.switch_applies`` (on, eval mode, autograd
    off, fp32 on the GPU, no AMP -- the module's ``use_amp`` or an autocast region around the call) and a covered head."""
    return switch_applies(head, x) and not torch.is_autocast_enabled() and x.dim() == 4 and min(x.shape) >= 1 \
        and supported(head) and head.shared_conv[0].weight.device == x.device


def routed_stages(x):
    """The stages of ``ROUTED`` that features `x` (B, Cin, H, W) take: the shared layer only if `x` is channels-last in
    memory or ``SHARED_FROM_NCHW`` is set."""
    return frozenset(st for st in ROUTED if st != "shared" or SHARED_FROM_NCHW or is_channels_last(x))


@torch.no_grad()
def forward(head, x):
    """`x` (B, Cin, H, W) fp32 on the GPU -> ``pred_dicts``: one dict per head, keys in ``sep_head_dict`` order, every value a
    contiguous (B, k, H, W) fp32 tensor.  NCHW features are converted once with ``contiguous(memory_format=channels_last)``
    where the shared layer runs on the kernel; where it runs through the library, it reads them as they arrive."""
    shared, trunk, finals = layers(head)
    s = int(shared[0].out_channels)
    routed = routed_stages(x)
    packs = pack(head)
    if "shared" in routed:
        if not is_channels_last(x):
            x = x.contiguous(memory_format=torch.channels_last)
        y, e = run_shared(packs["shared"], x.permute(0, 2, 3, 1))
    else:
        y = head.shared_conv(x).permute(0, 2, 3, 1).contiguous()
        e = expmap(y, s) if "trunk" in routed else None
    if "trunk" in routed:
        t, e2 = run_trunk(packs["trunk"], y, e)
    else:
        yv = y.permute(0, 3, 1, 2)
        t = torch.cat([seq[0](yv) for _, _, seq in branches(head)], dim=1).permute(0, 2, 3, 1).contiguous()
        e2 = expmap(t, s) if "finals" in routed else None
    if "finals" in routed:
        maps = run_finals(packs["finals"], t, e2)
    else:
        tv = t.permute(0, 3, 1, 2)
        maps = [conv(tv[:, b * s:(b + 1) * s]).contiguous() for b, conv in enumerate(finals)]
    pred_dicts = [dict() for _ in head.heads_list]
    for (i, name, _), m in zip(branches(head), maps):
        pred_dicts[i][name] = m
    return pred_dicts
