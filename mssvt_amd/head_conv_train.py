"""``CenterHead``'s shared layer and trunk in TRAINING mode on split-fp16 matrix instructions (csrc/head_conv.hip).

The head's eleven 3 x 3 convolutions (ref pcdet/models/dense_heads/center_head.py: shared_conv :76-84, SeparateHead :11-46) are
the shared layer Cin -> S, the first convolution S -> S of every branch (the "trunk") and the last one S -> k_b (the
"finals").  This module trains the first two on the project's kernels; the finals (64 -> 1 .. 3 channels, under 2 % of the work)
stay torch modules, as do every BatchNorm2d and ReLU unless ``fused_bn`` routes them.

``SharedFunction.apply(x, weight, bias_or_None)`` is ``y = conv2d(x, weight, bias, padding=1)``: x (B, Cin, H, W) fp32 on the
GPU (made channels-last), y (B, S, H, W), channels-last in memory.

    forward   mssvt_head_conv_shared_train: the inference kernel with scale 1, shift = bias, no ReLU;
    dX        mssvt_head_conv_shared_dgrad: the convolution S -> Cin over dY, taps rotated, channel axes swapped; skipped when
              the input needs no gradient;
    dW        mssvt_head_conv_shared_wgrad: ``bev_conv_train.conv_wgrad``'s kernel on S x S tiles of (S, Cin);
    db        mssvt_head_conv_bgrad: ordered sums over the pixels; skipped without a bias.

``TrunkFunction.apply(y, nb, *weights_then_biases)`` is the nb convolutions ``t_b = conv2d(y, W_b, bias_b, padding=1)`` reading
one y (B, S, H, W): a tuple of nb (B, S, H, W) tensors, channels-last views of ONE buffer [nb][B][H][W][S] (no ``torch.cat``, no
copy in front of the per-branch BatchNorm).  The arguments are the nb weights followed by the nb biases (None where absent).

    forward   mssvt_head_conv_trunk_train: one launch, branch-major output;
    dy        mssvt_head_conv_trunk_dgrad: the sum over the branches in ONE launch with one accumulation chain per element, from
              the nb upstream gradients as autograd hands them back (a host array of device pointers: no ``torch.stack``);
    dW        mssvt_head_conv_trunk_wgrad: one launch, every branch normalised on its own gradient;
    db        mssvt_head_conv_bgrad per branch, one launch.

An absent upstream gradient counts as zero.  The weights are repacked on every call (they change every step).  No float atomics:
the results are bit-identical from step to step.

``ROUTED_TRAIN`` lists the stages ``CenterHead.fused_train`` sends here at the product shape: those whose slowest forward +
backward beat the library's fastest at B = 1 and B = 4 in tools/time_head_conv_train.py (profiles/head_conv_train_times.json,
DESIGN section 5.5's rule).  ``ROUTED_BN`` lists the widths whose BatchNorm2d + ReLU pairs behind a routed stage go through
``bn_train.bn_relu`` when ``CenterHead.fused_bn`` is on as well, by the same rule on the same file.  A stage that did not clear
stays reachable through its Function.
"""
import ctypes

import torch
from torch.autograd.function import once_differentiable

from . import _lib, bev_conv, head_conv
from ._lib import MssvtHipError

STAGES = ("shared", "trunk")
# the stages that cleared the routing rule on an MI355X at the mssvt.yaml head shape (512 -> 64, five branches, 470 x 470;
# profiles/head_conv_train_times.json, slowest forward + backward against the library's fastest over BOTH records): the shared
# layer cleared everywhere, 3.06 / 3.63 ms (B = 1) and 12.04 / 14.40 ms (B = 4).  The trunk cleared the first record (2.37 / 3.13
# and 9.15 / 12.41 ms) and lost the second at B = 1 on one run of twenty (3.48 ms; the other nineteen 2.32 .. 2.45 ms, against the
# library's fastest 3.11 ms): it stays out and reachable through TrunkFunction
ROUTED_TRAIN = frozenset({"shared"})
# the BatchNorm widths that cleared it (the same file; 64 is the head's product width): 64 cleared at B = 4 in both records and at
# B = 1 in the second (0.127 / 0.189 ms) but lost at B = 1 in the first (0.191 .. 0.235 ms against the library's fastest 0.192 ms),
# so it stays out and reachable through bn_train
ROUTED_BN = frozenset()
# the narrow shape (Cin, S) exists for small module tests: never timed, routed whenever the switch is on, and with fused_bn so are
# the BatchNorms of such a head (a product head with S = 32 is not narrow: its width must be in ROUTED_BN)
NARROW_SHAPES = frozenset({(64, 32)})


def slice_pixels(cin, s):
    """Pixels per slice of the weight-gradient kernel for a layer cin -> s (the trunk: cin = s); 0: not covered."""
    return int(_lib.lib().mssvt_head_conv_train_wgrad_slice_pixels(cin, s))


def bias_piece_rows(s):
    """Pixels per piece of the bias-gradient kernel (0: not covered)."""
    return int(_lib.lib().mssvt_head_conv_train_bias_piece_rows(s))


def _nhwc(t):
    return t if bev_conv.is_channels_last(t) else t.contiguous(memory_format=torch.channels_last)


def _check(who, *tensors):
    for t in tensors:
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and bev_conv.is_channels_last(t)
                and min(t.shape) >= 1):
            raise MssvtHipError("head_conv_train.%s needs 4-D fp32 GPU tensors that are channels-last in memory (no CPU path)" % who)


def _vector(who, t, n, device):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dtype == torch.float32):
        raise MssvtHipError("head_conv_train.%s needs fp32 parameters on the input's GPU" % who)
    t = t.detach().contiguous()
    if t.numel() != n:
        raise MssvtHipError("head_conv_train.%s: a parameter has %d elements, not %d" % (who, t.numel(), n))
    return t


def _bytes(name, *sizes):
    n = int(getattr(_lib.lib(), name)(*sizes))
    if n <= 0:
        raise MssvtHipError("%s%r refused the size" % (name, sizes))
    return n


def _empty(n, device, dtype=torch.uint8):
    return torch.empty(int(n), dtype=dtype, device=device)


def _pointers(tensors):
    """The host array of device pointers the trunk's entry points read during the call."""
    addresses = [t.data_ptr() for t in tensors]
    return (ctypes.c_void_p * len(addresses))(*addresses)


# ---- the shared layer -----------------------------------------------------------------------------------------------------------
def shared_forward(x, weight, bias=None):
    """x (B, Cin, H, W) channels-last, weight (S, Cin, 3, 3), bias (S) or None -> y (B, S, H, W), channels-last."""
    _check("shared_forward", x)
    B, cin, H, W = x.shape
    s = int(weight.shape[0])
    if tuple(weight.shape) != (s, cin, 3, 3) or not _lib.lib().mssvt_head_conv_train_supported(cin, s, 1):
        raise MssvtHipError("head_conv_train.shared_forward: shape not covered (x %s, weight %s)" % (tuple(x.shape), tuple(weight.shape)))
    w = _vector("shared_forward", weight, s * cin * 9, x.device)
    b = None if bias is None else _vector("shared_forward", bias, s, x.device)
    blob = torch.zeros(_bytes("mssvt_head_conv_shared_pack_bytes", cin, s), dtype=torch.uint8, device=x.device)
    words = _empty(B * H * W, x.device, torch.int32)
    y = _empty(B * H * W * s, x.device, torch.float32).view(B, H, W, s)
    with torch.cuda.device(x.device):
        _lib.call("mssvt_head_conv_shared_pack", w.data_ptr(), _lib.addr(b), None, None, None, None, 0.0, cin, s, blob.data_ptr(),
                  _lib.stream())
        _lib.call("mssvt_head_conv_shared_train", x.data_ptr(), B, H, W, cin, s, blob.data_ptr(), words.data_ptr(), y.data_ptr(),
                  _lib.stream())
    return y.permute(0, 3, 1, 2)


def shared_dgrad(dy, weight):
    """dy (B, S, H, W) channels-last, weight (S, Cin, 3, 3) -> dx (B, Cin, H, W), channels-last."""
    _check("shared_dgrad", dy)
    B, s, H, W = dy.shape
    cin = int(weight.shape[1])
    w = _vector("shared_dgrad", weight, s * cin * 9, dy.device)
    ws = _empty(_bytes("mssvt_head_conv_shared_dgrad_workspace_bytes", B, H, W, cin, s), dy.device)
    dx = _empty(B * H * W * cin, dy.device, torch.float32).view(B, H, W, cin)
    with torch.cuda.device(dy.device):
        _lib.call("mssvt_head_conv_shared_dgrad", dy.data_ptr(), w.data_ptr(), B, H, W, cin, s, dx.data_ptr(), ws.data_ptr(),
                  _lib.stream())
    return dx.permute(0, 3, 1, 2)


def shared_wgrad(x, dy):
    """x (B, Cin, H, W), dy (B, S, H, W), channels-last -> dw (S, Cin, 3, 3)."""
    _check("shared_wgrad", x, dy)
    B, cin, H, W = x.shape
    s = int(dy.shape[1])
    if tuple(dy.shape) != (B, s, H, W) or dy.device != x.device:
        raise MssvtHipError("head_conv_train.shared_wgrad: x is %s, dy is %s" % (tuple(x.shape), tuple(dy.shape)))
    ws = _empty(_bytes("mssvt_head_conv_shared_wgrad_workspace_bytes", B, H, W, cin, s), x.device)
    dw = _empty(s * cin * 9, x.device, torch.float32).view(s, cin, 3, 3)
    with torch.cuda.device(x.device):
        _lib.call("mssvt_head_conv_shared_wgrad", x.data_ptr(), dy.data_ptr(), B, H, W, cin, s, dw.data_ptr(), ws.data_ptr(),
                  _lib.stream())
    return dw


def bias_grad(dys):
    """dys: nb tensors (B, S, H, W), channels-last -> db (nb, S): the sums over the pixels in the kernel's fixed order."""
    _check("bias_grad", *dys)
    B, s, H, W = dys[0].shape
    nb = len(dys)
    if any(tuple(t.shape) != (B, s, H, W) or t.device != dys[0].device for t in dys):
        raise MssvtHipError("head_conv_train.bias_grad: the gradients must share one shape and GPU")
    ws = _empty(_bytes("mssvt_head_conv_bgrad_workspace_bytes", B, H, W, s, nb), dys[0].device)
    db = _empty(nb * s, dys[0].device, torch.float32).view(nb, s)
    with torch.cuda.device(dys[0].device):
        _lib.call("mssvt_head_conv_bgrad", _pointers(dys), B, H, W, s, nb, db.data_ptr(), ws.data_ptr(), _lib.stream())
    return db


class SharedFunction(torch.autograd.Function):
    """``SharedFunction.apply(x, weight, bias_or_None)``."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x = _nhwc(x)
        y = shared_forward(x, weight, bias)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = _nhwc(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = shared_dgrad(dy, weight)
        if ctx.needs_input_grad[1]:
            dw = shared_wgrad(x, dy)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = bias_grad([dy])[0]
        return dx, dw, db


# ---- the trunk ------------------------------------------------------------------------------------------------------------------
def _trunk_weights(who, weights, s, device):
    return [_vector(who, w, s * s * 9, device) for w in weights]


def trunk_forward(y, weights, biases):
    """y (B, S, H, W) channels-last, nb weights (S, S, 3, 3), nb biases (S) or None -> nb (B, S, H, W) views of one buffer."""
    _check("trunk_forward", y)
    B, s, H, W = y.shape
    nb = len(weights)
    if nb < 1 or len(biases) != nb or any(tuple(w.shape) != (s, s, 3, 3) for w in weights) \
            or not _lib.lib().mssvt_head_conv_train_supported(64, s, nb):
        raise MssvtHipError("head_conv_train.trunk_forward: shape not covered (y %s, %d branches)" % (tuple(y.shape), nb))
    ws = _trunk_weights("trunk_forward", weights, s, y.device)
    bs = [None if b is None else _vector("trunk_forward", b, s, y.device) for b in biases]
    blob = torch.zeros(_bytes("mssvt_head_conv_trunk_pack_bytes", s, nb), dtype=torch.uint8, device=y.device)
    words = _empty(B * H * W, y.device, torch.int32)
    t = _empty(nb * B * H * W * s, y.device, torch.float32).view(nb, B, H, W, s)
    with torch.cuda.device(y.device):
        for b in range(nb):
            _lib.call("mssvt_head_conv_trunk_pack", ws[b].data_ptr(), _lib.addr(bs[b]), None, None, None, None, 0.0, s, nb, b,
                      blob.data_ptr(), _lib.stream())
        _lib.call("mssvt_head_conv_trunk_train", y.data_ptr(), B, H, W, s, nb, blob.data_ptr(), words.data_ptr(), t.data_ptr(),
                  _lib.stream())
    return tuple(t[b].permute(0, 3, 1, 2) for b in range(nb))


def trunk_dgrad(dts, weights):
    """dts: nb tensors (B, S, H, W) channels-last, weights: nb (S, S, 3, 3) -> dy (B, S, H, W), channels-last."""
    _check("trunk_dgrad", *dts)
    B, s, H, W = dts[0].shape
    nb = len(dts)
    if len(weights) != nb or any(tuple(t.shape) != (B, s, H, W) or t.device != dts[0].device for t in dts):
        raise MssvtHipError("head_conv_train.trunk_dgrad: the gradients must share one shape and GPU, one weight per gradient")
    w = _trunk_weights("trunk_dgrad", weights, s, dts[0].device)
    ws = _empty(_bytes("mssvt_head_conv_trunk_dgrad_workspace_bytes", B, H, W, s, nb), dts[0].device)
    dy = _empty(B * H * W * s, dts[0].device, torch.float32).view(B, H, W, s)
    with torch.cuda.device(dts[0].device):
        _lib.call("mssvt_head_conv_trunk_dgrad", _pointers(dts), _pointers(w), B, H, W, s, nb, dy.data_ptr(), ws.data_ptr(),
                  _lib.stream())
    return dy.permute(0, 3, 1, 2)


def trunk_wgrad(y, dts):
    """y (B, S, H, W), dts: nb tensors (B, S, H, W), channels-last -> dw (nb, S, S, 3, 3): branch b's gradient is dw[b]."""
    _check("trunk_wgrad", y, *dts)
    B, s, H, W = y.shape
    nb = len(dts)
    if any(tuple(t.shape) != (B, s, H, W) or t.device != y.device for t in dts):
        raise MssvtHipError("head_conv_train.trunk_wgrad: y is %s, the gradients must have its shape and GPU" % (tuple(y.shape),))
    ws = _empty(_bytes("mssvt_head_conv_trunk_wgrad_workspace_bytes", B, H, W, s, nb), y.device)
    dw = _empty(nb * s * s * 9, y.device, torch.float32).view(nb, s, s, 3, 3)
    with torch.cuda.device(y.device):
        _lib.call("mssvt_head_conv_trunk_wgrad", y.data_ptr(), _pointers(dts), B, H, W, s, nb, dw.data_ptr(), ws.data_ptr(),
                  _lib.stream())
    return dw


class TrunkFunction(torch.autograd.Function):
    """``TrunkFunction.apply(y, nb, *weights_then_biases)``: nb weights, then nb biases (None where a branch has none)."""

    @staticmethod
    def forward(ctx, y, nb, *params):
        nb = int(nb)
        if len(params) != 2 * nb:
            raise MssvtHipError("head_conv_train.TrunkFunction takes nb weights followed by nb biases (None where absent)")
        y = _nhwc(y)
        weights, biases = params[:nb], params[nb:]
        out = trunk_forward(y, weights, biases)
        ctx.save_for_backward(y, *weights)
        ctx.nb = nb
        ctx.has_bias = tuple(b is not None for b in biases)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, *dts):
        y, weights = ctx.saved_tensors[0], ctx.saved_tensors[1:]
        nb = ctx.nb
        # (autograd materialises an absent upstream gradient as zeros)
        dts = [_nhwc(torch.zeros_like(y) if d is None else d) for d in dts]
        need = ctx.needs_input_grad
        dy = trunk_dgrad(dts, weights) if need[0] else None
        dws = [None] * nb
        if any(need[2:2 + nb]):
            dw = trunk_wgrad(y, dts)
            dws = [dw[b] if need[2 + b] else None for b in range(nb)]
        dbs = [None] * nb
        if any(ctx.has_bias[b] and need[2 + nb + b] for b in range(nb)):
            db = bias_grad(dts)
            dbs = [db[b] if ctx.has_bias[b] and need[2 + nb + b] else None for b in range(nb)]
        return (dy, None) + tuple(dws) + tuple(dbs)


# ---- the module path ------------------------------------------------------------------------------------------------------------
def train_supported(head):
    """The structure test of ``head_conv.layers`` (the convolutions with or without bias) and the sizes the kernels cover."""
    found = head_conv.layers(head)
    if found is None:
        return False
    shared, trunk, _ = found
    conv = shared[0]
    if not conv.weight.is_cuda or any(c.weight.device != conv.weight.device for c, _ in trunk):
        return False
    return bool(_lib.lib().mssvt_head_conv_train_supported(int(conv.in_channels), int(conv.out_channels), len(trunk)))


def applies(head, x):
    """True where ``CenterHead.forward`` takes ``forward_train``: the switch on, training mode, autograd on, fp32 on the GPU,
    no AMP (the module's ``use_amp`` or an autocast region around the call) and a covered head."""
    return bool(getattr(head, "fused_train", False)) and head.training and torch.is_grad_enabled() \
        and not getattr(head, "use_amp", False) and isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 \
        and not torch.is_autocast_enabled() and x.dim() == 4 and min(x.shape) >= 1 and train_supported(head) \
        and head.shared_conv[0].weight.device == x.device


def _narrow(head):
    conv = head.shared_conv[0]
    return (int(conv.in_channels), int(conv.out_channels)) in NARROW_SHAPES


def routed_stages(head):
    """The stages of a covered head that go through the Functions: ``ROUTED_TRAIN``, or both for a narrow shape."""
    if _narrow(head):
        return frozenset(STAGES)
    return ROUTED_TRAIN


def _bn_relu(head, bn, relu, x):
    """The BatchNorm2d + ReLU pair behind a routed stage: ``bn_train.bn_relu`` with ``fused_bn`` for a width of ``ROUTED_BN``
    (or a narrow one), else the modules."""
    if getattr(head, "fused_bn", False) and (bn.num_features in ROUTED_BN or _narrow(head)):
        from . import bn_train
        if bn_train.bn_supported(bn):
            return bn_train.bn_relu(bn, x, True)
    return relu(bn(x))


def forward_train(head, x):
    """`x` (B, Cin, H, W) fp32 on the GPU -> ``pred_dicts`` as ``CenterHead.forward`` builds them in training mode: one dict
    per head, keys in ``sep_head_dict`` order, every value (B, k, H, W).  A routed stage runs through its Function and the
    BatchNorm2d, ReLU and final convolutions behind it as the modules they are, on the dense channels-last tensors; an
    unrouted stage runs as modules."""
    shared, trunk, finals = head_conv.layers(head)
    routed = routed_stages(head)
    if "shared" in routed:
        y = SharedFunction.apply(x, shared[0].weight, shared[0].bias)
        y = _bn_relu(head, shared[1], head.shared_conv[2], y)
    else:
        y = head.shared_conv(x)
    names = head_conv.branches(head)
    if "trunk" in routed:
        ts = TrunkFunction.apply(y, len(trunk), *([c.weight for c, _ in trunk] + [c.bias for c, _ in trunk]))
        maps = [final(_bn_relu(head, bn, seq[0][2], t)) for (_, _, seq), (_, bn), final, t in zip(names, trunk, finals, ts)]
    else:
        maps = [seq(y) for _, _, seq in names]
    pred_dicts = [dict() for _ in head.heads_list]
    for (i, name, _), m in zip(names, maps):
        pred_dicts[i][name] = m
    return pred_dicts
