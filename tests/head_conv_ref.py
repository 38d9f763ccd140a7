"""float64 numpy statement of CenterHead's convolution stages (csrc/head_conv.hip), built on tests/bev_conv_ref.py: the shared
layer, the trunk (the first Conv + BN + ReLU of every branch as one convolution S -> nb S) and the finals (every branch's
last convolution on ITS slice of the trunk tensor, planar output), each with its per-element error bound

    (3 2^-22 + S 2^-24) (|x| conv |w|) + 2^-24 max|x| sum|w|,   S = steps(3, cin)

(tests/test_bev_conv_gpu.py derives it).  For the finals max|x| is taken over the branch's own slice: the kernel normalises
every branch on its own exponent words.  With a folded scale / shift (BatchNorm, bias) the fold's two fp32 roundings add
2^-23 (|scale| A + |shift|) and the bound itself is multiplied by |scale|, as in
test_bev_conv_gpu.py::test_batch_norm_fold_bias_and_transposed_layout.  Also the builders of small CenterHead modules that
the head tests share.  Not a test module: tests/test_head_conv_ref_cpu.py holds it to torch in float64."""
import numpy as np

from tests import bev_conv_ref as ref


def bn_dict(bn):
    """dict(mean, var, eps, weight, bias) of a torch BatchNorm2d (or None)."""
    if bn is None:
        return None
    return dict(mean=bn.running_mean.detach().cpu().numpy(), var=bn.running_var.detach().cpu().numpy(), eps=bn.eps,
                weight=None if bn.weight is None else bn.weight.detach().cpu().numpy(),
                bias=None if bn.bias is None else bn.bias.detach().cpu().numpy())


def conv(x, w, bias=None, bn=None, relu=False):
    """x (B, H, W, cin), w (cout, cin, 3, 3) -> (y (B, H, W, cout) float64 = act(scale conv + shift), a = |x| conv |w|,
    scale, shift)."""
    w = np.asarray(w, np.float64)
    scale, shift = ref.fold(w.shape[0], bias, bn)
    y, a = ref.conv(x, w, 1, 1, scale=scale, shift=shift, relu=relu)
    return y, a, scale, shift


def error_bound(a, x, w, scale=None, shift=None):
    """The per-element bound of the module docstring for x (B, H, W, cin), w (cout, cin, 3, 3) and a = |x| conv |w|; with a
    fold: |scale| bound + 2^-23 (|scale| a + |shift|)."""
    b = ref.error_bound(a, x, w, 3, np.asarray(w).shape[1])
    if scale is None:
        return b
    return np.abs(scale) * b + 2.0 ** -23 * (np.abs(scale) * a + np.abs(shift))


def stage(x, w, bias=None, bn=None, relu=False):
    """(y, bound) of one Conv (+ bias, + BatchNorm fold) (+ ReLU)."""
    y, a, scale, shift = conv(x, w, bias, bn, relu)
    plain = bias is None and bn is None
    return y, error_bound(a, x, w, None if plain else scale, None if plain else shift)


def trunk(x, branches):
    """branches: [(w (S, S, 3, 3), bias or None, bn dict or None)] -> (y (B, H, W, nb S), bound): branch b in columns
    [b S, (b + 1) S)."""
    ys, bs = zip(*[stage(x, w, bias, bn, relu=True) for w, bias, bn in branches])
    return np.concatenate(ys, axis=3), np.concatenate(bs, axis=3)


def finals(t, branches):
    """t (B, H, W, nb S), branches: [(w (k_b, S, 3, 3), bias (k_b) or None)] -> [(y_b (B, k_b, H, W), bound_b)]: every branch
    on its own S-channel slice, value AND bound (max|x| over the slice)."""
    s = np.asarray(branches[0][0]).shape[1]
    out = []
    for b, (w, bias) in enumerate(branches):
        y, bound = stage(np.asarray(t)[..., b * s:(b + 1) * s], w, bias, None, relu=False)
        out.append((y.transpose(0, 3, 1, 2), bound.transpose(0, 3, 1, 2)))
    return out


def planar(maps):
    """The finals' one buffer [branch][B][k_b][H][W] from the per-branch maps."""
    return np.concatenate([np.ascontiguousarray(m).ravel() for m in maps])


def exp_words(x, channels):
    """The largest |value| of every row of `channels` floats as float32 bits (int32): the kernels' exponent words."""
    rows = np.abs(np.asarray(x, np.float32).reshape(-1, channels))
    return rows.max(axis=1).view(np.int32)


def head_forward(sd, x, branch_names, relu=True):
    """A whole CenterHead's convolutions from its state dict (numpy values, the module's keys): x (B, H, W, cin) ->
    {(head index, name): (B, k, H, W)} float64.  branch_names: [[names of head 0], ...] in ``sep_head_dict`` order."""
    def bn(prefix):
        return dict(mean=sd[prefix + ".running_mean"], var=sd[prefix + ".running_var"], eps=sd["eps"],
                    weight=sd[prefix + ".weight"], bias=sd[prefix + ".bias"])

    y, _, _, _ = conv(x, sd["shared_conv.0.weight"], sd.get("shared_conv.0.bias"), bn("shared_conv.1"), relu=True)
    keys = [(i, n) for i, names in enumerate(branch_names) for n in names]
    pre = ["heads_list.%d.%s" % k for k in keys]
    t, _ = trunk(y, [(sd[p + ".0.0.weight"], sd.get(p + ".0.0.bias"), bn(p + ".0.1")) for p in pre])
    maps = finals(t, [(sd[p + ".1.weight"], sd[p + ".1.bias"]) for p in pre])
    return {k: m for k, (m, _) in zip(keys, maps)}


# ---- small CenterHead modules ------------------------------------------------------------------------------------------
CLASSES = ["Vehicle", "Pedestrian", "Cyclist"]


def head_config(shared=32, heads=None, vel=False, num_conv=None, fused=None, max_objs=50, post_max=30, score_thresh=0.1):
    """A DENSE_HEAD node: `heads` = CLASS_NAMES_EACH_HEAD, `num_conv` = {branch: layers} overrides (default 2 everywhere)."""
    num_conv = dict(num_conv or {})
    hd = {"center": 2, "center_z": 1, "dim": 3, "rot": 2}
    if vel:
        hd["vel"] = 2
    cfg = dict(CLASS_AGNOSTIC=False, CLASS_NAMES_EACH_HEAD=heads or [list(CLASSES)], SHARED_CONV_CHANNEL=shared,
               USE_BIAS_BEFORE_NORM=True, NUM_HM_CONV=int(num_conv.get("hm", 2)),
               SEPARATE_HEAD_CFG=dict(HEAD_ORDER=list(hd), HEAD_DICT={k: dict(out_channels=v, num_conv=int(num_conv.get(k, 2)))
                                                                     for k, v in hd.items()}),
               TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=1, NUM_MAX_OBJS=500, GAUSSIAN_OVERLAP=0.1, MIN_RADIUS=2),
               POST_PROCESSING=dict(SCORE_THRESH=score_thresh, POST_CENTER_LIMIT_RANGE=[-100.0, -100.0, -10.0, 100.0, 100.0, 10.0],
                                    MAX_OBJ_PER_SAMPLE=max_objs,
                                    NMS_CONFIG=dict(NMS_TYPE="nms_gpu", NMS_THRESH=0.5, NMS_PRE_MAXSIZE=200, NMS_POST_MAXSIZE=post_max)))
    if fused is not None:
        cfg["FUSED_CONVS"] = fused
    return cfg


def build_head(cin, seed=0, **kw):
    """An eval-mode CenterHead on `cin` input channels with random BatchNorm statistics and heat-map biases that let some
    peaks pass the score threshold."""
    import torch
    from mssvt_amd.center_head import CenterHead
    from mssvt_amd.config import Config
    torch.manual_seed(seed)
    head = CenterHead(Config.wrap(head_config(**kw)), cin, len(CLASSES), CLASSES, np.array([40, 40, 1]),
                      np.array([-20.0, -20.0, -2.0, 20.0, 20.0, 4.0]), [1.0, 1.0, 6.0], predict_boxes_when_training=False).eval()
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in head.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
        for sep in head.heads_list:
            sep.hm[-1].bias.fill_(-1.0)
    return head
