"""``BaseBEVBackbone`` -- the 2-D BEV backbone behind HeightCompression.

Drop-in for pcdet/models/backbones_2d/base_bev_backbone.py:6-114: constructor ``(model_cfg, input_channels)``, the
config keys LAYER_NUMS / LAYER_STRIDES / NUM_FILTERS / UPSAMPLE_STRIDES / NUM_UPSAMPLE_FILTERS, ``num_bev_features``,
``forward(data_dict)`` reading ``spatial_features`` and writing ``spatial_features_2d`` (+ ``spatial_features_{s}x``),
and the state-dict keys ``blocks.{i}.{k}.*`` / ``deblocks.{i}.{k}.*`` (a reference checkpoint loads by key).  Dense
convolutions run through the library (MIOpen) -- they are not on the sparse hot path.

``fused_convs`` (off by default; yaml key ``FUSED_CONVS``): in eval mode with autograd off, an fp32 GPU input and ``AMP`` off,
the tensors are channels-last and every Conv + BN + ReLU triple that ``bev_conv.routed`` accepts (the 1x1 stride-1 deblock
included) runs on the split-fp16 kernel of csrc/bev_conv.hip; the 2x2 stride-2 transposed deblock and any other layer run
through the library on the same tensors.  Shapes and ``data_dict`` keys are unchanged, only strides differ.

``fused_deblocks`` (off by default; yaml key ``FUSED_DEBLOCKS``) takes effect only where ``fused_convs`` does and only with it
on, in a module with one deblock per block and more than one of them: the concatenated ``(B, H, W, sum of upsample filters)``
tensor is allocated once and every deblock writes its own channel slice of it -- a routed 1x1 stride-1 deblock through
``bev_conv.conv_bn_act(out=, channel=)``, a 2x2 stride-2 transposed deblock that ``bev_conv.up2_routed`` accepts through
``bev_conv.up2_bn_act``, any other through the library and a copy into its slice.  There is no ``torch.cat``.

``fused_train`` (off by default; yaml key ``FUSED_TRAIN``, named like ``DynamicVFE``'s): in training mode with autograd on, an
fp32 GPU input and ``AMP`` off, blocks and deblocks run channels-last through ``bev_conv_train.run_layers_train``: every
convolution ``bev_conv_train.train_routed`` accepts (3 x 3, stride 1, cin = cout) on the split-fp16 kernels -- forward, input
gradient and weight gradient; the stride-2 layer (unless ``fused_train_down``), the deblocks, BatchNorm in training mode and
ReLU stay torch modules.

``fused_bn`` (off by default; yaml key ``FUSED_BN``) takes effect only where and when ``fused_train`` does: every BatchNorm2d
that ``bn_train.bn_routed`` accepts then runs, together with the ReLU behind it, through ``bn_train.BnReluFunction`` -- the
kernels of csrc/bn_train.hip, forward and backward, bit-identical from step to step -- instead of as torch modules.

``fused_train_deblocks`` (off by default; yaml key ``FUSED_TRAIN_DEBLOCKS``) takes effect only where and when ``fused_train``
does, on its own it does nothing: every ``ConvTranspose2d`` deblock that ``bev_deblock_train.deblock_train_routed`` accepts
(kernel = stride in {1, 2}, no bias, a routed shape) then runs through ``bev_deblock_train.DeblockFunction`` -- forward, input
gradient and weight gradient on the split-fp16 kernels.  An unrouted deblock, the trailing deblock over the concatenated
tensor and fractional strides stay modules; BatchNorm + ReLU behind the deblock and ``torch.cat`` stay as they are.

``fused_train_down`` (off by default; yaml key ``FUSED_TRAIN_DOWN``) takes effect only where and when ``fused_train`` does, on
its own it does nothing: the 3 x 3 stride-2 convolution at the head of a block (``ZeroPad2d(1)`` + padding 0, or padding 1)
that ``bev_down_train.down_train_routed`` accepts then runs through ``bev_down_train.DownFunction`` -- forward on the
inference kernel, input gradient as four parity phases and weight gradient on the split-fp16 kernels.  An unrouted shape
stays a module."""
import torch
from torch import nn


def _get(cfg, key, default=None):
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


class BaseBEVBackbone(nn.Module):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums = list(_get(model_cfg, "LAYER_NUMS", None) or [])
        layer_strides = list(_get(model_cfg, "LAYER_STRIDES", None) or [])
        num_filters = list(_get(model_cfg, "NUM_FILTERS", None) or [])
        assert len(layer_nums) == len(layer_strides) == len(num_filters)
        up_strides = list(_get(model_cfg, "UPSAMPLE_STRIDES", None) or [])
        up_filters = list(_get(model_cfg, "NUM_UPSAMPLE_FILTERS", None) or [])
        assert len(up_strides) == len(up_filters)
        bn = lambda c: nn.BatchNorm2d(c, eps=1e-3, momentum=0.01)  # noqa: E731
        c_in = [input_channels] + num_filters[:-1]
        self.blocks, self.deblocks = nn.ModuleList(), nn.ModuleList()
        for i, (n_layers, stride, width) in enumerate(zip(layer_nums, layer_strides, num_filters)):
            layers = [nn.ZeroPad2d(1), nn.Conv2d(c_in[i], width, kernel_size=3, stride=stride, padding=0, bias=False),
                      bn(width), nn.ReLU()]
            for _ in range(n_layers):
                layers += [nn.Conv2d(width, width, kernel_size=3, padding=1, bias=False), bn(width), nn.ReLU()]
            self.blocks.append(nn.Sequential(*layers))
            if up_strides:
                s = up_strides[i]
                if s >= 1:
                    up = nn.ConvTranspose2d(width, up_filters[i], s, stride=s, bias=False)
                else:  # a fractional stride downsamples (ref :59-69)
                    k = int(round(1.0 / s))
                    up = nn.Conv2d(width, up_filters[i], k, stride=k, bias=False)
                self.deblocks.append(nn.Sequential(up, bn(up_filters[i]), nn.ReLU()))
        c_out = sum(up_filters)
        if len(up_strides) > len(layer_nums):
            self.deblocks.append(nn.Sequential(
                nn.ConvTranspose2d(c_out, c_out, up_strides[-1], stride=up_strides[-1], bias=False), bn(c_out), nn.ReLU()))
        self.num_bev_features = c_out
        self.use_amp = bool(_get(model_cfg, "AMP", False))
        self.fused_convs = bool(_get(model_cfg, "FUSED_CONVS", False))
        self.fused_deblocks = bool(_get(model_cfg, "FUSED_DEBLOCKS", False))
        self.fused_train = bool(_get(model_cfg, "FUSED_TRAIN", False))
        self.fused_bn = bool(_get(model_cfg, "FUSED_BN", False))
        self.fused_train_deblocks = bool(_get(model_cfg, "FUSED_TRAIN_DEBLOCKS", False))
        self.fused_train_down = bool(_get(model_cfg, "FUSED_TRAIN_DOWN", False))
        self._up_filters = [int(c) for c in up_filters[:len(layer_nums)]]

    def _deblock_into(self, bev_conv, deblock, x, out, channel):
        """`deblock`(x) written into channels [channel, ...) of `out` (None: allocated here from the first result's size)."""
        layers = list(deblock)
        conv, bn = layers[0], layers[1] if len(layers) > 1 and isinstance(layers[1], nn.BatchNorm2d) else None
        relu = len(layers) == 3 and isinstance(layers[2], nn.ReLU)
        whole = bn is not None and len(layers) == (3 if relu else 2)  # Conv + BN (+ ReLU) and nothing else
        up2 = whole and bev_conv.up2_routed(conv, bn)
        if up2 or (whole and bev_conv.routed(conv, bn) and conv.stride[0] == 1):
            s = 2 if up2 else 1
            if out is None:
                out = torch.empty((x.shape[0], s * x.shape[2], s * x.shape[3], sum(self._up_filters)), dtype=torch.float32,
                                  device=x.device).permute(0, 3, 1, 2)
            if up2:
                bev_conv.up2_bn_act(x, bev_conv.pack_up2(conv, bn), relu, out=out, channel=channel)
            else:
                bev_conv.conv_bn_act(x, bev_conv.pack(conv, bn), relu, out=out, channel=channel)
            return out
        y = bev_conv.run_layers(deblock, x)
        if out is None:
            out = torch.empty((y.shape[0], y.shape[2], y.shape[3], sum(self._up_filters)), dtype=torch.float32,
                              device=y.device).permute(0, 3, 1, 2)
        out[:, channel:channel + y.shape[1]].copy_(y)
        return out

    def _forward_fused(self, data_dict, feats):
        from . import bev_conv
        x, ups = feats.contiguous(memory_format=torch.channels_last), []
        into = self.fused_deblocks and len(self.blocks) > 1 and len(self.deblocks) >= len(self.blocks)
        cat, channel = None, 0  # (into: the concatenated tensor, every deblock writing its own channel slice)
        for i, blk in enumerate(self.blocks):
            x = bev_conv.run_layers(blk, x)
            data_dict["spatial_features_%dx" % int(feats.shape[2] / x.shape[2])] = x
            if into:
                cat = self._deblock_into(bev_conv, self.deblocks[i], x, cat, channel)
                channel += self._up_filters[i]
            else:
                ups.append(bev_conv.run_layers(self.deblocks[i], x) if len(self.deblocks) > 0 else x)
        if into:
            x = cat
        elif len(ups) > 1:
            x = torch.cat(ups, dim=1)
        elif len(ups) == 1:
            x = ups[0]
        if len(self.deblocks) > len(self.blocks):
            x = bev_conv.run_layers(self.deblocks[-1], x)
        data_dict["spatial_features_2d"] = x
        return data_dict

    def _forward_train(self, data_dict, feats):
        from .bev_conv_train import run_layers_train
        x, ups = feats.contiguous(memory_format=torch.channels_last), []
        for i, blk in enumerate(self.blocks):
            x = run_layers_train(blk, x, fused_bn=self.fused_bn, fused_down=self.fused_train_down)
            data_dict["spatial_features_%dx" % int(feats.shape[2] / x.shape[2])] = x
            ups.append(run_layers_train(self.deblocks[i], x, fused_bn=self.fused_bn, fused_deblocks=self.fused_train_deblocks)
                       if len(self.deblocks) > 0 else x)
        if len(ups) > 1:
            x = torch.cat(ups, dim=1)
        elif len(ups) == 1:
            x = ups[0]
        if len(self.deblocks) > len(self.blocks):
            x = run_layers_train(self.deblocks[-1], x, fused_bn=self.fused_bn)  # (the trailing deblock stays a module)
        data_dict["spatial_features_2d"] = x
        return data_dict

    def forward(self, data_dict):
        feats = data_dict["spatial_features"]
        if self.fused_train:
            from . import bev_conv_train
            if bev_conv_train.switch_applies(self, feats):
                return self._forward_train(data_dict, feats)
        if self.fused_convs:
            from . import bev_conv
            if bev_conv.switch_applies(self, feats):
                return self._forward_fused(data_dict, feats)
        with torch.autocast(device_type=feats.device.type, enabled=self.use_amp and feats.is_cuda):
            x, ups = feats, []
            for i, blk in enumerate(self.blocks):
                x = blk(x)
                data_dict["spatial_features_%dx" % int(feats.shape[2] / x.shape[2])] = x
                ups.append(self.deblocks[i](x) if len(self.deblocks) > 0 else x)
            if len(ups) > 1:
                x = torch.cat(ups, dim=1)
            elif len(ups) == 1:
                x = ups[0]
            if len(self.deblocks) > len(self.blocks):
                x = self.deblocks[-1](x)
        data_dict["spatial_features_2d"] = x.float()
        return data_dict
