"""Detector shell: ``CenterPoint`` over the MsSVT backbone, the way mssvt.yaml wires it.

Mirrors the reference's ``Detector3DTemplate`` (pcdet/models/detectors/detector3d_template.py:14-173: module topology
vfe -> backbone_3d -> map_to_bev_module -> backbone_2d -> dense_head, each built from its config node and registered
under that attribute name, so state-dict keys read ``vfe.*``, ``backbone_3d.backbone.{i}.*``, ``map_to_bev_module.*``,
``backbone_2d.*``, ``dense_head.*``), ``CenterPoint.forward`` / ``post_processing`` (detectors/centerpoint.py:4-50) in
eval mode with the recall bookkeeping of ``generate_recall_record`` (detector3d_template.py:286-328: with ``gt_boxes`` in
the batch, ``det(batch)`` returns ``(pred_dicts, recall_dict)`` for the eval loop to sum; the 3-D IoU comes from
csrc/box_iou.hip, trimming and counting stay on the device, one read-back per batch), and the checkpoint loaders
``load_params_from_file`` / ``_load_state_dict`` (:330-372: update by key where the shapes agree, report what stayed).
The dataset classes, dataset-level AP evaluation and the spconv weight layout adaptation (no spconv module exists here)
are out of scope."""
import contextlib
import os
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from .base_bev_backbone import BaseBEVBackbone
from . import iou3d_nms_utils
from .center_head import CenterHead, unpad
from .dynamic_vfe import DynamicVFE
from .height_compression import HeightCompression
from .mssvt_backbone import MixedScaleSparseTransformer

VFE = {"DynamicVFE": DynamicVFE}
BACKBONES_3D = {"MixedScaleSparseTransformer": MixedScaleSparseTransformer}
MAP_TO_BEV = {"HeightCompression": HeightCompression}
BACKBONES_2D = {"BaseBEVBackbone": BaseBEVBackbone}
DENSE_HEADS = {"CenterHead": CenterHead}


def dataset_info(cfg, num_point_features=5):
    """What the reference's detector reads from its dataset object (detector3d_template.py:36-44), from the yaml."""
    pcr = np.array(cfg.DATA_CONFIG.POINT_CLOUD_RANGE, dtype=np.float64)
    vs = next(p["VOXEL_SIZE"] for p in cfg.DATA_CONFIG.DATA_PROCESSOR if "VOXEL_SIZE" in p)
    grid = np.round((pcr[3:6] - pcr[0:3]) / np.array(vs)).astype(np.int64)  # ref data_processor.py:66-68
    return SimpleNamespace(class_names=list(cfg.CLASS_NAMES), grid_size=grid, point_cloud_range=pcr, voxel_size=list(vs),
                           point_feature_encoder=SimpleNamespace(num_point_features=num_point_features),
                           depth_downsample_factor=None)


class CenterPoint(nn.Module):
    module_topology = ["vfe", "backbone_3d", "map_to_bev_module", "backbone_2d", "dense_head"]

    def __init__(self, model_cfg, num_class, dataset):
        super().__init__()
        self.model_cfg, self.num_class, self.dataset = model_cfg, num_class, dataset
        self.class_names = dataset.class_names
        self.register_buffer("global_step", torch.LongTensor(1).zero_())
        self.module_list = self.build_networks()

    @property
    def mode(self):
        return "TRAIN" if self.training else "TEST"

    def build_networks(self):
        ds = self.dataset
        info = dict(module_list=[], num_rawpoint_features=ds.point_feature_encoder.num_point_features,
                    num_point_features=ds.point_feature_encoder.num_point_features, grid_size=ds.grid_size,
                    point_cloud_range=ds.point_cloud_range, voxel_size=ds.voxel_size)
        for name in self.module_topology:
            module = getattr(self, "build_%s" % name)(info)
            self.add_module(name, module)
            if module is not None:
                info["module_list"].append(module)
        return info["module_list"]

    def build_vfe(self, info):
        cfg = self.model_cfg.get("VFE", None)
        if cfg is None:
            return None
        m = VFE[cfg.NAME](model_cfg=cfg, num_point_features=info["num_rawpoint_features"],
                          point_cloud_range=info["point_cloud_range"], voxel_size=info["voxel_size"],
                          grid_size=info["grid_size"])
        info["num_point_features"] = m.get_output_feature_dim()
        return m

    def build_backbone_3d(self, info):
        cfg = self.model_cfg.get("BACKBONE_3D", None)
        if cfg is None:
            return None
        m = BACKBONES_3D[cfg.NAME](model_cfg=cfg, input_channels=info["num_point_features"], grid_size=info["grid_size"],
                                   voxel_size=info["voxel_size"], point_cloud_range=info["point_cloud_range"])
        info["num_point_features"] = m.num_point_features
        return m

    def build_map_to_bev_module(self, info):
        cfg = self.model_cfg.get("MAP_TO_BEV", None)
        if cfg is None:
            return None
        m = MAP_TO_BEV[cfg.NAME](model_cfg=cfg, grid_size=info["grid_size"])
        info["num_bev_features"] = m.num_bev_features
        return m

    def build_backbone_2d(self, info):
        cfg = self.model_cfg.get("BACKBONE_2D", None)
        if cfg is None:
            return None
        m = BACKBONES_2D[cfg.NAME](model_cfg=cfg, input_channels=info["num_bev_features"])
        info["num_bev_features"] = m.num_bev_features
        return m

    def build_dense_head(self, info):
        cfg = self.model_cfg.get("DENSE_HEAD", None)
        if cfg is None:
            return None
        return DENSE_HEADS[cfg.NAME](
            model_cfg=cfg, input_channels=info["num_bev_features"],
            num_class=self.num_class if not cfg.get("CLASS_AGNOSTIC", False) else 1, class_names=self.class_names,
            grid_size=info["grid_size"], point_cloud_range=info["point_cloud_range"],
            predict_boxes_when_training=bool(self.model_cfg.get("ROI_HEAD", False)), voxel_size=info["voxel_size"])

    def forward(self, batch_dict):
        for m in self.module_list:
            batch_dict = m(batch_dict)
        if self.training:  # ref centerpoint.py:13-32: ({'loss': ...}, tb_dict, disp_dict)
            loss, tb_dict = self.dense_head.get_loss()
            if getattr(self.dense_head, "fused_loss", False):  # the loss stays on the device: no host synchronisation
                return dict(loss=loss), dict(loss_rpn=loss.detach(), **tb_dict), {}
            return dict(loss=loss), dict(loss_rpn=loss.item(), **tb_dict), {}
        return self.post_processing(batch_dict)

    def post_processing(self, batch_dict):
        """(pred_dicts, recall_dict), ref centerpoint.py:36-50; recall_dict stays {} without ground truth in the batch."""
        if "final_box_dicts" not in batch_dict and "final_box_padded" in batch_dict:
            # CenterHead.padded_predictions: the head's decode ran without a host sync, the lists cost one read-back here
            batch_dict["final_box_dicts"] = unpad(batch_dict["final_box_padded"])
        final_pred_dict = batch_dict["final_box_dicts"]
        recall_dict = {}
        if "gt_boxes" not in batch_dict:
            return final_pred_dict, recall_dict
        thresh_list = self.model_cfg.POST_PROCESSING.RECALL_THRESH_LIST
        counts = [self._recall_counts(final_pred_dict[index]["pred_boxes"], index, batch_dict, thresh_list)
                  for index in range(batch_dict["batch_size"])]
        if counts:  # the samples' counters travel to the host together
            recall_dict = self._recall_add(recall_dict, torch.stack(counts).sum(0).tolist(), thresh_list)
        return final_pred_dict, recall_dict

    @staticmethod
    def generate_recall_record(box_preds, recall_dict, batch_index, data_dict=None, thresh_list=None, iou_fn=None):
        """Adds sample `batch_index` to the recall counters (ref detector3d_template.py:286-328): 'gt' ground-truth boxes
        seen, 'rcnn_<t>' / 'roi_<t>' those whose best 3-D IoU with a predicted box / a RoI exceeds t (strict).  Nothing
        happens without 'gt_boxes' in `data_dict`; 'roi_*' only count when it holds 'rois'.  `iou_fn(boxes_a, boxes_b)`
        (test hook) replaces iou3d_nms_utils.boxes_iou3d_gpu.  One read-back per call."""
        if "gt_boxes" not in data_dict:
            return recall_dict
        counts = CenterPoint._recall_counts(box_preds, batch_index, data_dict, thresh_list, iou_fn)
        return CenterPoint._recall_add(recall_dict, counts.tolist(), thresh_list)

    @staticmethod
    def _recall_add(recall_dict, counts, thresh_list):
        """`counts` [gt, rcnn per threshold, roi per threshold] (Python ints) added to the dict, its keys made on first use."""
        if len(recall_dict) == 0:
            recall_dict = {"gt": 0}
            for t in thresh_list:
                recall_dict["roi_%s" % str(t)] = 0
                recall_dict["rcnn_%s" % str(t)] = 0
        nt = len(thresh_list)
        recall_dict["gt"] += int(counts[0])
        for k, t in enumerate(thresh_list):
            recall_dict["rcnn_%s" % str(t)] += int(counts[1 + k])
            recall_dict["roi_%s" % str(t)] += int(counts[1 + nt + k])
        return recall_dict

    @staticmethod
    def _recall_counts(box_preds, batch_index, data_dict, thresh_list, iou_fn=None):
        """int64 (1 + 2 T) [gt, rcnn_t ..., roi_t ...] of one sample, on the ground truth's device, without a host sync
        (the reference reads one row sum per padded ground-truth row and one count per threshold back)."""
        iou_fn = iou_fn or iou3d_nms_utils.boxes_iou3d_gpu
        gt_boxes = data_dict["gt_boxes"][batch_index]
        rois = data_dict["rois"][batch_index] if "rois" in data_dict else None
        num_rows, nt = gt_boxes.shape[0], len(thresh_list)
        if num_rows == 0:
            return torch.zeros(1 + 2 * nt, dtype=torch.int64, device=gt_boxes.device)
        # the reference trims trailing all-zero (padding) rows with `while k > 0 and cur_gt[k].sum() == 0`: row 0 always
        # survives, so a sample whose ground truth is ALL padding counts ONE ground-truth box.  Reproduced: the number of
        # rows kept is the index of the last row with a non-zero sum (0 if there is none) + 1, as a mask over the rows
        rows = torch.arange(num_rows, device=gt_boxes.device)
        num_gt = (rows * (gt_boxes.sum(dim=1) != 0)).max() + 1
        kept = rows < num_gt

        def recalled(boxes):
            if boxes is None or boxes.shape[0] == 0:
                return torch.zeros(nt, dtype=torch.int64, device=gt_boxes.device)
            best = iou_fn(boxes[:, 0:7], gt_boxes[:, 0:7]).max(dim=0)[0]  # padded rows are zero-size boxes: IoU 0
            return torch.stack([((best > t) & kept).sum() for t in thresh_list])

        return torch.cat([num_gt.view(1), recalled(box_preds), recalled(rois)])

    # ---- checkpoints (ref detector3d_template.py:330-372) ----------------------------------------------------
    def _load_state_dict(self, model_state_disk, *, strict=True):
        state = self.state_dict()
        update = {k: v for k, v in model_state_disk.items() if k in state and state[k].shape == v.shape}
        if strict:
            self.load_state_dict(update)
        else:
            state.update(update)
            self.load_state_dict(state)
        return state, update

    def load_params_from_file(self, filename, logger=None, to_cpu=False):
        if not os.path.isfile(filename):
            raise FileNotFoundError(filename)
        loc = torch.device("cpu") if to_cpu else None
        import pickle
        try:
            # tensors / plain containers only: loading a checkpoint cannot run code.  The numpy scalar types OpenPCDet
            # stores beside the weights (epoch, it, version strings) are plain data: allowed explicitly.
            safe = []
            try:
                import numpy as np
                core = getattr(np, "_core", None) or getattr(np, "core")
                safe = [core.multiarray.scalar, np.dtype]
            except Exception:  # noqa: BLE001
                safe = []
            with (torch.serialization.safe_globals(safe) if safe and hasattr(torch.serialization, "safe_globals")
                  else contextlib.nullcontext()):
                ckpt = torch.load(filename, map_location=loc, weights_only=True)
        except pickle.UnpicklingError as err:  # a global weights_only does not allow; corrupt files / I/O errors propagate as they are
            if os.environ.get("MSSVT_TRUST_CHECKPOINTS", "0") != "1":
                raise RuntimeError(
                    "%s holds pickled objects beyond tensors (%s); unpickling them can execute arbitrary code. Set "
                    "MSSVT_TRUST_CHECKPOINTS=1 to load a checkpoint you trust." % (filename, type(err).__name__)) from err
            ckpt = torch.load(filename, map_location=loc, weights_only=False)
        state, update = self._load_state_dict(ckpt["model_state"], strict=False)
        missed = [k for k in state if k not in update]
        if logger is not None:
            for k in missed:
                logger.info("Not updated weight %s: %s" % (k, str(state[k].shape)))
            logger.info("==> Done (loaded %d/%d)" % (len(update), len(state)))
        return len(update), len(state), missed


def build_detector(cfg=None):
    """The detector of a yaml config (default: mssvt_amd/cfgs/mssvt.yaml), built as the reference's build_network does
    (pcdet/models/__init__.py:10-14, detectors/__init__.py)."""
    from . import config
    cfg = cfg if cfg is not None else config.load_yaml(config.DEFAULT_CFG)
    assert cfg.MODEL.NAME == "CenterPoint"
    return CenterPoint(cfg.MODEL, len(cfg.CLASS_NAMES), dataset_info(cfg))
