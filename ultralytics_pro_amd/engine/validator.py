"""Validation loop of the detect, segment and pose paths on the HIP kernels, one process per GPU (reference: engine/validator.py:195-260 and
models/yolo/detect/val.py:168-288).

Per batch shard: model forward -> `non_max_suppression` with the validator's defaults (conf 0.001, iou 0.7, multi_label,
max_det 300; validator.py / val.py:108-123) -> true-positive matrices against the batch's labels (`upa_match_predictions`) -
all device side, fixed shapes, no host sync.  End of run: the per-image statistics of every rank are gathered with two
`all_gather_into_tensor` calls (RCCL; the reference pickles Python lists through `dist.gather_object`, val.py:225-240) and
every rank computes the class metrics (`ap_per_class`) on the host exactly as `DetMetrics.process` does.
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from ..parallel import dp
from ..utils import metrics as M
from ..utils.nms import nms_raw


class DetectionValidator:
    head = "Detect"  # the head type this validator takes: a head with an extra branch needs that branch's statistics next to the box ones
    _OTHER_HEADS = {"Segment": "segmentation models (Segment head) cannot be validated by {}: use SegmentationValidator (box and mask mAP)",
                    "Pose": "pose models (Pose head) cannot be validated by {}: use PoseValidator (box and pose mAP)"}

    def __init__(self, model=None, conf: float = 0.001, iou: float = 0.7, max_det: int = 300, max_gt: int = 64):
        for m in (model.modules() if model is not None else ()):
            name = type(m).__name__
            if name in self._OTHER_HEADS and name != self.head:
                raise L.UpaError(self._OTHER_HEADS[name].format(type(self).__name__))
        self.model, self.conf, self.iou, self.max_det, self.max_gt = model, conf, iou, max_det, max_gt
        self.reset()

    def reset(self):
        self._det, self._cnt, self._tp, self._gt, self._ngt = [], [], [], [], []
        self._loss, self._loss_batches = None, 0

    # ---- validation loss (training-time validate only) --------------------------------------------------------------------
    def add_loss(self, loss_items: torch.Tensor):
        """Accumulate one batch's (box, cls, dfl) loss items (validator.py:222: `self.loss += model.loss(batch, preds)[1]`)."""
        li = loss_items.detach().float()
        self._loss = li.clone() if self._loss is None else self._loss + li
        self._loss_batches += 1

    def reduce_loss(self, dst: int = 0):
        """The accumulated validation loss averaged over the ranks on rank `dst` (validator.py:241-249: `dist.reduce(loss, dst=0,
        op=AVG)`, then divided by the number of batches); every other rank gets None, as the reference returns there."""
        import torch.distributed as dist
        if self._loss is None:
            return None
        loss = dp.reduce_mean_(self._loss.clone(), dst)
        if dist.is_available() and dist.is_initialized() and dist.get_rank() != dst:
            return None
        return loss / max(self._loss_batches, 1)

    # ---- per batch ------------------------------------------------------------------------------------------------------
    def pack_labels(self, labels: dict, batch_size: int, imgsz_hw, device):
        """{"batch_idx", "cls", "bboxes" (normalised xywh)} -> padded (B, max_gt, 5) [cls, x1, y1, x2, y2] pixels + counts:
        the label preparation of DetectionValidator._prepare_batch (val.py:141-166: xywh2xyxy * imgsz)."""
        h, w = imgsz_hw
        bi = labels["batch_idx"].view(-1).long().cpu()
        cls = labels["cls"].view(-1).float().cpu()
        bb = labels["bboxes"].view(-1, 4).float().cpu() * torch.tensor([w, h, w, h], dtype=torch.float32)
        per = [(bi == j).nonzero().view(-1) for j in range(batch_size)]
        cap = max(self.max_gt, max([int(ix.numel()) for ix in per] + [1]))
        gt = torch.zeros(batch_size, cap, 5)
        ngt = torch.zeros(batch_size, dtype=torch.int32)
        for j, ix in enumerate(per):
            k = int(ix.numel())
            if k:
                xy, wh = bb[ix, :2], bb[ix, 2:] / 2
                gt[j, :k, 0] = cls[ix]
                gt[j, :k, 1:3] = xy - wh
                gt[j, :k, 3:5] = xy + wh
            ngt[j] = k
        return gt.to(device), ngt.to(device)

    def update(self, preds, gt: torch.Tensor, ngt: torch.Tensor):
        """preds: the model's eval output (y or (y, raw)); gt / ngt: padded labels of the same images (device tensors)."""
        out, counts, _ = nms_raw(preds, self.conf, self.iou, multi_label=True, max_det=self.max_det)
        self.update_detections(out, counts, gt, ngt)

    def update_detections(self, out: torch.Tensor, counts: torch.Tensor, gt: torch.Tensor, ngt: torch.Tensor):
        """Already post-processed detections (B, max_det, 6) + counts: match them and keep the batch's statistics."""
        tp = M.match_predictions_batched(out, counts, gt, ngt)
        self._det.append(out.clone())
        self._cnt.append(counts.clone())
        self._tp.append(tp)
        self._gt.append(gt[:, :, 0].clone())
        self._ngt.append(ngt.clone())

    def add_batch_stats(self, out: torch.Tensor, counts: torch.Tensor, tp: torch.Tensor, gt: torch.Tensor, ngt: torch.Tensor):
        """Statistics of a batch whose matching already ran (e.g. inside a captured step: `bench.py --workload val`)."""
        self._det.append(out.clone())
        self._cnt.append(counts.clone())
        self._tp.append(tp.clone())
        self._gt.append(gt[:, :, 0].clone())
        self._ngt.append(ngt.clone())

    # ---- end of run -----------------------------------------------------------------------------------------------------
    def local_stats(self):
        """This rank's fixed-shape statistics: (conf|cls|tp rows (I, max_det, 12) f32, counts (I,), gt classes (I, G) f32,
        n_gt (I,)) with I = images seen by this rank."""
        det = torch.cat(self._det, 0)
        tp = torch.cat(self._tp, 0).float()
        rows = torch.cat([det[:, :, 4:6], tp], 2).contiguous()
        g = max(t.shape[1] for t in self._gt)
        gcls = torch.cat([torch.nn.functional.pad(t, (0, g - t.shape[1])) for t in self._gt], 0).contiguous()
        return rows, torch.cat(self._cnt, 0).contiguous(), gcls, torch.cat(self._ngt, 0).contiguous()

    def gather_stats(self):
        """All ranks' statistics on every rank, ordered by rank (= by global image index for contiguous shards)."""
        rows, cnt, gcls, ngt = self.local_stats()
        # shards may differ in image count (uneven split) and in the padded gt width (`pack_labels` grows it to the rank's
        # largest image, COCO has images with > max_gt boxes): the ranks agree on both before anything is gathered
        rows, cnt = dp.gather_ragged(rows, cnt)
        gcls, ngt = dp.gather_ragged(gcls, ngt)
        return rows, cnt, gcls, ngt

    stat_cols = 12  # conf | cls | tp (10 IoU thresholds)

    def _gathered(self):
        """(kept statistics rows of all images of all ranks (n, stat_cols) f32, target classes (m,) f32) as numpy arrays."""
        rows, cnt, gcls, ngt = (t.cpu() for t in self.gather_stats())
        cnt, ngt = cnt.tolist(), ngt.tolist()
        sel = [rows[i, :cnt[i]] for i in range(len(cnt))]
        allr = torch.cat(sel, 0).numpy() if sel else np.zeros((0, self.stat_cols), np.float32)
        tcls = np.concatenate([gcls[i, :ngt[i]].numpy() for i in range(len(ngt))]) if ngt else np.zeros(0, np.float32)
        return allr, tcls

    @staticmethod
    def _class_metrics(tp, conf, pred_cls, tcls):
        """{p, r, f1, ap, classes, mean} of one true-positive matrix (`Metric` of DetMetrics / SegmentMetrics)."""
        if len(tp) and len(tcls):
            p, r, f1, ap, uc = M.ap_per_class(tp, conf, pred_cls, tcls)
            mp, mr, map50, map5095 = M.mean_results(p, r, ap)
        else:
            p = r = f1 = np.zeros(0)
            ap, uc = np.zeros((0, 10)), np.zeros(0, int)
            mp = mr = map50 = map5095 = 0.0
        return dict(p=p, r=r, f1=f1, ap=ap, classes=uc, mean=(mp, mr, map50, map5095))

    def get_stats(self):
        """{"tp", "conf", "pred_cls", "target_cls"} numpy arrays over all images of all ranks (val.py:212-240) and the class
        metrics `DetMetrics.process` derives from them."""
        allr, tcls = self._gathered()
        stats = dict(tp=allr[:, 2:12].astype(bool), conf=allr[:, 0], pred_cls=allr[:, 1], target_cls=tcls)
        stats.update(self._class_metrics(stats["tp"], stats["conf"], stats["pred_cls"], tcls))
        return stats


class ExtraValidator(DetectionValidator):
    """Validation of a model whose head has an extra per-anchor branch (`head`): box statistics AND a second true-positive matrix of
    what that branch predicts, under `tp_key` in the statistics and with its class metrics under `metrics_key`.  Per batch, all on the
    device with fixed shapes and no host sync: val-mode NMS -> the kept anchors' extra columns (`upa_nms_gather_extra`) -> box true
    positives (`upa_match_predictions`) -> the subclass's matching kernel.  The statistics rows are 22 wide: conf | cls | tp | tp_key."""

    stat_cols = 22
    tp_key = metrics_key = None

    def reset(self):
        super().reset()
        self._tp2 = []

    def add_batch_stats(self, out: torch.Tensor, counts: torch.Tensor, tp: torch.Tensor, gt: torch.Tensor, ngt: torch.Tensor,
                        tp2: torch.Tensor):
        """Statistics of a batch whose matching already ran (e.g. inside a captured step); `out`: (B, max_det, >= 6) rows."""
        super().add_batch_stats(out[:, :, :6], counts, tp, gt, ngt)
        self._tp2.append(tp2.clone())

    def local_stats(self):
        """As DetectionValidator.local_stats with (I, max_det, 22) rows: conf | cls | tp | tp_key."""
        rows, cnt, gcls, ngt = super().local_stats()
        return torch.cat([rows, torch.cat(self._tp2, 0).float()], 2).contiguous(), cnt, gcls, ngt

    def get_stats(self):
        """What DetectionValidator.get_stats returns for the boxes, plus `tp_key` and `metrics_key` = {p, r, f1, ap, classes, mean} of
        the second matrix: the same `ap_per_class` on its true positives, as SegmentMetrics / PoseMetrics.process do (utils/metrics.py)."""
        allr, tcls = self._gathered()
        stats = dict(tp=allr[:, 2:12].astype(bool), conf=allr[:, 0], pred_cls=allr[:, 1], target_cls=tcls)
        stats[self.tp_key] = allr[:, 12:22].astype(bool)
        stats.update(self._class_metrics(stats["tp"], stats["conf"], stats["pred_cls"], tcls))
        stats[self.metrics_key] = self._class_metrics(stats[self.tp_key], stats["conf"], stats["pred_cls"], tcls)
        return stats


class SegmentationValidator(ExtraValidator):
    """Validation of a Segment model: box AND mask P / R / mAP50 / mAP50-95 (models/yolo/segment/val.py:94-172, utils/metrics.py
    SegmentMetrics.process).  The mask true positives are `upa_segment_match`'s: the predicted masks are assembled, ANDed and popcounted
    against the packed label masks on the chip; no mask buffer exists.

    Scope: the validator's default mask path, `process_mask` at proto resolution.  `save_json` / `save_txt` (which switch the
    reference to `process_mask_native`), RLE export and plots are not provided."""

    head, tp_key, metrics_key = "Segment", "tp_m", "seg"

    def __init__(self, model=None, conf: float = 0.001, iou: float = 0.7, max_det: int = 300, max_gt: int = 64, overlap_mask: bool = True):
        self.overlap_mask = overlap_mask
        super().__init__(model, conf, iou, max_det, max_gt)

    # ---- per batch ------------------------------------------------------------------------------------------------------
    def pack_masks(self, labels: dict, batch_size: int, proto_hw, device):
        """labels["masks"] -> (bit rows (B, max_gt, words) int32, areas (B, max_gt) int32, see utils.metrics.pack_mask_bits) for the
        labels `pack_labels` packs (same order, same padded width): SegmentationValidator._prepare_batch (segment/val.py:119-143).
        With `overlap_mask` (the default) the masks are (B, h, w) index maps, instance k + 1 of an image being its label k as
        `Format` leaves them; else (n, h, w) binary planes in label order.  Masks that are not at proto resolution are resampled
        with `upa_resize_bilinear` and thresholded at > 0.5 (val.py:138-141); an index map is expanded to planes for that."""
        mh, mw = int(proto_hw[0]), int(proto_hw[1])
        bi = labels["batch_idx"].view(-1).long().cpu()
        per = [int((bi == j).sum()) for j in range(batch_size)]
        cap = max(self.max_gt, max(per + [1]))
        ngt = torch.tensor(per, dtype=torch.int32).to(device)
        masks = labels["masks"]
        if masks.dtype not in (torch.uint8, torch.bool, torch.float32, torch.int32):
            masks = masks.float()
        masks = masks.to(device)
        overlap = self.overlap_mask
        if overlap and masks.dtype == torch.bool:
            masks = masks.to(torch.uint8)
        if tuple(masks.shape[1:]) != (mh, mw):
            if overlap:  # an index map cannot be interpolated: its instances as planes first (val.py:133-134)
                planes = [masks[j][None] == torch.arange(1, k + 1, device=device).view(k, 1, 1).to(masks.dtype) for j, k in enumerate(per) if k]
                masks = torch.cat(planes, 0) if planes else masks[:0]
                overlap = False
            src = masks.float().contiguous()
            n, h, w = src.shape
            masks = torch.empty((n, mh, mw), dtype=torch.float32, device=device)
            if n:
                L.check(L.lib().upa_resize_bilinear(src.data_ptr(), n, h, w, 0, 0, h, w, masks.data_ptr(), mh, mw,
                                                    L.current_stream(device)), "resize_bilinear")
        elif not overlap and masks.dtype == torch.int32:
            masks = masks.float()
        return M.pack_mask_bits(masks, batch_size, cap, ngt, overlap=overlap)

    def update(self, preds, gt: torch.Tensor, ngt: torch.Tensor, gt_bits: torch.Tensor, gt_area: torch.Tensor, key=None,
               record: bool = True):
        """preds: the Segment model's eval output (y, (raw, mc, protos)); gt / ngt from `pack_labels`, gt_bits / gt_area from
        `pack_masks` of the same images.  `key` names the step's static buffers and `record = False` leaves the statistics to a later
        `add_batch_stats` when the call is captured into a graph.  Returns the step's device tensors (out, counts, tp, tp_m)."""
        from ..utils import ops
        y, mc, p = ops._seg_parts(preds, 0)
        out, rows, counts, _ = ops.nms_gather_extra(y, mc, (key, "segval_rows") if key is not None else None, self.conf, self.iou,
                                                    multi_label=True, max_det=self.max_det, key=key)
        return self.update_detections(out, counts, gt, ngt, rows, ops._protos_nhwc(p), gt_bits, gt_area, key=key, record=record)

    def update_detections(self, out: torch.Tensor, counts: torch.Tensor, gt: torch.Tensor, ngt: torch.Tensor, rows: torch.Tensor,
                          protos: torch.Tensor, gt_bits: torch.Tensor, gt_area: torch.Tensor, key=None, record: bool = True):
        """Already post-processed detections - out (B, max_det, 6), rows (B, max_det, 6 + nm) with the mask coefficients, counts -
        and the protos (NHWC view): match boxes and masks and keep the batch's statistics."""
        from ..engine import runtime as R
        mh, mw = int(protos.shape[2]), int(protos.shape[3])
        tp = R.alloc_plain(tuple(out.shape[:2]) + (10,), torch.uint8, out.device, key=(key, "tp")) if key is not None else None
        tp = M.match_predictions_batched(out, counts, gt, ngt, out=tp)
        # the boxes are in network-input pixels, 4 x the proto map (segment/val.py:105: imgsz = 4 * proto.shape[2:])
        tp_m = M.match_masks_batched(protos, rows, counts, (4 * mh, 4 * mw), gt, gt_bits, gt_area, ngt, key=key)
        if record:
            self.add_batch_stats(out, counts, tp, gt, ngt, tp_m)
        return out, counts, tp, tp_m


class PoseValidator(ExtraValidator):
    """Validation of a Pose model: box AND pose P / R / mAP50 / mAP50-95 (models/yolo/pose/val.py:106-197, utils/metrics.py
    PoseMetrics).  The pose true positives are `upa_pose_match`'s: OKS of every detection against the labels of its class and the
    claim step, one launch.

    Scope: `save_json` / `save_txt`, flip-index TTA and plots are not provided."""

    head, tp_key, metrics_key = "Pose", "tp_p", "pose"

    def __init__(self, model=None, conf: float = 0.001, iou: float = 0.7, max_det: int = 300, max_gt: int = 64, kpt_shape=None):
        if kpt_shape is None:
            kpt_shape = getattr(model, "kpt_shape", None) or (17, 3)
        self.kpt_shape = tuple(int(v) for v in kpt_shape)
        nkpt = self.kpt_shape[0]
        self.sigma = M.OKS_SIGMA if self.kpt_shape == (17, 3) else np.ones(nkpt) / nkpt  # pose/val.py:114-116
        super().__init__(model, conf, iou, max_det, max_gt)

    # ---- per batch ------------------------------------------------------------------------------------------------------
    def pack_keypoints(self, labels: dict, batch_size: int, device, imgsz_hw=None):
        """labels["keypoints"] (n, nkpt, 2 | 3) -> padded (B, max_gt, nkpt, 3) [x, y, visibility] for the labels `pack_labels` packs
        (same order, same padded width).  The keypoints are in network-input pixels; with `imgsz_hw` they are normalised ones and
        are multiplied by (w, h) as PoseValidator._prepare_batch does (pose/val.py:161-166).  Two-value keypoints count as visible."""
        nkpt = self.kpt_shape[0]
        bi = labels["batch_idx"].view(-1).long().cpu()
        kp = labels["keypoints"].float().cpu().reshape(-1, nkpt, labels["keypoints"].shape[-1])
        if kp.shape[-1] == 2:
            kp = torch.cat([kp, torch.ones(kp.shape[0], nkpt, 1)], 2)
        if imgsz_hw is not None:
            kp = kp * torch.tensor([float(imgsz_hw[1]), float(imgsz_hw[0]), 1.0])
        per = [(bi == j).nonzero().view(-1) for j in range(batch_size)]
        cap = max(self.max_gt, max([int(ix.numel()) for ix in per] + [1]))
        out = torch.zeros(batch_size, cap, nkpt, 3)
        for j, ix in enumerate(per):
            out[j, :int(ix.numel())] = kp[ix]
        return out.to(device)

    def update(self, preds, gt: torch.Tensor, ngt: torch.Tensor, gt_kpt: torch.Tensor, key=None, record: bool = True):
        """preds: the Pose model's eval output; gt / ngt from `pack_labels`, gt_kpt from `pack_keypoints` of the same images.  `key`
        names the step's static buffers and `record = False` leaves the statistics to a later `add_batch_stats` when the call is
        captured into a graph.  Returns the step's device tensors (rows, counts, tp, tp_p)."""
        from ..utils import ops
        rows, counts, _ = ops.pose_postprocess_raw(preds, self.conf, self.iou, max_det=self.max_det, key=key, multi_label=True)
        return self.update_detections(rows, counts, gt, ngt, gt_kpt, key=key, record=record)

    def update_detections(self, rows: torch.Tensor, counts: torch.Tensor, gt: torch.Tensor, ngt: torch.Tensor, gt_kpt: torch.Tensor,
                          key=None, record: bool = True):
        """Already post-processed detections - rows (B, max_det, 6 + nk) with the keypoints, counts: match boxes and keypoints and
        keep the batch's statistics."""
        from ..engine import runtime as R
        b, max_det, ld = rows.shape
        dev = rows.device
        out = R.alloc_plain((b, max_det, 6), torch.float32, dev, key=(key, "pose_det") if key is not None else None)
        L.check(L.lib().upa_copy_rows(rows.data_ptr(), b * max_det, 6, ld, out.data_ptr(), 6, L.current_stream(dev)), "copy_rows")
        tp = R.alloc_plain((b, max_det, 10), torch.uint8, dev, key=(key, "tp")) if key is not None else None
        tp = M.match_predictions_batched(out, counts, gt, ngt, out=tp)
        tp_p = M.match_keypoints_batched(rows, counts, gt, ngt, gt_kpt, self.kpt_shape, self.sigma, key=key)
        if record:
            self.add_batch_stats(out, counts, tp, gt, ngt, tp_p)
        return rows, counts, tp, tp_p


class ClassificationValidator:
    """Validation of a `Classify` model: top-1 / top-5 accuracy (models/yolo/classify/val.py:96-140).  Per batch the indices of the
    min(nc, 5) largest logits of every image - ranked on the device by `upa_softmax_topk` inside the head's forward, what the
    reference's `preds.argsort(1, descending=True)[:, :n5]` keeps - are copied to the host as int32 next to the targets;
    `get_stats` is `ClassifyMetrics.process` on those lists and `finalize_metrics` the confusion matrix.  One process: the
    multi-rank gather (`gather_stats`) is not provided."""

    def __init__(self, model=None):
        self.model = model
        self.metrics = M.ClassifyMetrics()
        self.names = getattr(model, "names", None)
        self.reset()

    def reset(self):
        self.pred, self.targets = [], []

    def init_metrics(self, model):
        self.names = model.names
        self.nc = len(model.names)
        self.reset()

    @staticmethod
    def postprocess(preds):
        return preds[0] if isinstance(preds, (list, tuple)) else preds

    def update_metrics(self, preds, batch):
        """preds: the model's eval output ((probs, logits) or probs) of THIS forward; batch["cls"]: the (N,) target classes."""
        probs = self.postprocess(preds)
        top = getattr(probs, "_upa_top5", None)
        if top is None:
            raise L.UpaError("ClassificationValidator: the predictions carry no device top-k (pass the Classify head's own output)")
        n5 = min(int(probs.shape[1]), 5)
        if tuple(top.shape) != (int(probs.shape[0]), n5):
            raise L.UpaError(f"ClassificationValidator: top-k of shape {tuple(top.shape)} for predictions {tuple(probs.shape)}")
        self.pred.append(top.to(torch.int32).cpu())  # a stream-ordered copy: synchronises with the forward that wrote it
        self.targets.append(torch.as_tensor(batch["cls"]).view(-1).to(torch.int32).cpu())

    def __call__(self, batches):
        """Run the model over an iterable of {"img": float NCHW in [0, 1], "cls": (N,)} batches; returns `get_stats()`."""
        if self.model is None:
            raise L.UpaError("ClassificationValidator: no model")
        self.init_metrics(self.model)
        dev = next(self.model.parameters()).device
        dt = getattr(self.model, "compute_dtype", torch.float32)
        with torch.no_grad():
            for batch in batches:
                self.update_metrics(self.model(batch["img"].to(dev).to(dt)), batch)
        self.finalize_metrics()
        return self.get_stats()

    def finalize_metrics(self):
        nc = len(self.names) if self.names is not None else int(max(int(t.max()) for t in self.pred + self.targets)) + 1
        self.metrics.confusion_matrix = M.process_cls_preds(self.pred, self.targets, nc)

    def get_stats(self):
        self.metrics.process(self.targets, self.pred)
        return self.metrics.results_dict
