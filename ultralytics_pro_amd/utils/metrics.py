"""Detection and segmentation validation metrics with the reference's function names (ultralytics/utils/metrics.py,
engine/validator.py:267-308, models/yolo/detect/val.py:274-288).

IoU and the greedy prediction-to-label matching run on the GPU for a whole batch at once (`upa_match_predictions` on the
fixed-shape NMS outputs: no per-image host round trip); what remains on the host is what the reference's `DetMetrics.process`
does on the host too - the per-class cumulative sums and the 101-point AP integration over a few thousand rows, once per
validation run (`ap_per_class` + `mean_results` reproduce P, R, mAP50, mAP50-95 bit for bit).
"""

from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L


def box_iou(box1: torch.Tensor, box2: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """(N,4), (M,4) xyxy on the GPU -> (N,M) IoU (utils/metrics.py:54-74)."""
    L.require_gpu(box1, "box_iou")
    b1, b2 = box1.float().contiguous(), box2.float().contiguous()
    out = torch.empty((b1.shape[0], b2.shape[0]), dtype=torch.float32, device=b1.device)
    if out.numel() == 0:
        return out
    L.check(L.lib().upa_box_iou(b1.data_ptr(), b1.shape[0], b2.data_ptr(), b2.shape[0], float(eps), out.data_ptr(),
                                L.current_stream(b1.device)), "box_iou")
    return out


IOUV = np.linspace(0.5, 0.95, 10).astype(np.float32)  # torch.linspace(0.5, 0.95, 10), detect/val.py:59


def match_predictions_batched(det: torch.Tensor, counts: torch.Tensor, gt: torch.Tensor, ngt: torch.Tensor, iouv=IOUV,
                              out: torch.Tensor | None = None) -> torch.Tensor:
    """True-positive matrices of a whole batch on the GPU (`upa_match_predictions`): det (B, max_det, 6) + counts (B,) as
    `nms_raw` returns them, gt (B, max_gt, 5) rows [cls, x1, y1, x2, y2] + ngt (B,) -> (B, max_det, 10) uint8, no host sync
    (engine/validator.py:267-308 through models/yolo/detect/val.py:274-288)."""
    L.require_gpu(det, "match_predictions")
    b, max_det, _ = det.shape
    thr = np.ascontiguousarray(np.asarray(iouv, dtype=np.float32))
    tp = out if out is not None else torch.empty((b, max_det, thr.shape[0]), dtype=torch.uint8, device=det.device)
    L.check(L.lib().upa_match_predictions(det.data_ptr(), counts.data_ptr(), b, max_det, gt.data_ptr(), ngt.data_ptr(),
                                          int(gt.shape[1]), thr.ctypes.data, int(thr.shape[0]), tp.data_ptr(),
                                          L.current_stream(det.device)), "match_predictions")
    return tp


def process_batch(pred_boxes: torch.Tensor, pred_cls: torch.Tensor, gt_boxes: torch.Tensor, gt_cls: torch.Tensor) -> np.ndarray:
    """True-positive matrix of one image (detect/val.py:274-288) - the single-image form of `match_predictions_batched`."""
    n, m = int(pred_cls.shape[0]), int(gt_cls.shape[0])
    if m == 0 or n == 0:
        return np.zeros((n, len(IOUV)), dtype=bool)
    dev = pred_boxes.device
    det = torch.zeros((1, n, 6), dtype=torch.float32, device=dev)
    det[0, :, :4] = pred_boxes.float()
    det[0, :, 5] = pred_cls.float()
    gt = torch.cat([gt_cls.float().view(1, m, 1), gt_boxes.float().view(1, m, 4)], 2).contiguous()
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    ng = torch.tensor([m], dtype=torch.int32, device=dev)
    return match_predictions_batched(det, cnt, gt, ng)[0].cpu().numpy().astype(bool)


# ---- mask IoU and mask true positives on bit masks (csrc/segval.hip) -------------------------------------------------------------------
# A mask of mh x mw pixels is ceil(mh * mw / 32) int32 words, bit k of word w = pixel 32 w + k.  (torch has no uint32 arithmetic worth
# the name: the rows are int32 tensors that the kernels read as uint32.)

_SRC_TYPE = {torch.uint8: L.MASK_U8, torch.bool: L.MASK_U8, torch.float32: L.MASK_F32, torch.int32: L.MASK_I32}


def mask_words(npix: int) -> int:
    return (int(npix) + 31) // 32


def pack_mask_bits(src: torch.Tensor, batch: int, max_gt: int, ngt: torch.Tensor | None = None, overlap: bool = False, key=None):
    """Ground-truth masks on the GPU -> (bits (batch, max_gt, words) int32, areas (batch, max_gt) int32) (`upa_pack_mask_bits`).
    `overlap`: src = (batch, mh, mw) index maps, label k of image b is `src[b] == k + 1` (segment/val.py:131-134; uint8, int32 or
    float32); else src = (rows, mh, mw) binary planes, bit = v > 0.5, the plane of (image b, label k) being row sum(ngt[:b]) + k
    (uint8 / bool or float32).  Rows k >= ngt[b] are zero; ngt None = max_gt labels everywhere."""
    from ..engine import runtime as R
    L.require_gpu(src, "pack_mask_bits")
    if src.dim() != 3 or src.dtype not in _SRC_TYPE or (src.dtype == torch.int32 and not overlap):
        raise L.UpaError(f"pack_mask_bits: {tuple(src.shape)} {src.dtype} masks are outside the supported forms")
    src = src.contiguous()
    mh, mw = int(src.shape[1]), int(src.shape[2])
    dev = src.device
    bits = R.alloc_plain((batch, max_gt, mask_words(mh * mw)), torch.int32, dev, key=(key, "gt_bits") if key is not None else None)
    areas = R.alloc_plain((batch, max_gt), torch.int32, dev, key=(key, "gt_area") if key is not None else None)
    if bits.numel() == 0 or mh * mw == 0:
        return bits.zero_(), areas.zero_()
    if src.shape[0] == 0:  # no plane at all: a valid (never dereferenced) address for the null check
        src = torch.zeros((1, mh, mw), dtype=src.dtype, device=dev)
    L.check(L.lib().upa_pack_mask_bits(src.data_ptr(), _SRC_TYPE[src.dtype], L.MASKS_OVERLAP if overlap else L.MASKS_PLANES,
                                       int(src.shape[0]), int(batch), int(max_gt), mh, mw, None if ngt is None else ngt.data_ptr(),
                                       bits.data_ptr(), areas.data_ptr(), L.current_stream(dev)), "pack_mask_bits")
    return bits, areas


def mask_iou(mask1: torch.Tensor, mask2: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """(N, n), (M, n) flattened 0/1 masks (float or uint8) on the GPU -> (N, M) IoU (utils/metrics.py:146-161): the rows are packed
    to bits, the intersections are popcounts (`upa_mask_iou_bits`); bit for bit the reference's float matmul form for 0/1 rows."""
    L.require_gpu(mask1, "mask_iou")
    L.require_gpu(mask2, "mask_iou")
    n, m, npix = int(mask1.shape[0]), int(mask2.shape[0]), int(mask1.shape[1])
    if int(mask2.shape[1]) != npix:
        raise L.UpaError(f"mask_iou: rows of {npix} and {int(mask2.shape[1])} pixels")
    out = torch.empty((n, m), dtype=torch.float32, device=mask1.device)
    if out.numel() == 0:
        return out
    if npix == 0:
        return out.zero_()
    prep = lambda t: (t if t.dtype in (torch.uint8, torch.bool, torch.float32) else t.float()).reshape(t.shape[0], 1, npix)  # noqa: E731
    b1, a1 = pack_mask_bits(prep(mask1), 1, n)
    b2, a2 = pack_mask_bits(prep(mask2), 1, m)
    L.check(L.lib().upa_mask_iou_bits(b1.data_ptr(), a1.data_ptr(), n, b2.data_ptr(), a2.data_ptr(), m, npix, float(eps), out.data_ptr(),
                                      L.current_stream(mask1.device)), "mask_iou")
    return out


def _cls_ld(gt: torch.Tensor) -> int:
    """Label classes as (B, max_gt) f32 or as the (B, max_gt, 5) [cls, box] rows of `match_predictions_batched`: the element stride."""
    if gt.dtype != torch.float32 or not gt.is_contiguous() or gt.dim() not in (2, 3):
        raise L.UpaError("label classes must be a contiguous float32 (B, max_gt) or (B, max_gt, 5) tensor")
    return 1 if gt.dim() == 2 else int(gt.shape[2])


def _match_workspace(b, max_det, dev, key):
    from ..engine import runtime as R
    nbytes = L.lib().upa_segment_match_workspace_bytes(int(b), int(max_det))
    return R.alloc_plain((max(nbytes // 8, 1),), torch.int64, dev, key=(key, "segmatch_ws") if key is not None else None), nbytes


def match_masks_batched(protos: torch.Tensor, rows: torch.Tensor, counts: torch.Tensor, imgsz, gt_cls: torch.Tensor,
                        gt_bits: torch.Tensor, gt_area: torch.Tensor, ngt: torch.Tensor, iouv=IOUV, out: torch.Tensor | None = None,
                        pred_bits: torch.Tensor | None = None, pred_area: torch.Tensor | None = None,
                        iou_out: torch.Tensor | None = None, key=None) -> torch.Tensor:
    """Mask true-positive matrices of a whole batch on the GPU (`upa_segment_match`; models/yolo/segment/val.py:94-117 + :145-172):
    protos - the Segment head's (B, nm, mh, mw) NHWC view, f32 or bf16 -, rows (B, max_det, 6 + nm) [box, conf, cls, coefficients] +
    counts (B,) as `nms_raw` returns them for a Segment output, imgsz = (H, W) of the network input the boxes are in, gt_cls
    (B, max_gt) f32 or the (B, max_gt, 5) label rows, gt_bits / gt_area from `pack_mask_bits`, ngt (B,) -> (B, max_det, 10) uint8, no host sync.  The predicted masks
    exist on the chip only; `pred_bits` (B, max_det, words) int32 + `pred_area` (B, max_det) int32 and `iou_out` (B, max_det, max_gt)
    f32 receive them for tests."""
    from ..engine import runtime as R
    L.require_gpu(rows, "match_masks")
    vp = R.view_of(protos)
    b, max_det, ld = rows.shape
    dev = rows.device
    thr = np.ascontiguousarray(np.asarray(iouv, dtype=np.float32))
    tp = out if out is not None else R.alloc_plain((b, max_det, thr.shape[0]), torch.uint8, dev, key=(key, "tp_m") if key is not None else None)
    ws, nbytes = _match_workspace(b, max_det, dev, key)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    L.check(L.lib().upa_segment_match(vp.ptr, vp.n, vp.h, vp.w, vp.c, vp.ld, vp.dtype, rows.data_ptr(), int(ld), int(max_det),
                                      counts.data_ptr(), float(vp.w / imgsz[1]), float(vp.h / imgsz[0]), gt_cls.data_ptr(), _cls_ld(gt_cls),
                                      gt_bits.data_ptr(), gt_area.data_ptr(), ngt.data_ptr(), int(gt_cls.shape[1]), thr.ctypes.data,
                                      int(thr.shape[0]), tp.data_ptr(), ptr(pred_bits), ptr(pred_area), ptr(iou_out), ws.data_ptr(),
                                      nbytes, L.current_stream(dev)), "segment_match")
    return tp


def match_mask_bits_batched(det_bits: torch.Tensor, det_area: torch.Tensor, det: torch.Tensor, counts: torch.Tensor, map_hw,
                            gt_cls: torch.Tensor, gt_bits: torch.Tensor, gt_area: torch.Tensor, ngt: torch.Tensor, iouv=IOUV,
                            iou_out: torch.Tensor | None = None) -> torch.Tensor:
    """`match_masks_batched` from given detection masks (`upa_segment_match_bits`): det_bits (B, max_det, words) int32 + det_area
    (B, max_det) int32 of (mh, mw) = map_hw masks, det (B, max_det, >= 6) rows with the class in column 5."""
    L.require_gpu(det, "match_mask_bits")
    b, max_det, ld = det.shape
    dev = det.device
    thr = np.ascontiguousarray(np.asarray(iouv, dtype=np.float32))
    tp = torch.empty((b, max_det, thr.shape[0]), dtype=torch.uint8, device=dev)
    ws, nbytes = _match_workspace(b, max_det, dev, None)
    L.check(L.lib().upa_segment_match_bits(det_bits.data_ptr(), det_area.data_ptr(), int(b), int(map_hw[0]), int(map_hw[1]),
                                           det.data_ptr(), int(ld), int(max_det), counts.data_ptr(), gt_cls.data_ptr(), _cls_ld(gt_cls),
                                           gt_bits.data_ptr(), gt_area.data_ptr(), ngt.data_ptr(), int(gt_cls.shape[1]), thr.ctypes.data,
                                           int(thr.shape[0]), tp.data_ptr(), None if iou_out is None else iou_out.data_ptr(),
                                           ws.data_ptr(), nbytes, L.current_stream(dev)), "segment_match_bits")
    return tp


def process_batch_masks(pred_masks: torch.Tensor, pred_cls: torch.Tensor, gt_masks: torch.Tensor, gt_cls: torch.Tensor) -> np.ndarray:
    """Mask true-positive matrix of one image (segment/val.py:165-170) - the single-image form of the batched matching: pred_masks
    (N, h, w) and gt_masks (M, h, w) binary (uint8 / bool / float32) on the GPU, classes (N,), (M,) -> (N, 10) bool."""
    n, m = int(pred_cls.shape[0]), int(gt_cls.shape[0])
    if m == 0 or n == 0:
        return np.zeros((n, len(IOUV)), dtype=bool)
    L.require_gpu(pred_masks, "process_batch_masks")
    dev = pred_masks.device
    hw = tuple(int(v) for v in pred_masks.shape[1:])
    if tuple(int(v) for v in gt_masks.shape[1:]) != hw:
        raise L.UpaError(f"process_batch_masks: predicted masks {hw} and label masks {tuple(gt_masks.shape[1:])} differ in size")
    pb, pa = pack_mask_bits(pred_masks, 1, n)
    gb, ga = pack_mask_bits(gt_masks, 1, m)
    det = torch.zeros((1, n, 6), dtype=torch.float32, device=dev)
    det[0, :, 5] = pred_cls.float()
    cnt = torch.tensor([n], dtype=torch.int32, device=dev)
    ng = torch.tensor([m], dtype=torch.int32, device=dev)
    tp = match_mask_bits_batched(pb, pa, det, cnt, hw, gt_cls.float().view(1, m).contiguous(), gb, ga, ng)
    return tp[0].cpu().numpy().astype(bool)


# ---- host-side AP arithmetic.  These three functions are a numerical RECIPE, not a design: validation mAP has to come out equal to
# the reference's to the last bit (tests/test_validator.py compares at 1e-7 against goldens produced by the imported reference), and
# that fixes the operations and their order - the box filter's edge padding, `np.interp` on the NEGATED confidences (descending x),
# the precision envelope by a reversed running maximum and the 101-point trapezoid.  They restate utils/metrics.py:612-617, 708-737
# and 740-835 (plotting, names and the per-class dict output left out); everything on the GPU side of validation (`match_predictions`,
# the statistics gather) is this repository's own.
def smooth(y: np.ndarray, f: float = 0.05) -> np.ndarray:
    """Box filter of fraction f (utils/metrics.py:612-617)."""
    nf = round(len(y) * f * 2) // 2 + 1
    pad = np.ones(nf // 2)
    return np.convolve(np.concatenate((pad * y[0], y, pad * y[-1]), 0), np.ones(nf) / nf, mode="valid")


def compute_ap(recall, precision):
    """101-point interpolated AP (utils/metrics.py:708-737)."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    return np.trapezoid(np.interp(x, mrec, mpre), x), mpre, mrec


def ap_per_class(tp, conf, pred_cls, target_cls, eps: float = 1e-16):
    """Per-class precision / recall / F1 at the max-F1 confidence and AP at the 10 IoU thresholds
    (utils/metrics.py:740-835 without plotting). Returns (p, r, f1, ap, unique_classes)."""
    order = np.argsort(-conf)
    tp, conf, pred_cls = tp[order], conf[order], pred_cls[order]
    classes, n_labels = np.unique(target_cls, return_counts=True)
    x = np.linspace(0, 1, 1000)
    ap = np.zeros((classes.shape[0], tp.shape[1]))
    p_curve, r_curve = np.zeros((classes.shape[0], 1000)), np.zeros((classes.shape[0], 1000))
    for ci, c in enumerate(classes):
        sel = pred_cls == c
        if sel.sum() == 0 or n_labels[ci] == 0:
            continue
        fpc, tpc = (1 - tp[sel]).cumsum(0), tp[sel].cumsum(0)
        recall = tpc / (n_labels[ci] + eps)
        precision = tpc / (tpc + fpc)
        r_curve[ci] = np.interp(-x, -conf[sel], recall[:, 0], left=0)
        p_curve[ci] = np.interp(-x, -conf[sel], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j] = compute_ap(recall[:, j], precision[:, j])[0]
    f1_curve = 2 * p_curve * r_curve / (p_curve + r_curve + eps)
    best = smooth(f1_curve.mean(0), 0.1).argmax()
    return p_curve[:, best], r_curve[:, best], f1_curve[:, best], ap, classes.astype(int)


def mean_results(p, r, ap):
    """(mean precision, mean recall, mAP50, mAP50-95) as `Metric.mean_results` reports them."""
    if not len(ap):
        return 0.0, 0.0, 0.0, 0.0
    return float(p.mean()), float(r.mean()), float(ap[:, 0].mean()), float(ap.mean())


# ---- classification (utils/metrics.py:1450-1501, :353-362) -----------------------------------------------------------------------------

class ClassifyMetrics:
    """top-1 / top-5 accuracy with the reference's keys.  `process(targets, pred)` takes the validator's lists: per batch the (N,) int32
    targets and the (N, min(nc, 5)) int32 indices of the largest logits, best first (host tensors; integer comparisons only)."""

    keys = ["metrics/accuracy_top1", "metrics/accuracy_top5"]

    def __init__(self) -> None:
        self.top1 = 0
        self.top5 = 0
        self.speed = {"preprocess": 0.0, "inference": 0.0, "loss": 0.0, "postprocess": 0.0}
        self.task = "classify"
        self.confusion_matrix = None

    def process(self, targets, pred):
        pred, targets = torch.cat(list(pred)), torch.cat(list(targets))
        correct = (targets[:, None] == pred).float()
        acc = torch.stack((correct[:, 0], correct.max(1).values), dim=1)  # (top1, top5) accuracy
        self.top1, self.top5 = acc.mean(0).tolist()

    @property
    def fitness(self) -> float:
        return (self.top1 + self.top5) / 2

    @property
    def results_dict(self) -> dict:
        return dict(zip([*self.keys, "fitness"], [self.top1, self.top5, self.fitness]))

    def summary(self, normalize: bool = True, decimals: int = 5):
        return [{"top1_acc": round(self.top1, decimals), "top5_acc": round(self.top5, decimals)}]


def process_cls_preds(preds, targets, nc: int) -> np.ndarray:
    """The classification confusion matrix (ConfusionMatrix.process_cls_preds, utils/metrics.py:353-362): matrix[predicted top-1,
    target] counts over all batches, (nc, nc) int64, on the host."""
    p, t = torch.cat(list(preds))[:, 0].cpu().numpy(), torch.cat(list(targets)).cpu().numpy()
    matrix = np.zeros((nc, nc), dtype=np.int64)
    np.add.at(matrix, (p, t), 1)
    return matrix


# ---- pose: object keypoint similarity and pose true positives (csrc/pose.hip) -------------------------------------------------------------
# the 17 COCO keypoint constants (utils/metrics.py:17-20)
OKS_SIGMA = np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89]) / 10.0


def match_keypoints_batched(rows: torch.Tensor, counts: torch.Tensor, gt: torch.Tensor, ngt: torch.Tensor, gt_kpt: torch.Tensor,
                            kpt_shape, sigma, iouv=IOUV, out: torch.Tensor | None = None, oks_out: torch.Tensor | None = None,
                            key=None) -> torch.Tensor:
    """Pose true-positive matrices of a whole batch on the GPU (`upa_pose_match`; models/yolo/pose/val.py:169-197): rows
    (B, max_det, 6 + nk) [box, conf, cls, keypoints] + counts (B,) as `pose_postprocess_raw` returns them, gt (B, max_gt, 5) label
    rows [cls, x1, y1, x2, y2] + ngt (B,), gt_kpt (B, max_gt, nkpt, 3) [x, y, visibility] in the same pixels -> (B, max_det, 10)
    uint8, no host sync.  `oks_out` (B, max_det, max_gt) f32 receives the OKS matrix."""
    from ..engine import runtime as R
    L.require_gpu(rows, "match_keypoints")
    b, max_det, ld = rows.shape
    nkpt, ndim = int(kpt_shape[0]), int(kpt_shape[1])
    max_gt = int(gt.shape[1])
    for t, shape, what in ((gt, (b, max_gt, 5), "gt"), (gt_kpt, (b, max_gt, nkpt, 3), "gt_kpt"), (rows, (b, max_det, ld), "rows")):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape:
            raise L.UpaError(f"match_keypoints: {what} must be a contiguous float32 {shape} tensor, got {tuple(t.shape)} {t.dtype}")
    if oks_out is not None and (oks_out.dtype != torch.float32 or not oks_out.is_contiguous() or tuple(oks_out.shape) != (b, max_det, max_gt)):
        raise L.UpaError(f"match_keypoints: oks_out must be a contiguous float32 {(b, max_det, max_gt)} tensor")
    sg = np.ascontiguousarray(np.asarray(sigma, dtype=np.float32))
    if sg.shape != (nkpt,):
        raise L.UpaError(f"match_keypoints: {sg.shape[0] if sg.ndim else 0} sigmas for {nkpt} keypoints")
    thr = np.ascontiguousarray(np.asarray(iouv, dtype=np.float32))
    tp = out if out is not None else R.alloc_plain((b, max_det, thr.shape[0]), torch.uint8, rows.device,
                                                   key=(key, "tp_p") if key is not None else None)
    L.check(L.lib().upa_pose_match(rows.data_ptr(), int(ld), int(b), int(max_det), counts.data_ptr(), gt.data_ptr(), ngt.data_ptr(), max_gt,
                                   gt_kpt.data_ptr(), nkpt, ndim, sg.ctypes.data, thr.ctypes.data, int(thr.shape[0]), tp.data_ptr(),
                                   None if oks_out is None else oks_out.data_ptr(), L.current_stream(rows.device)), "pose_match")
    return tp


def kpt_iou(kpt1: torch.Tensor, kpt2: torch.Tensor, area: torch.Tensor, sigma, eps: float = 1e-7) -> torch.Tensor:
    """Object keypoint similarity (utils/metrics.py:164-184) on the GPU: kpt1 (N, nkpt, 3) label keypoints, kpt2 (M, nkpt, 2 | 3)
    predicted ones, area (N,) label areas -> (N, M) f32.  One image of `upa_pose_match` with every pair in one class: the kernel
    derives the area from a label box, so each label gets the box (0, 0, area / 0.53, 1)."""
    L.require_gpu(kpt1, "kpt_iou")
    if eps != 1e-7:
        raise L.UpaError("kpt_iou: eps is fixed at 1e-7 on the HIP path")
    n, m, nkpt, ndim = int(kpt1.shape[0]), int(kpt2.shape[0]), int(kpt1.shape[1]), int(kpt2.shape[2])
    dev = kpt1.device
    if n == 0 or m == 0:
        return torch.zeros((n, m), dtype=torch.float32, device=dev)
    if kpt1.shape[2] != 3 or int(kpt2.shape[1]) != nkpt:
        raise L.UpaError(f"kpt_iou: label keypoints {tuple(kpt1.shape)} and predicted keypoints {tuple(kpt2.shape)}")
    rows = torch.zeros((1, m, 6 + nkpt * ndim), dtype=torch.float32, device=dev)
    rows[0, :, 6:] = kpt2.float().reshape(m, -1)
    gt = torch.zeros((1, n, 5), dtype=torch.float32, device=dev)
    gt[0, :, 3] = area.float().to(dev) / 0.53
    gt[0, :, 4] = 1.0
    cnt = torch.tensor([m], dtype=torch.int32, device=dev)
    ng = torch.tensor([n], dtype=torch.int32, device=dev)
    oks = torch.empty((1, m, n), dtype=torch.float32, device=dev)
    match_keypoints_batched(rows, cnt, gt, ng, kpt1.float().reshape(1, n, nkpt, 3).contiguous(), (nkpt, ndim), sigma, oks_out=oks)
    return oks[0].t().contiguous()
