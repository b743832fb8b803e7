"""CPU checker (test infrastructure) of the segmentation validator's mask arithmetic, in integers: `mask_iou`
(ultralytics/utils/metrics.py:146-161) and the mask half of SegmentationValidator._process_batch (models/yolo/segment/val.py:145-172).

Masks are boolean arrays.  An intersection is a count of pixels, an area is a count of pixels, every count is an integer below 2^24 -
so the f32 expression  inter / ((area1 + area2) - inter + eps)  has exactly representable operands and equals the reference's float
matmul form whatever order the matmul sums in.  The matching follows oracle/metrics.py's `match_predictions` (the reference's
non-scipy branch).  Pinned against outputs of the imported reference by tests/golden/ops_segval.npz and map_yolov8n-seg.npz.
"""

from __future__ import annotations

import numpy as np

IOUV = np.linspace(0.5, 0.95, 10).astype(np.float32)  # torch.linspace(0.5, 0.95, 10), detect/val.py:59


def words_of(npix: int) -> int:
    return (int(npix) + 31) // 32


def pack_bits(masks: np.ndarray) -> np.ndarray:
    """(..., h, w) or (..., n) boolean -> (..., ceil(n / 32)) uint32: bit k of word w = pixel 32 w + k (row-major), padding bits 0."""
    m = np.asarray(masks).astype(bool)
    flat = m.reshape(m.shape[:-2] + (m.shape[-2] * m.shape[-1],)) if m.ndim >= 3 else m
    n = flat.shape[-1]
    pad = words_of(n) * 32 - n
    flat = np.concatenate([flat, np.zeros(flat.shape[:-1] + (pad,), bool)], -1)
    by = np.ascontiguousarray(np.packbits(flat, axis=-1, bitorder="little"))
    return by.reshape(-1).view("<u4").reshape(flat.shape[:-1] + (words_of(n),))


def unpack_bits(words: np.ndarray, npix: int) -> np.ndarray:
    """(..., words) uint32 -> (..., npix) boolean."""
    w = np.ascontiguousarray(np.asarray(words).astype("<u4"))
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[:-1] + (4 * w.shape[-1],)), axis=-1, bitorder="little")[..., :npix].astype(bool)


def mask_iou(mask1: np.ndarray, mask2: np.ndarray, eps: float = 1e-7) -> np.ndarray:
    """(N, ...) and (M, ...) boolean masks -> (N, M) f32 IoU, the reference's operation order on integer counts."""
    a = np.asarray(mask1).astype(bool).reshape(len(mask1), -1)
    b = np.asarray(mask2).astype(bool).reshape(len(mask2), -1)
    inter = (a.astype(np.int64) @ b.astype(np.int64).T).astype(np.float32)
    a1, a2 = a.sum(1).astype(np.float32), b.sum(1).astype(np.float32)
    union = (a1[:, None] + a2[None]) - inter
    return (inter / (union + np.float32(eps))).astype(np.float32)


def match_predictions(pred_classes: np.ndarray, true_classes: np.ndarray, iou: np.ndarray, iouv=IOUV) -> np.ndarray:
    """(N,) predicted classes, (M,) label classes, (M, N) IoU -> (N, 10) bool (engine/validator.py:267-308; oracle/metrics.py)."""
    correct = np.zeros((pred_classes.shape[0], len(iouv)), bool)
    correct_class = np.asarray(true_classes)[:, None] == np.asarray(pred_classes)
    iou = np.asarray(iou, np.float32) * correct_class
    for i, threshold in enumerate(np.asarray(iouv, np.float32).tolist()):
        matches = np.array(np.nonzero(iou >= threshold)).T
        if matches.shape[0]:
            if matches.shape[0] > 1:
                matches = matches[iou[matches[:, 0], matches[:, 1]].argsort()[::-1]]
                matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
                matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
            correct[matches[:, 1].astype(int), i] = True
    return correct


def process_batch_masks(pred_masks: np.ndarray, pred_cls: np.ndarray, gt_masks: np.ndarray, gt_cls: np.ndarray):
    """(IoU (M, N) f32 - labels x predictions, as the reference calls mask_iou -, TP (N, 10) bool) of one image (val.py:165-170)."""
    n, m = len(pred_cls), len(gt_cls)
    if n == 0 or m == 0:
        return np.zeros((m, n), np.float32), np.zeros((n, len(IOUV)), bool)
    iou = mask_iou(gt_masks, pred_masks)
    return iou, match_predictions(np.asarray(pred_cls), np.asarray(gt_cls), iou)
