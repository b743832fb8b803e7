"""Label packing on the host: the reference's batch dict -> the padded tensors the loss kernels read.  Host tensors only - this module
imports without the library."""

from __future__ import annotations

import torch

from ..._lib import UpaError

MAX_GT = 64        # initial gt-row capacity per image; grows with the data (the loss kernels take it at run time)
MAX_GT_CAP = 1024  # upa_detection_loss: LDS arrays of the assignment-resolve kernel
MASK_ID_MAX = 255  # upa_mask_loss reads the overlap mask as uint8 (the reference's dataset builds it as uint8 as well, data/utils.py)


def _pixel_boxes(labels, imgsz_h, imgsz_w):
    """(image index (n,), pixel xyxy (n, 4), keep (n,)) of a batch's labels: keep = the boxes whose xyxy coordinates do not sum to zero,
    the reference's `mask_gt` (loss.py:489).  The one statement of that rule for `pack_targets` and `pack_mask_ids`."""
    bi = labels["batch_idx"].view(-1).cpu().long()
    bb = labels["bboxes"].view(-1, 4).cpu().float()
    scale = torch.tensor([imgsz_w, imgsz_h, imgsz_w, imgsz_h], dtype=torch.float32)
    xywh = bb * scale
    xy, wh = xywh[:, :2], xywh[:, 2:] / 2
    xyxy = torch.cat([xy - wh, xy + wh], 1)
    return bi, xyxy, xyxy.sum(1) > 0


def pack_targets(labels, batch_size, imgsz_h, imgsz_w, min_rows=MAX_GT, nc=None):
    """loss.py:445-461 on the host: (n,) image index, (n,) class, (n,4) normalised xywh -> padded (B, rows, 5)
    [cls, x1, y1, x2, y2] in pixels + per-image counts (host tensors; a few hundred bytes per step).  `rows` = the largest
    per-image count rounded up to a multiple of 64 (at least `min_rows`), as the reference pads to counts.max().  Boxes
    whose xyxy coordinates sum to zero are dropped: the reference masks them (`mask_gt = gt_bboxes.sum(2) > 0`,
    loss.py:489), so they never take part in the assignment.  With `nc` given, a class id outside [0, nc) is refused here: the
    kernels index the class logits with it unchecked (the reference fails on the host with an index error)."""
    cls = labels["cls"].view(-1).cpu().float()
    bi, xyxy, keep = _pixel_boxes(labels, imgsz_h, imgsz_w)
    if nc is not None and bool(((cls < 0) | (cls >= nc)).any()):
        bad = cls[(cls < 0) | (cls >= nc)]
        raise UpaError(f"label class {float(bad[0]):g} is outside [0, {nc}) of the model's classes")
    per = [((bi == j) & keep).nonzero().view(-1) for j in range(batch_size)]
    most = max([int(ix.numel()) for ix in per] + [1])
    rows = max(min_rows, (most + 63) // 64 * 64)
    if rows > MAX_GT_CAP:
        raise UpaError(f"an image has {most} boxes; the loss kernels hold at most {MAX_GT_CAP} per image")
    gt = torch.zeros(batch_size, rows, 5)
    ngt = torch.zeros(batch_size, dtype=torch.int32)
    for j, ix in enumerate(per):
        k = int(ix.numel())
        if k:
            gt[j, :k, 0] = cls[ix]
            gt[j, :k, 1:] = xyxy[ix]
        ngt[j] = k
    return gt, ngt


def pack_mask_ids(labels, batch_size, imgsz_h, imgsz_w, rows):
    """The sibling of `pack_targets` for the overlap mask: (B, rows) int32, for every gt row `pack_targets` keeps the value that marks
    its instance in `batch["masks"]` = the label's position within its image + 1 (0 in the unused rows).  The reference keeps the boxes
    `pack_targets` drops as rows of zeros and only masks them (loss.py:445-461, :563), so its `target_gt_idx + 1` (loss.py:696) is the
    ORIGINAL position; a row index of the compacted rows would be off by the number of dropped boxes in front of it."""
    bi, _, keep = _pixel_boxes(labels, imgsz_h, imgsz_w)
    mid = torch.zeros(batch_size, rows, dtype=torch.int32)
    for j in range(batch_size):
        pos = (bi == j).nonzero().view(-1)          # the image's labels in batch order: position p <-> mask value p + 1
        kept = keep[pos].nonzero().view(-1)
        if kept.numel() > rows:
            raise UpaError(f"image {j} keeps {int(kept.numel())} boxes but the gt rows hold {rows}")
        mid[j, :kept.numel()] = (kept + 1).to(torch.int32)
    return mid


def pack_keypoints(labels, batch_size, imgsz_h, imgsz_w, rows, kpt_shape):
    """The sibling of `pack_targets` for `batch["keypoints"]`, (n, nkpt, ndim) normalised [x, y(, visibility)]: (B, rows, nkpt, 3)
    float32 [x, y, visibility] in pixels (loss.py:775-777), for every gt row `pack_targets` keeps the keypoints of that label (zeros
    in the unused rows); ndim 2 gets visibility 1 (loss.py:864).  The boxes `pack_targets` drops are dropped here by the same rule
    (`_pixel_boxes`), so a zero box in front of a label does not move its keypoints off its gt row."""
    nkpt, ndim = (int(v) for v in kpt_shape)
    kp = torch.as_tensor(labels["keypoints"]).detach().cpu().float().view(-1, nkpt, ndim)
    bi, _, keep = _pixel_boxes(labels, imgsz_h, imgsz_w)
    if kp.shape[0] != bi.numel():
        raise UpaError(f"{kp.shape[0]} keypoint rows for {bi.numel()} labels")
    out = torch.zeros(batch_size, rows, nkpt, 3)
    for j in range(batch_size):
        ix = ((bi == j) & keep).nonzero().view(-1)
        k = int(ix.numel())
        if k > rows:
            raise UpaError(f"image {j} keeps {k} boxes but the gt rows hold {rows}")
        if k:
            out[j, :k, :, 0] = kp[ix, :, 0] * imgsz_w
            out[j, :k, :, 1] = kp[ix, :, 1] * imgsz_h
            out[j, :k, :, 2] = kp[ix, :, 2] if ndim == 3 else 1.0
    return out


def pack_cls_targets(labels, batch_size, nc):
    """`batch["cls"]` of the reference's classification batch - (B,) integer class ids (models/yolo/classify/train.py
    preprocess_batch) - as a host int32 tensor.  A label outside [0, nc) is refused here (torch's cross_entropy fails on the host with
    an index error; the kernel would make the row NaN)."""
    cls = labels["cls"] if isinstance(labels, dict) else labels
    cls = torch.as_tensor(cls).detach().view(-1).cpu()
    if cls.dtype.is_floating_point or cls.dtype == torch.bool:
        raise UpaError(f"classification labels must be integer class ids, got {cls.dtype}")
    if cls.numel() != batch_size:
        raise UpaError(f"{cls.numel()} labels for a batch of {batch_size} images")
    cls = cls.long()
    bad = (cls < 0) | (cls >= nc)
    if bool(bad.any()):
        raise UpaError(f"label class {int(cls[bad][0])} is outside [0, {nc}) of the model's classes")
    return cls.to(torch.int32)
