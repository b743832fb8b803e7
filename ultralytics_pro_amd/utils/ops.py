"""Image-space helpers either side of the hot path, reference signatures (ultralytics/utils/ops.py)."""

from __future__ import annotations

import math

import torch

from .. import _lib as L


def scale_boxes(img1_shape, boxes: torch.Tensor, img0_shape, ratio_pad=None, padding: bool = True, xywh: bool = False):
    """Rescale xyxy boxes (in place, GPU) from the letterboxed `img1_shape` (h, w) to the original `img0_shape` and clip
    (utils/ops.py:102-152 + clip_boxes :154-178).  `boxes` is (..., k>=4) float32 with the box in the first 4 columns."""
    if xywh:
        raise L.UpaError("scale_boxes(xywh=True) is outside the hot-path scope")
    L.require_gpu(boxes, "scale_boxes")
    if boxes.dtype != torch.float32 or (boxes.numel() and not boxes.is_contiguous()):
        raise L.UpaError("scale_boxes expects contiguous float32 rows")
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad_x = round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1)
        pad_y = round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1)
    else:
        gain = ratio_pad[0][0]
        pad_x, pad_y = ratio_pad[1]
    rows = boxes.numel() // boxes.shape[-1] if boxes.numel() else 0
    if rows:
        L.check(L.lib().upa_scale_boxes(boxes.data_ptr(), rows, boxes.shape[-1], float(gain), float(pad_x), float(pad_y),
                                        int(bool(padding)), float(img0_shape[1]), float(img0_shape[0]),
                                        L.current_stream(boxes.device)), "scale_boxes")
    return boxes


def make_divisible(x, divisor):
    """Nearest multiple of divisor not below x (utils/ops.py:137-150)."""
    return math.ceil(x / divisor) * divisor


# ---- instance masks (utils/ops.py:489-583, models/yolo/segment/predict.py:84-109) on `upa_process_mask` ----------------------------

def _protos_nhwc(protos: torch.Tensor) -> torch.Tensor:
    """(B, nm, mh, mw) protos as an NHWC view: Segment's own output already is one, anything else goes through the transpose kernel."""
    from ..engine import runtime as R
    if protos.dim() == 3:
        protos = protos[None]
    if R.is_nhwc_view(protos) and protos.dtype in (torch.float32, torch.bfloat16):
        return protos
    return R.to_nhwc(protos.float().contiguous(), torch.float32)


def scale_masks_window(mh: int, mw: int, shape, padding: bool = True):
    """(top, left, bottom, right) of the proto map that scale_masks resamples to `shape` (ops.py:562-583, same rounding)."""
    gain = min(mh / shape[0], mw / shape[1])
    pad_w = mw - shape[1] * gain
    pad_h = mh - shape[0] * gain
    if padding:
        pad_w /= 2
        pad_h /= 2
    top, left = (round(pad_h - 0.1), round(pad_w - 0.1)) if padding else (0, 0)
    bottom = mh - round(pad_h + 0.1)
    right = mw - round(pad_w + 0.1)
    return int(top), int(left), int(bottom), int(right)


def crop_mask(masks: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
    """masks (N, H, W) zeroed outside the xyxy boxes (N, 4) (ops.py:489-513), on `upa_crop_mask`: the float-comparison form, the
    branch the reference takes on a GPU.  Returns a new float32 tensor."""
    L.require_gpu(masks, "crop_mask")
    if boxes.device != masks.device:
        boxes = boxes.to(masks.device)
    m = masks.float().contiguous()
    b = boxes.float().contiguous()
    n, h, w = m.shape
    out = torch.empty_like(m)
    if out.numel() == 0:
        return out
    L.check(L.lib().upa_crop_mask(m.data_ptr(), n, h, w, b.data_ptr(), int(b.shape[-1]) if n else 4, out.data_ptr(),
                                  L.current_stream(m.device)), "crop_mask")
    return out


def scale_masks(masks: torch.Tensor, shape, padding: bool = True) -> torch.Tensor:
    """(N, C, H, W) masks resampled to `shape` (h, w) after removing the letterbox padding (ops.py:562-583), on `upa_resize_bilinear`
    (bilinear, align_corners = False).  Returns float32."""
    L.require_gpu(masks, "scale_masks")
    m = masks.float().contiguous()
    n, c, mh, mw = m.shape
    oh, ow = int(shape[0]), int(shape[1])
    top, left, bottom, right = scale_masks_window(int(mh), int(mw), (oh, ow), padding)
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=m.device)
    if out.numel() == 0:
        return out
    L.check(L.lib().upa_resize_bilinear(m.data_ptr(), n * c, mh, mw, top, left, bottom, right, out.data_ptr(), oh, ow,
                                        L.current_stream(m.device)), "scale_masks")
    return out


def _launch_process_mask(p, coef, coef_ld, det, det_ld, max_det, counts, out_hw, native, crop, window, masks, nonempty, capacity, total):
    from ..engine import runtime as R
    vp = R.view_of(p)
    top, left, bottom, right = window
    L.check(L.lib().upa_process_mask(vp.ptr, vp.n, vp.h, vp.w, vp.c, vp.ld, vp.dtype, coef.data_ptr(), int(coef_ld), det.data_ptr(),
                                     int(det_ld), int(max_det), counts.data_ptr(), int(out_hw[0]), int(out_hw[1]), int(bool(native)),
                                     float(crop[0]), float(crop[1]), int(top), int(left), int(bottom), int(right),
                                     None if masks is None else masks.data_ptr(), None if nonempty is None else nonempty.data_ptr(),
                                     int(capacity), total.data_ptr(), L.current_stream(p.device)), "process_mask")


def _single_image_masks(protos, masks_in, bboxes, out_hw, native, crop, window):
    L.require_gpu(masks_in, "process_mask")
    p = _protos_nhwc(protos)
    n = int(masks_in.shape[0])
    dev = masks_in.device
    masks = torch.empty((n, int(out_hw[0]), int(out_hw[1])), dtype=torch.uint8, device=dev)
    if n == 0:
        return masks
    coef = masks_in.float().contiguous()
    det = bboxes.float().contiguous()
    counts = torch.tensor([n], dtype=torch.int32, device=dev)
    nonempty = torch.empty((n,), dtype=torch.int32, device=dev)
    total = torch.empty((1,), dtype=torch.int32, device=dev)
    _launch_process_mask(p, coef, coef.shape[1], det, det.shape[1], n, counts, out_hw, native, crop, window, masks, nonempty, n, total)
    return masks


def process_mask(protos, masks_in, bboxes, shape, upsample: bool = False):
    """(N, H, W) uint8 masks (ops.py:517-545): coefficients x protos, crop_mask at proto resolution with the boxes scaled by
    (mw / W, mh / H), bilinear to `shape` when `upsample` (else the (mh, mw) proto grid), > 0.  protos: (nm, mh, mw) of one image."""
    p = protos if protos.dim() == 3 else protos[0]
    _, mh, mw = p.shape
    out = tuple(int(s) for s in shape[:2]) if upsample else (int(mh), int(mw))
    return _single_image_masks(p, masks_in, bboxes, out, False, (mw / shape[1], mh / shape[0]), (0, 0, int(mh), int(mw)))


def process_mask_native(protos, masks_in, bboxes, shape):
    """(N, H, W) uint8 masks (ops.py:548-560): coefficients x protos, scale_masks to `shape`, crop_mask with the boxes in `shape`
    coordinates, > 0."""
    p = protos if protos.dim() == 3 else protos[0]
    _, mh, mw = p.shape
    out = tuple(int(s) for s in shape[:2])
    return _single_image_masks(p, masks_in, bboxes, out, True, (1.0, 1.0), scale_masks_window(int(mh), int(mw), out))


def _extra_parts(preds, nc: int):
    """(y (B, 4+nc, A), extra (B, ne, A)) from the eval output `(y | cat([y, extra], 1), rest)` of a head with an extra per-anchor
    branch (Segment: mask coefficients, Pose: decoded keypoints), or from its first element: the parts that travel with it
    (`_upa_parts`); without them a Segment output's own mc next to y or the detection rows of the concatenated tensor, else the two
    halves of a (B, 4+nc+ne, A) tensor with nc given."""
    first, rest = (preds[0], preds[1] if len(preds) > 1 else None) if isinstance(preds, (list, tuple)) else (preds, None)
    parts = getattr(first, "_upa_parts", None)
    if parts is not None:
        return parts
    if isinstance(rest, (list, tuple)) and len(rest) == 3:  # (raw, mc, protos)
        mc = rest[1]
        nc = nc or (int(first.shape[1]) - 4 - int(mc.shape[1]))
        # (a concatenated tensor without its parts: the detection rows as a contiguous copy)
        return (first if first.shape[1] == 4 + nc else first[:, :4 + nc].contiguous()), mc
    if not nc or first.dim() != 3 or first.shape[1] <= 4 + nc:
        raise L.UpaError("pose postprocess expects a Pose head's eval output (or a (B, 4+nc+nk, A) tensor with nc given)")
    return first[:, :4 + nc].contiguous(), first[:, 4 + nc:].contiguous()


def _seg_parts(preds, nc: int):
    """(y (B, 4+nc, A), mc (B, nm, A), protos) from a Segment head's eval output `(y | cat([y, mc], 1), (raw, mc, p))`."""
    if not (isinstance(preds[1], (list, tuple)) and len(preds[1]) == 3):
        raise L.UpaError("segment postprocess expects a Segment head's eval output (y, (raw, mc, protos))")
    return _extra_parts(preds, nc)[0], preds[1][1], preds[1][2]


def nms_gather_extra(y, extra, rows_key, conf_thres, iou_thres, classes=None, agnostic=False, multi_label=False, max_det=300, key=None):
    """NMS on y (B, 4+nc, A), then the kept anchors' columns of extra (B, ne, A) behind their detections: (out (B, max_det, 6), rows
    (B, max_det, 6 + ne) under the buffer key `rows_key`, counts (B,), keep (B, max_det)), no host synchronisation."""
    from ..engine import runtime as R
    from .nms import nms_raw
    b, ne, a = extra.shape
    out, counts, keep = nms_raw(y, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, int(y.shape[1]) - 4, key=key)
    rows = R.alloc_plain((b, max_det, 6 + ne), torch.float32, y.device, key=rows_key)
    L.check(L.lib().upa_nms_gather_extra(extra.data_ptr(), b, ne, a, keep.data_ptr(), counts.data_ptr(), int(max_det), out.data_ptr(),
                                         rows.data_ptr(), 6 + ne, L.current_stream(y.device)), "nms_gather_extra")
    return out, rows, counts, keep


def segment_postprocess_raw(preds, conf_thres: float = 0.25, iou_thres: float = 0.7, classes=None, agnostic: bool = False,
                            multi_label: bool = False, max_det: int = 300, nc: int = 0, imgsz=None, orig_shape=None,
                            retina_masks: bool = False, capacity: int | None = None, key=None):
    """Device-side segmentation postprocess with no host synchronisation (capturable in `DetectionModel.compile(post=...)` and
    `PipelinedRunner`): NMS -> coefficient gather -> masks -> scale_boxes, as SegmentationPredictor.construct_result
    (models/yolo/segment/predict.py:84-109) does image by image.

    Returns a dict of device tensors: rows (B, max_det, 6 + nm) [box, conf, cls, coefficients] with the box scaled to `orig_shape`
    when given, counts (B,), masks (capacity, H, W) uint8 - the mask of (image i, detection j) is row base[i] + j, base = exclusive
    prefix sum of counts -, nonempty (capacity,) int32 (the predictor's keep filter), total (1,) int32 = sum(counts): rows past
    `capacity` are not written (the caller compares total with capacity).  (H, W) = imgsz, the network input size (default: 4x the
    proto map, which is what Proto produces from the stride-8 level), or orig_shape with `retina_masks` (process_mask_native).  One
    `orig_shape` for the whole batch."""
    from ..engine import runtime as R
    y, mc, p = _seg_parts(preds, nc)
    b, nm, _ = mc.shape
    dev = y.device
    _, rows, counts, _ = nms_gather_extra(y, mc, (key, "seg_rows"), conf_thres, iou_thres, classes, agnostic, multi_label, max_det, key)
    pv = _protos_nhwc(p)
    mh, mw = int(pv.shape[2]), int(pv.shape[3])
    ih, iw = (4 * mh, 4 * mw) if imgsz is None else (int(imgsz[0]), int(imgsz[1]))
    out_hw = (int(orig_shape[0]), int(orig_shape[1])) if (retina_masks and orig_shape is not None) else (ih, iw)
    if capacity is None:  # every row up to a 256 MB mask buffer
        capacity = max(1, min(b * max_det, (256 << 20) // (out_hw[0] * out_hw[1])))
    masks = R.alloc_plain((capacity, out_hw[0], out_hw[1]), torch.uint8, dev, key=(key, "seg_masks"))
    nonempty = R.alloc_plain((capacity,), torch.int32, dev, key=(key, "seg_nonempty"))
    total = R.alloc_plain((1,), torch.int32, dev, key=(key, "seg_total"))
    if retina_masks and orig_shape is not None:
        scale_boxes((ih, iw), rows, orig_shape)  # boxes to image space first, then masks in image coordinates
        _launch_process_mask(pv, rows[..., 6:], 6 + nm, rows, 6 + nm, max_det, counts, out_hw, True, (1.0, 1.0),
                             scale_masks_window(mh, mw, out_hw), masks, nonempty, capacity, total)
    else:
        _launch_process_mask(pv, rows[..., 6:], 6 + nm, rows, 6 + nm, max_det, counts, out_hw, False, (mw / iw, mh / ih),
                             (0, 0, mh, mw), masks, nonempty, capacity, total)
        if orig_shape is not None:
            scale_boxes((ih, iw), rows, orig_shape)
    return dict(rows=rows, counts=counts, masks=masks, nonempty=nonempty, total=total)


def segment_postprocess(preds, conf_thres: float = 0.25, iou_thres: float = 0.7, classes=None, agnostic: bool = False,
                        multi_label: bool = False, max_det: int = 300, nc: int = 0, imgsz=None, orig_shape=None,
                        retina_masks: bool = False, capacity: int | None = None):
    """Per image (boxes (n, 6) [x1, y1, x2, y2, conf, cls], masks (n, H, W) uint8 or None), mirroring
    SegmentationPredictor.construct_result: rows whose mask is empty are dropped.  Raises if the masks overflow `capacity`."""
    r = segment_postprocess_raw(preds, conf_thres, iou_thres, classes, agnostic, multi_label, max_det, nc, imgsz, orig_shape,
                                retina_masks, capacity)
    n = r["counts"].tolist()
    total = int(r["total"].item())
    cap = int(r["masks"].shape[0])
    if total > cap:
        raise L.UpaError(f"{total} masks overflow the mask buffer of {cap} rows: pass a larger capacity")
    res, base = [], 0
    for i, k in enumerate(n):
        det = r["rows"][i, :k, :6]
        if k == 0:
            res.append((det, None))
            continue
        masks = r["masks"][base:base + k]
        keep = r["nonempty"][base:base + k] > 0
        if not bool(keep.all()):
            det, masks = det[keep], masks[keep]
        res.append((det, masks))
        base += k
    return res


# ---- pose: keypoints of the kept rows (models/yolo/pose/predict.py, utils/ops.py:586-618 scale_coords) on `upa_scale_coords` ------------

def _coords_geometry(img1_shape, img0_shape, ratio_pad):
    """(gain, pad_x, pad_y) of scale_coords, host floats as `scale_boxes` computes its own.  The reference's scale_coords does NOT
    round the padding (ops.py:603-604), unlike its scale_boxes (:126-127): restated as it is."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        return gain, (img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2
    return ratio_pad[0][0], ratio_pad[1][0], ratio_pad[1][1]


def scale_coords(img1_shape, coords: torch.Tensor, img0_shape, ratio_pad=None, normalize: bool = False, padding: bool = True):
    """Rescale (..., >= 2) float32 coordinates (x, y[, visibility]) in place on the GPU from the letterboxed `img1_shape` (h, w) to
    the original `img0_shape` and clip them (utils/ops.py:586-618 + clip_coords :180-201); a third value is untouched."""
    if normalize:
        raise L.UpaError("scale_coords(normalize=True) is outside the hot-path scope")
    L.require_gpu(coords, "scale_coords")
    if coords.dtype != torch.float32 or coords.dim() < 1 or coords.shape[-1] < 2 or (coords.numel() and not coords.is_contiguous()):
        raise L.UpaError("scale_coords expects contiguous float32 (..., >= 2) coordinates")
    gain, pad_x, pad_y = _coords_geometry(img1_shape, img0_shape, ratio_pad)
    nd = int(coords.shape[-1])
    n = coords.numel() // nd
    if n:
        L.check(L.lib().upa_scale_coords(coords.data_ptr(), 1, n, nd, 0, 1, nd, None, float(gain), float(pad_x), float(pad_y),
                                         int(bool(padding)), float(img0_shape[1]), float(img0_shape[0]),
                                         L.current_stream(coords.device)), "scale_coords")
    return coords


def pose_postprocess_raw(preds, conf_thres: float = 0.25, iou_thres: float = 0.7, classes=None, agnostic: bool = False,
                         max_det: int = 300, nc: int = 0, key=None, multi_label: bool = False):
    """Device-side pose postprocess with no host synchronisation (capturable in `compile(post=...)` and `PipelinedRunner`): NMS ->
    keypoint gather (`upa_nms_gather_extra`).  Returns (rows (B, max_det, 6 + nk) [box, conf, cls, keypoints], counts (B,), keep
    (B, max_det)): in network-input pixels, rows past counts zero."""
    y, pk = _extra_parts(preds, nc)
    _, rows, counts, keep = nms_gather_extra(y, pk, (key, "pose_rows"), conf_thres, iou_thres, classes, agnostic, multi_label, max_det, key)
    return rows, counts, keep


def scale_pose_rows(rows: torch.Tensor, counts: torch.Tensor, imgsz, orig_shape, kpt_shape, ratio_pad=None, padding: bool = True):
    """scale_boxes + scale_coords in place on (B, max_det, 6 + nk) pose rows (one `orig_shape` for the batch), the first counts[i]
    rows of every image, counts read on the device."""
    b, max_det, ld = rows.shape
    scale_boxes(imgsz, rows, orig_shape, ratio_pad=ratio_pad, padding=padding)
    gain, pad_x, pad_y = _coords_geometry(imgsz, orig_shape, ratio_pad)
    L.check(L.lib().upa_scale_coords(rows.data_ptr(), int(b), int(max_det), int(ld), 6, int(kpt_shape[0]), int(kpt_shape[1]),
                                     counts.data_ptr(), float(gain), float(pad_x), float(pad_y), int(bool(padding)),
                                     float(orig_shape[1]), float(orig_shape[0]), L.current_stream(rows.device)), "scale_coords")
    return rows


def pose_postprocess(preds, conf_thres: float = 0.25, iou_thres: float = 0.7, classes=None, agnostic: bool = False, max_det: int = 300,
                     nc: int = 0, kpt_shape=(17, 3), imgsz=(640, 640), orig_shapes=None):
    """Per image (boxes (n, 6) [x1, y1, x2, y2, conf, cls], keypoints (n, nkpt, ndim)), both scaled to the image's `orig_shapes[i]`
    (h, w) when given, as PosePredictor.construct_result does (models/yolo/pose/predict.py)."""
    rows, counts, _ = pose_postprocess_raw(preds, conf_thres, iou_thres, classes, agnostic, max_det, nc)
    nkpt, ndim = int(kpt_shape[0]), int(kpt_shape[1])
    if rows.shape[2] != 6 + nkpt * ndim:
        raise L.UpaError(f"pose_postprocess: rows of {int(rows.shape[2]) - 6} keypoint values for kpt_shape {tuple(kpt_shape)}")
    n = counts.tolist()
    res = []
    for i, k in enumerate(n):
        r = rows[i, :k].contiguous()
        if orig_shapes is not None and k:
            scale_pose_rows(r[None], counts[i:i + 1], imgsz, orig_shapes[i], (nkpt, ndim))
        res.append((r[:, :6], r[:, 6:].reshape(k, nkpt, ndim)))
    return res
