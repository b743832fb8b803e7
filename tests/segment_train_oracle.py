"""ORACLE for segmentation training (test infrastructure, never on the product path).

CPU restatement, in plain torch f32 ops with autograd, of v8SegmentationLoss (utils/loss.py:531-709: the detection terms of
oracle/loss.py plus calculate_segmentation_loss / single_mask_loss with crop_mask's COMPARISON branch, utils/ops.py:510-513 - the
branch a GPU run of the reference takes) and of one training step on tests/segment_oracle.SegmentationModel, stepped with
oracle.train's parameter groups, SGD-Nesterov and EMA.  tools/gen_golden_segment_train.py pins it to the imported reference
(tests/golden/train_yolov8n-seg.npz); `overlap_masks` builds the procedural overlap masks both sides train on.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import loss as ol
from oracle import train as otr
from oracle.modules import dist2bbox, make_anchors

GAINS = dict(box=7.5, cls=0.5, dfl=1.5)


def overlap_masks(labels, batch_size, mh, mw):
    """(B, mh, mw) uint8 overlap mask from the labels alone: instance p of an image (its p-th label in batch order) is an ellipse (even
    p) or a diamond (odd p) inscribed in its box, painted as p + 1, later instances over earlier ones."""
    bi = labels["batch_idx"].view(-1).long()
    bb = labels["bboxes"].view(-1, 4).float()
    ys = (torch.arange(mh, dtype=torch.float32) + 0.5).view(-1, 1) / mh
    xs = (torch.arange(mw, dtype=torch.float32) + 0.5).view(1, -1) / mw
    out = torch.zeros(batch_size, mh, mw, dtype=torch.uint8)
    for j in range(batch_size):
        for p, i in enumerate((bi == j).nonzero().view(-1).tolist()):
            cx, cy, w, h = (float(v) for v in bb[i])
            if w <= 0 or h <= 0:
                continue
            dx, dy = (xs - cx).abs() / (w / 2), (ys - cy).abs() / (h / 2)
            inside = (dx * dx + dy * dy <= 1.0) if p % 2 == 0 else (dx + dy <= 1.0)
            out[j][inside] = p + 1
    return out


def crop_mask_compare(masks, boxes):
    """utils/ops.py:510-513."""
    _, h, w = masks.shape
    x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
    r = torch.arange(w, dtype=x1.dtype)[None, None, :]
    c = torch.arange(h, dtype=x1.dtype)[None, :, None]
    return masks * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))


def mask_term(fg_mask, masks, target_gt_idx, target_bboxes, proto, pred_masks, imgsz):
    """utils/loss.py:646-709 with overlap = True."""
    _, _, mh, mw = proto.shape
    tbn = target_bboxes / imgsz[[1, 0, 1, 0]]
    marea = (tbn[..., 2] - tbn[..., 0]) * (tbn[..., 3] - tbn[..., 1])
    mxyxy = tbn * torch.tensor([mw, mh, mw, mh], dtype=tbn.dtype)
    loss = 0
    for i in range(proto.shape[0]):
        fg = fg_mask[i]
        if fg.any():
            gt_mask = (masks[i] == (target_gt_idx[i][fg] + 1).view(-1, 1, 1)).float()
            pred = torch.einsum("in,nhw->ihw", pred_masks[i][fg], proto[i])
            bce = F.binary_cross_entropy_with_logits(pred, gt_mask, reduction="none")
            loss = loss + (crop_mask_compare(bce, mxyxy[i][fg]).mean(dim=(1, 2)) / marea[i][fg]).sum()
        else:
            loss = loss + (proto * 0).sum() + (pred_masks * 0).sum()
    return loss / fg_mask.sum()


def v8_segmentation_loss(preds, batch, strides, nc=80, reg_max=16, gains=GAINS, tal_topk=10):
    """utils/loss.py:539-620.  preds: (feats, mask coefficients (B, nm, A), proto (B, nm, mh, mw)), the train-mode Segment output.
    Returns (loss (4,) * batch_size [box, seg, cls, dfl], detached loss items (4,))."""
    feats, pred_masks, proto = preds
    no = nc + reg_max * 4
    b = feats[0].shape[0]
    mh, mw = proto.shape[-2:]
    pred_distri, pred_scores = torch.cat([xi.view(b, no, -1) for xi in feats], 2).split((reg_max * 4, nc), 1)
    pred_scores = pred_scores.permute(0, 2, 1).contiguous()
    pred_distri = pred_distri.permute(0, 2, 1).contiguous()
    pred_masks = pred_masks.permute(0, 2, 1).contiguous()
    dtype = pred_scores.dtype
    imgsz = torch.tensor(feats[0].shape[2:], dtype=dtype) * strides[0]
    anchor_points, stride_tensor = make_anchors(feats, strides, 0.5)
    targets = ol.preprocess_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], b, imgsz[[1, 0, 1, 0]])
    gt_labels, gt_bboxes = targets.split((1, 4), 2)
    mask_gt = gt_bboxes.sum(2, keepdim=True).gt_(0.0)
    proj = torch.arange(reg_max, dtype=torch.float)
    pred_ltrb = pred_distri.view(b, -1, 4, reg_max).softmax(3).matmul(proj.type(dtype))
    pred_bboxes = dist2bbox(pred_ltrb, anchor_points, xywh=False)
    assigner = ol.TaskAlignedAssigner(topk=tal_topk, num_classes=nc, alpha=0.5, beta=6.0)
    _, target_bboxes, target_scores, fg_mask, target_gt_idx = assigner(
        pred_scores.detach().sigmoid(), (pred_bboxes.detach() * stride_tensor).type(gt_bboxes.dtype),
        anchor_points * stride_tensor, gt_labels, gt_bboxes, mask_gt)
    tss = max(target_scores.sum(), 1)
    loss = torch.zeros(4)
    loss[2] = ol.slide_bce(pred_scores, target_scores.to(dtype)).sum() / tss
    if fg_mask.sum():
        tb = target_bboxes / stride_tensor
        weight = target_scores.sum(-1)[fg_mask].unsqueeze(-1)
        iou = ol.ciou_xyxy(pred_bboxes[fg_mask], tb[fg_mask])
        loss[0] = ((1.0 - iou) * weight).sum() / tss
        t_ltrb = ol.bbox2dist(anchor_points, tb, reg_max - 1)
        ld = ol.dfl_loss(pred_distri[fg_mask].view(-1, reg_max), t_ltrb[fg_mask], reg_max) * weight
        loss[3] = ld.sum() / tss
        masks = batch["masks"].float()
        assert tuple(masks.shape[-2:]) == (mh, mw), "masks must come at prototype resolution"
        loss[1] = mask_term(fg_mask, masks, target_gt_idx, target_bboxes, proto, pred_masks, imgsz)
    else:
        loss[1] += (proto * 0).sum() + (pred_masks * 0).sum()
    loss[0] *= gains["box"]
    loss[1] *= gains["box"]
    loss[2] *= gains["cls"]
    loss[3] *= gains["dfl"]
    return loss * b, loss.detach()


def train_step(model, state, batch, hyp=otr.HYP):
    """oracle.train.train_step with the segmentation loss: returns (loss items (4,), gradient norm before clipping); the model is
    updated in place and the clipped gradients stay on .grad."""
    model.train()
    for p in model.parameters():
        p.grad = None
    preds = model(batch["img"])
    loss, items = v8_segmentation_loss(preds, batch, model.stride, nc=model.model[-1].nc)
    loss.sum().backward()
    params = [p for p in model.parameters() if p.grad is not None]
    total_norm = torch.nn.utils.clip_grad_norm_(params, max_norm=hyp["max_norm"])
    g0, g1, g2 = otr.param_groups(model)
    mom = hyp["momentum"]
    with torch.no_grad():
        for group, wd in ((g2, 0.0), (g0, hyp["weight_decay"]), (g1, 0.0)):
            for name, p in group:
                if p.grad is None:
                    continue
                g = p.grad
                if wd:
                    g = g.add(p, alpha=wd)
                buf = state.momentum.get(name)
                if buf is None:
                    buf = state.momentum[name] = g.clone()
                else:
                    buf.mul_(mom).add_(g)
                p.add_(g.add(buf, alpha=mom), alpha=-hyp["lr"])
        state.updates += 1
        d = hyp["ema_decay"] * (1 - math.exp(-state.updates / hyp["ema_tau"]))
        msd = model.state_dict()
        for k, v in state.ema.items():
            if v.dtype.is_floating_point:
                v.mul_(d)
                v.add_((1 - d) * msd[k].detach())
    return items, float(total_norm)
