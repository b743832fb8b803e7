"""ORACLE for pose training (test infrastructure, never on the product path).

CPU restatement, in plain torch f32 ops with autograd, of v8PoseLoss (utils/loss.py:712-870: the detection terms of oracle/loss.py plus
kpts_decode, calculate_keypoints_loss and KeypointLoss, :396-412) and of one training step on tests/pose_oracle.PoseModel, stepped with
oracle.train's parameter groups, SGD-Nesterov and EMA, as tests/segment_train_oracle.py does for segmentation.
tools/gen_golden_pose_train.py pins it to the imported reference (tests/golden/train_yolov8n-pose.npz); `pose_labels` builds the
procedural keypoint labels both sides train on."""

from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import loss as ol
from oracle import train as otr
from oracle.modules import dist2bbox, make_anchors
from tests.pose_oracle import OKS_SIGMA
from ultralytics_pro_amd.utils import procedural as P

GAINS = dict(box=7.5, cls=0.5, dfl=1.5, pose=12.0, kobj=1.0)


def pose_labels(batch, seed=0, kpt_shape=(17, 3)):
    """`P.synthetic_labels(batch, seed)` as a pose batch: class 0 for every label (yolov8-pose has one class) and "keypoints"
    (n, nkpt, ndim) normalised [x, y(, visibility)].  Keypoint k of a label lies at its box centre + U(-0.65, 0.65) x the box size, so
    about a quarter of them lie outside their box (some outside the image: the reference does not clip them in the loss); visibility
    is 0, 1 or 2 (a third each, ndim 3); the LAST label of the batch has every keypoint invisible."""
    nkpt, ndim = kpt_shape
    lab = P.synthetic_labels(batch, seed=seed)
    lab["cls"] = torch.zeros_like(lab["cls"])
    bb = lab["bboxes"].numpy()
    n = bb.shape[0]
    u = P.hash_uniform(f"keypoints:{seed}:{batch}:{nkpt}", n * nkpt * 3).reshape(n, nkpt, 3)
    kp = np.zeros((n, nkpt, ndim), dtype=np.float32)
    kp[..., 0] = bb[:, None, 0] + (u[..., 0] - 0.5) * 1.3 * bb[:, None, 2]
    kp[..., 1] = bb[:, None, 1] + (u[..., 1] - 0.5) * 1.3 * bb[:, None, 3]
    if ndim == 3:
        kp[..., 2] = np.floor(u[..., 2] * 3).clip(0, 2)
        kp[-1, :, 2] = 0.0
    lab["keypoints"] = torch.from_numpy(kp)
    return lab


def keypoint_terms(fg_mask, target_gt_idx, keypoints, batch_idx, stride_tensor, target_bboxes, pred_kpts, sigmas):
    """utils/loss.py:829-870 + :404-412.  target_bboxes are in grid units; returns (kpts_loss, kpts_obj_loss) before the gains."""
    batch_idx = batch_idx.flatten()
    b = len(fg_mask)
    most = int(torch.unique(batch_idx, return_counts=True)[1].max())
    batched = torch.zeros(b, most, keypoints.shape[1], keypoints.shape[2])
    for i in range(b):
        ki = keypoints[batch_idx == i]
        batched[i, :ki.shape[0]] = ki
    idx = target_gt_idx.unsqueeze(-1).unsqueeze(-1)
    selected = batched.gather(1, idx.expand(-1, -1, keypoints.shape[1], keypoints.shape[2]))
    selected[..., :2] /= stride_tensor.view(1, -1, 1, 1)
    gt_kpt = selected[fg_mask]
    tb = target_bboxes[fg_mask]
    area = ((tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])).view(-1, 1)  # xyxy2xywh(...)[:, 2:].prod(1, keepdim=True)
    pred_kpt = pred_kpts[fg_mask]
    kpt_mask = gt_kpt[..., 2] != 0 if gt_kpt.shape[-1] == 3 else torch.full_like(gt_kpt[..., 0], True)
    d = (pred_kpt[..., 0] - gt_kpt[..., 0]).pow(2) + (pred_kpt[..., 1] - gt_kpt[..., 1]).pow(2)
    factor = kpt_mask.shape[1] / (torch.sum(kpt_mask != 0, dim=1) + 1e-9)
    e = d / ((2 * sigmas).pow(2) * (area + 1e-9) * 2)
    loc = (factor.view(-1, 1) * ((1 - torch.exp(-e)) * kpt_mask)).mean()
    obj = 0
    if pred_kpt.shape[-1] == 3:
        obj = F.binary_cross_entropy_with_logits(pred_kpt[..., 2], kpt_mask.float())
    return loc, obj


def v8_pose_loss(preds, batch, strides, kpt_shape, nc=1, reg_max=16, gains=GAINS, tal_topk=10, info=None):
    """utils/loss.py:725-789.  preds: (feats, keypoints (B, nk, A)), the train-mode Pose output.  Returns (loss (5,) * batch_size
    [box, pose, kobj, cls, dfl], detached loss items (5,)).  `info`: a dict that receives fg_mask, target_gt_idx and the assigner's
    alignment metric gaps (tools/gen_golden_pose_train.py's assertions)."""
    feats, pred_kpts = preds
    nkpt, ndim = kpt_shape
    no = nc + reg_max * 4
    b = feats[0].shape[0]
    pred_distri, pred_scores = torch.cat([xi.view(b, no, -1) for xi in feats], 2).split((reg_max * 4, nc), 1)
    pred_scores = pred_scores.permute(0, 2, 1).contiguous()
    pred_distri = pred_distri.permute(0, 2, 1).contiguous()
    pred_kpts = pred_kpts.permute(0, 2, 1).contiguous()
    dtype = pred_scores.dtype
    imgsz = torch.tensor(feats[0].shape[2:], dtype=dtype) * strides[0]
    anchor_points, stride_tensor = make_anchors(feats, strides, 0.5)
    targets = ol.preprocess_targets(batch["batch_idx"], batch["cls"], batch["bboxes"], b, imgsz[[1, 0, 1, 0]])
    gt_labels, gt_bboxes = targets.split((1, 4), 2)
    mask_gt = gt_bboxes.sum(2, keepdim=True).gt_(0.0)
    proj = torch.arange(reg_max, dtype=torch.float)
    pred_ltrb = pred_distri.view(b, -1, 4, reg_max).softmax(3).matmul(proj.type(dtype))
    pred_bboxes = dist2bbox(pred_ltrb, anchor_points, xywh=False)
    y = pred_kpts.view(b, -1, nkpt, ndim).clone()  # kpts_decode, :791-798
    y[..., :2] *= 2.0
    y[..., 0] += anchor_points[:, [0]] - 0.5
    y[..., 1] += anchor_points[:, [1]] - 0.5
    assigner = ol.TaskAlignedAssigner(topk=tal_topk, num_classes=nc, alpha=0.5, beta=6.0)
    _, target_bboxes, target_scores, fg_mask, target_gt_idx = assigner(
        pred_scores.detach().sigmoid(), (pred_bboxes.detach() * stride_tensor).type(gt_bboxes.dtype),
        anchor_points * stride_tensor, gt_labels, gt_bboxes, mask_gt)
    if info is not None:
        info.update(fg_mask=fg_mask.clone(), target_gt_idx=target_gt_idx.clone())
        if info.get("assign_only"):  # (the generator's tie check runs the assignment alone, in float64)
            return None, None
    tss = max(target_scores.sum(), 1)
    loss = torch.zeros(5)
    loss[3] = ol.slide_bce(pred_scores, target_scores.to(dtype)).sum() / tss
    if fg_mask.sum():
        tb = target_bboxes / stride_tensor
        weight = target_scores.sum(-1)[fg_mask].unsqueeze(-1)
        iou = ol.ciou_xyxy(pred_bboxes[fg_mask], tb[fg_mask])
        loss[0] = ((1.0 - iou) * weight).sum() / tss
        t_ltrb = ol.bbox2dist(anchor_points, tb, reg_max - 1)
        ld = ol.dfl_loss(pred_distri[fg_mask].view(-1, reg_max), t_ltrb[fg_mask], reg_max) * weight
        loss[4] = ld.sum() / tss
        keypoints = batch["keypoints"].float().clone()
        keypoints[..., 0] *= imgsz[1]
        keypoints[..., 1] *= imgsz[0]
        # loss.py:720-722: the COCO sigmas arrive as a float64 array, so the reference evaluates e and the term in float64
        sigmas = torch.from_numpy(OKS_SIGMA) if tuple(kpt_shape) == (17, 3) else torch.ones(nkpt) / nkpt
        loss[1], loss[2] = keypoint_terms(fg_mask, target_gt_idx, keypoints, batch["batch_idx"].view(-1, 1), stride_tensor, tb, y, sigmas)
    else:
        loss[1] += (pred_kpts * 0).sum()
    loss[0] *= gains["box"]
    loss[1] *= gains["pose"]
    loss[2] *= gains["kobj"]
    loss[3] *= gains["cls"]
    loss[4] *= gains["dfl"]
    return loss * b, loss.detach()


def train_step(model, state, batch, hyp=otr.HYP, info=None):
    """oracle.train.train_step with the pose loss: returns (loss items (5,), gradient norm before clipping); the model is updated in
    place and the clipped gradients stay on .grad."""
    model.train()
    for p in model.parameters():
        p.grad = None
    preds = model(batch["img"])
    head = model.model[-1]
    loss, items = v8_pose_loss(preds, batch, model.stride, tuple(head.kpt_shape), nc=head.nc, info=info)
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
