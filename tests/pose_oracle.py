"""ORACLE for pose estimation (test infrastructure, never on the product path).

CPU restatement, in plain torch f32 ops, of the reference's pose pieces: the Pose head with `kpts_decode`, the model builder row that
creates it, `scale_coords`, `kpt_iou` and the pose half of PoseValidator._process_batch - plus a float64 `kpt_iou`.  It is composed with
the existing oracle pieces (oracle/modules.py, tests/yolo11_oracle.py, tests/segment_oracle.py's builder).  Citations are paths relative to
the reference's ultralytics/ package.  The GPU tests compare the HIP path against this module (the reference is not available there);
tests/test_pose_oracle.py pins it to the goldens tools/gen_golden_pose.py captured from the imported reference.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn

from oracle import modules as om
from oracle import tasks as ot
from tests import segment_oracle as S
from tests import yolo11_oracle as Y

OKS_SIGMA = np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89, 0.89]) / 10.0
IOUV = torch.linspace(0.5, 0.95, 10)


def kpts_decode(kpts: torch.Tensor, anchors: torch.Tensor, strides: torch.Tensor, ndim: int) -> torch.Tensor:
    """nn/modules/head.py:1264-1273: kpts (B, nk, A), anchors (2, A) cell centres, strides (1, A)."""
    y = kpts.clone()
    if ndim == 3:
        y[:, 2::ndim] = y[:, 2::ndim].sigmoid()
    y[:, 0::ndim] = (y[:, 0::ndim] * 2.0 + (anchors[0] - 0.5)) * strides
    y[:, 1::ndim] = (y[:, 1::ndim] * 2.0 + (anchors[1] - 0.5)) * strides
    return y


def _pose_class(base):
    class Pose(base):
        """Detect + cv4 keypoint branches (nn/modules/head.py:1208-1273)."""

        def __init__(self, nc=80, kpt_shape=(17, 3), ch=()):
            super().__init__(nc, ch)
            self.kpt_shape = kpt_shape
            self.nk = kpt_shape[0] * kpt_shape[1]
            c4 = max(ch[0] // 4, self.nk)
            self.cv4 = nn.ModuleList(nn.Sequential(om.Conv(x, c4, 3), om.Conv(c4, c4, 3), nn.Conv2d(c4, self.nk, 1)) for x in ch)

        def forward(self, x):
            bs = x[0].shape[0]
            kpt = torch.cat([self.cv4[i](x[i]).view(bs, self.nk, -1) for i in range(self.nl)], -1)
            x = base.forward(self, x)
            if self.training:
                return x, kpt
            anchors, strides = (t.transpose(0, 1) for t in om.make_anchors(x[1], self.stride, 0.5))
            return torch.cat([x[0], kpts_decode(kpt, anchors, strides, self.kpt_shape[1])], 1), (x[1], kpt)

    return Pose


Pose = _pose_class(om.Detect)  # legacy class branch (v8)
Pose11 = _pose_class(Y.Detect)  # DWConv class branch (YOLO11)


def parse_model(d, ch):
    """tests/segment_oracle.py:parse_model with the Pose row `[nc, kpt_shape]` (nn/tasks.py: `kpt_shape` is resolved from the YAML)."""
    import copy
    d = copy.deepcopy(d)
    rows = d["backbone"] + d["head"]
    assert rows[-1][2] == "Pose", rows[-1]
    f, n, _, args = rows[-1]
    rows[-1] = [f, n, "Detect", ["nc"]]  # build the graph with a Detect tail, then swap the head in
    d["head"] = rows[len(d["backbone"]):]
    model, save = S.parse_model(d, ch)
    det = model[-1]
    chans = [c[0].conv.in_channels for c in det.cv2]
    legacy = isinstance(det, om.Detect) and not isinstance(det, Y.Detect)
    head = (Pose if legacy else Pose11)(d["nc"], tuple(d["kpt_shape"]), chans)
    head.np = sum(x.numel() for x in head.parameters())
    head.i, head.f, head.type = det.i, det.f, f"{type(head).__module__}.Pose"
    layers = list(model.children())[:-1] + [head]
    return nn.Sequential(*layers), save


class PoseModel(S.SegmentationModel):
    """tests/segment_oracle.py's model class on the pose builder.  `cfg`: a YAML name the product resolves, or a loaded dict."""

    def __init__(self, cfg="yolov8n-pose.yaml", ch=3, nc=None):
        nn.Module.__init__(self)
        if not isinstance(cfg, dict):
            from ultralytics_pro_amd.nn.tasks import yaml_model_load  # YAML resolution only (the builder golden pins the rows)
            cfg = yaml_model_load(cfg)
        self.yaml = cfg
        if nc and nc != self.yaml["nc"]:
            self.yaml["nc"] = nc
        self.model, self.save = parse_model(self.yaml, ch=ch)
        self.names = {i: f"{i}" for i in range(self.yaml["nc"])}
        self.inplace, self.end2end = True, False
        m = self.model[-1]
        s = 256  # nn/tasks.py:1315-1331
        self.eval()
        m.training = True
        with torch.no_grad():
            outs = self._predict_once(torch.zeros(1, ch, s, s))[0]
        m.stride = torch.tensor([s / x.shape[-2] for x in outs])
        self.stride = m.stride
        m.bias_init()
        for mod in self.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.eps, mod.momentum = 1e-3, 0.03
        self.eval()


# ---- scale_coords (utils/ops.py:586-618, clip_coords :180-201) -----------------------------------------------------------------------

def scale_coords(img1_shape, coords, img0_shape, ratio_pad=None, normalize=False, padding=True):
    coords = coords.clone()
    h0, w0 = img0_shape[:2]
    if ratio_pad is None:
        gain = min(img1_shape[0] / h0, img1_shape[1] / w0)
        pad = (img1_shape[1] - w0 * gain) / 2, (img1_shape[0] - h0 * gain) / 2
    else:
        gain, pad = ratio_pad[0][0], ratio_pad[1]
    if padding:
        coords[..., 0] -= pad[0]
        coords[..., 1] -= pad[1]
    coords[..., 0] /= gain
    coords[..., 1] /= gain
    coords[..., 0].clamp_(0, w0)
    coords[..., 1].clamp_(0, h0)
    if normalize:
        coords[..., 0] /= w0
        coords[..., 1] /= h0
    return coords


# ---- OKS and the pose true positives (utils/metrics.py:164-184, models/yolo/pose/val.py:169-197) -----------------------------------------

def kpt_iou(kpt1, kpt2, area, sigma, eps=1e-7):
    """(N, nkpt, 3) label keypoints, (M, nkpt, 2 | 3) predictions, (N,) areas -> (N, M), in the dtype of kpt1 (f32 or f64)."""
    d = (kpt1[:, None, :, 0] - kpt2[..., 0]).pow(2) + (kpt1[:, None, :, 1] - kpt2[..., 1]).pow(2)
    sigma = torch.as_tensor(np.asarray(sigma), dtype=kpt1.dtype)
    kpt_mask = kpt1[..., 2] != 0
    e = d / ((2 * sigma).pow(2) * (area[:, None, None] + eps) * 2)
    return ((-e).exp() * kpt_mask[:, None]).sum(-1) / (kpt_mask.sum(-1)[:, None] + eps)


def kpt_iou_f64(kpt1, kpt2, area, sigma, eps=1e-7):
    """The same from the f32 INPUTS (the f32 area included) in float64: the exact value the f32 forms approximate."""
    return kpt_iou(kpt1.double(), kpt2.double(), area.double(), np.asarray(sigma, dtype=np.float32).astype(np.float64), eps)


def label_area(gt_boxes):
    """ops.xyxy2xywh(bboxes)[:, 2:].prod(1) * 0.53 (pose/val.py:193)."""
    return ((gt_boxes[:, 2] - gt_boxes[:, 0]) * (gt_boxes[:, 3] - gt_boxes[:, 1])) * 0.53


def match_predictions(pred_cls, true_cls, iou, iouv=IOUV):
    """engine/validator.py:267-308, the non-scipy branch: iou (labels, predictions) -> (predictions, 10) bool."""
    correct = np.zeros((pred_cls.shape[0], iouv.shape[0])).astype(bool)
    correct_class = true_cls[:, None] == pred_cls
    iou = (iou * correct_class).cpu().numpy()
    for i, threshold in enumerate(iouv.cpu().tolist()):
        matches = np.array(np.nonzero(iou >= threshold)).T
        if matches.shape[0]:
            if matches.shape[0] > 1:
                matches = matches[iou[matches[:, 0], matches[:, 1]].argsort()[::-1]]
                matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
                matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
            correct[matches[:, 1].astype(int), i] = True
    return correct


def process_batch_pose(pred_kpts, pred_cls, gt_boxes, gt_cls, gt_kpts, sigma):
    """pose/val.py:187-196: (OKS (labels, predictions) f32, tp_p (predictions, 10) bool)."""
    n, m = int(pred_cls.shape[0]), int(gt_cls.shape[0])
    if n == 0 or m == 0:
        return torch.zeros((m, n)), np.zeros((n, 10), dtype=bool)
    iou = kpt_iou(gt_kpts, pred_kpts, label_area(gt_boxes), sigma)
    return iou, match_predictions(pred_cls, gt_cls, iou)


def no_tie_violations(oks, pred_cls, gt_cls, tol=1e-5):
    """The number of (detection, label) pairs that break the goldens' no-tie condition: a same-class OKS within `tol` of a threshold,
    or a detection with two same-class labels whose OKS differ by less than `tol` (both above 0: a pair of zeros decides nothing)."""
    oks = np.asarray(oks, dtype=np.float64)
    same = np.asarray(gt_cls)[:, None] == np.asarray(pred_cls)[None]
    bad = int((same[:, :, None] & (np.abs(oks[:, :, None] - IOUV.numpy().astype(np.float64)[None, None]) <= tol)).sum())
    for j in range(oks.shape[1]):
        v = np.sort(oks[:, j][same[:, j] & (oks[:, j] >= 0.5 - tol)])
        bad += int((np.diff(v) < tol).sum())
    return bad


# ---- the bf16 emulation's distance from the f32 golden (the GPU keypoint gate, tests/pose_cases.py:BF16_KPT_EMUL) ----------------------

def kpt_split(d, nc):
    """|d| of the sampled head rows -> (box, score, keypoint x / y, visibility) maxima."""
    k = d[:, 4 + nc:]
    xy = [j for j in range(51) if j % 3 != 2]
    return float(d[:, :4].max()), float(d[:, 4:4 + nc].max()), float(k[:, xy].max()), float(k[:, 2::3].max())


def emulated_kpt_distance(name, golden_dir):
    """CPU: the distance of oracle/bf16_emul.py's emulation of the smooth-family pose model from the reference's f32 golden over the
    sampled rows -> (box, score, keypoint x / y, visibility) maxima."""
    from oracle.bf16_emul import emulate_bf16
    from ultralytics_pro_amd.utils import procedural as P
    g = np.load(golden_dir / f"e2e_{name}_smooth.npz")
    o = PoseModel(name + ".yaml")
    P.apply_procedural_weights(o, family=f"smooth:{name}")
    o.fuse()
    e = emulate_bf16(o)
    with torch.no_grad():
        y = e(P.synthetic_images(2).to(torch.bfloat16).float())[0]
    d = np.abs(y[:, :, g["anchor_sel"]].numpy() - g["y_sel"])
    return kpt_split(d, int(g["nc"]))
