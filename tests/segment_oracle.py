"""ORACLE for instance segmentation (test infrastructure, never on the product path).

CPU restatement, in plain torch f32 ops, of the reference's segmentation pieces: Proto, the Segment head, the model builder rows that
create it, and the mask operations (crop_mask in BOTH of its branches, process_mask, process_mask_native, scale_masks).  It is
composed with the existing oracle pieces (oracle/modules.py, tests/yolo11_oracle.py).  Citations are paths relative to the
reference's ultralytics/ package.  The GPU tests compare the HIP path against this module (the reference is not available there);
tests/test_segment_oracle.py pins it to the goldens tools/gen_golden_segment.py captured from the imported reference.
"""

from __future__ import annotations

import ast
import contextlib
from copy import deepcopy

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import modules as om
from oracle import tasks as ot
from tests import yolo11_oracle as Y


class Proto(nn.Module):
    """cv3(cv2(upsample(cv1(x)))), upsample = ConvTranspose2d(c_, c_, 2, 2, 0, bias=True) (nn/modules/block.py:257-276)."""

    def __init__(self, c1, c_=256, c2=32):
        super().__init__()
        self.cv1 = om.Conv(c1, c_, k=3)
        self.upsample = nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True)
        self.cv2 = om.Conv(c_, c_, k=3)
        self.cv3 = om.Conv(c_, c2)

    def forward(self, x):
        return self.cv3(self.cv2(self.upsample(self.cv1(x))))


def _segment_class(base):
    class Segment(base):
        """Detect + Proto + cv4 mask-coefficient branches (nn/modules/head.py:790-837)."""

        def __init__(self, nc=80, nm=32, npr=256, ch=()):
            super().__init__(nc, ch)
            self.nm, self.npr = nm, npr
            self.proto = Proto(ch[0], self.npr, self.nm)
            c4 = max(ch[0] // 4, self.nm)
            self.cv4 = nn.ModuleList(nn.Sequential(om.Conv(x, c4, 3), om.Conv(c4, c4, 3), nn.Conv2d(c4, self.nm, 1)) for x in ch)

        def forward(self, x):
            p = self.proto(x[0])
            bs = p.shape[0]
            mc = torch.cat([self.cv4[i](x[i]).view(bs, self.nm, -1) for i in range(self.nl)], 2)
            x = base.forward(self, x)
            if self.training:
                return x, mc, p
            return torch.cat([x[0], mc], 1), (x[1], mc, p)

    return Segment


Segment = _segment_class(om.Detect)  # legacy class branch (v8)
Segment11 = _segment_class(Y.Detect)  # DWConv class branch (YOLO11)

_MODULES = dict(Y._MODULES)


def parse_model(d, ch):
    """tests/yolo11_oracle.py:parse_model plus the Segment row: npr = make_divisible(min(npr, max_channels) * width, 8)
    (nn/tasks.py:2987-2994)."""
    d = deepcopy(d)
    legacy = True
    max_channels = float("inf")
    nc, scales = d.get("nc"), d.get("scales")
    depth, width = d.get("depth_multiple", 1.0), d.get("width_multiple", 1.0)
    scale = d.get("scale")
    if scales:
        if not scale:
            scale = next(iter(scales.keys()))
        depth, width, max_channels = scales[scale][:3]
    ch = [ch]
    layers, save, c2 = [], [], ch[-1]
    for i, (f, n, mname, args) in enumerate(d["backbone"] + d["head"]):
        m = getattr(nn, mname[3:]) if "nn." in mname else (mname if mname in ("Detect", "Segment") else _MODULES[mname])
        args = list(args)
        for j, a in enumerate(args):
            if isinstance(a, str):
                with contextlib.suppress(ValueError):
                    args[j] = nc if a == "nc" else ast.literal_eval(a)
        n = max(round(n * depth), 1) if n > 1 else n
        if m in Y._BASE:
            c1, c2 = ch[f], args[0]
            if c2 != nc:
                c2 = ot.make_divisible(min(c2, max_channels) * width, 8)
            args = [c1, c2, *args[1:]]
            if m in Y._REPEAT:
                args.insert(2, n)
                n = 1
            if m is Y.C3k2:
                legacy = False
                if scale in "mlx":
                    args[3] = True
        elif m is om.Concat:
            c2 = sum(ch[x] for x in f)
        elif m in ("Detect", "Segment"):
            args.append([ch[x] for x in f])
            if m == "Segment":
                args[2] = ot.make_divisible(min(args[2], max_channels) * width, 8)
                m = Segment if legacy else Segment11
            else:
                m = om.Detect if legacy else Y.Detect
        else:
            c2 = ch[f]
        m_ = nn.Sequential(*(m(*args) for _ in range(n))) if n > 1 else m(*args)
        m_.np = sum(x.numel() for x in m_.parameters())
        m_.i, m_.f, m_.type = i, f, f"{m.__module__}.{m.__name__}"
        save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
        layers.append(m_)
        if i == 0:
            ch = []
        ch.append(c2)
    return nn.Sequential(*layers), sorted(save)


class SegmentationModel(ot.DetectionModel):
    """oracle/tasks.py:DetectionModel on the segmentation builder.  `cfg` is a model YAML name the product resolves
    ('yolov8n-seg.yaml') or a loaded dict."""

    def __init__(self, cfg="yolov8n-seg.yaml", ch=3, nc=None):
        nn.Module.__init__(self)
        if not isinstance(cfg, dict):
            from ultralytics_pro_amd.nn.tasks import yaml_model_load  # YAML resolution only (the builder golden pins the rows)
            cfg = yaml_model_load(cfg)
        self.yaml = cfg
        if nc and nc != self.yaml["nc"]:
            self.yaml["nc"] = nc
        self.model, self.save = parse_model(self.yaml, ch=ch)
        self.names = {i: f"{i}" for i in range(self.yaml["nc"])}
        self.inplace = True
        self.end2end = False
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
                mod.eps = 1e-3
                mod.momentum = 0.03
        self.eval()


# ---- mask operations (utils/ops.py:489-583) --------------------------------------------------------------------------------------

def crop_mask(masks, boxes, branch: str = "auto"):
    """ops.py:489-513.  branch 'auto' = the reference's choice (the rounded-integer loop for < 50 masks on the CPU, else the float
    comparisons); 'loop' / 'compare' force one.  The GPU product implements 'compare'."""
    masks = masks.clone()
    n, h, w = masks.shape
    if branch == "loop" or (branch == "auto" and n < 50 and not masks.is_cuda):
        for i, (x1, y1, x2, y2) in enumerate(boxes.round().int()):
            masks[i, :y1] = 0
            masks[i, y2:] = 0
            masks[i, :, :x1] = 0
            masks[i, :, x2:] = 0
        return masks
    x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
    r = torch.arange(w, device=masks.device, dtype=x1.dtype)[None, None, :]
    c = torch.arange(h, device=masks.device, dtype=x1.dtype)[None, :, None]
    return masks * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))


def mask_logits(protos, masks_in):
    """masks_in @ protos: (N, mh, mw) pre-crop, pre-threshold values (ops.py:532, :558)."""
    c, mh, mw = protos.shape
    return (masks_in @ protos.float().view(c, -1)).view(-1, mh, mw)


def process_mask_values(protos, masks_in, bboxes, shape, upsample=False, branch="auto"):
    """process_mask (ops.py:516-545) before `gt_(0.0)`."""
    c, mh, mw = protos.shape
    masks = mask_logits(protos, masks_in)
    ratios = torch.tensor([[mw / shape[1], mh / shape[0], mw / shape[1], mh / shape[0]]], device=bboxes.device)
    masks = crop_mask(masks, bboxes * ratios, branch)
    if upsample:
        masks = F.interpolate(masks[None], shape, mode="bilinear")[0]
    return masks


def process_mask(protos, masks_in, bboxes, shape, upsample=False, branch="auto"):
    return process_mask_values(protos, masks_in, bboxes, shape, upsample, branch).gt_(0.0).byte()


def scale_masks(masks, shape, padding=True):
    """ops.py:562-583."""
    mh, mw = masks.shape[2:]
    gain = min(mh / shape[0], mw / shape[1])
    pad_w = mw - shape[1] * gain
    pad_h = mh - shape[0] * gain
    if padding:
        pad_w /= 2
        pad_h /= 2
    top, left = (round(pad_h - 0.1), round(pad_w - 0.1)) if padding else (0, 0)
    bottom = mh - round(pad_h + 0.1)
    right = mw - round(pad_w + 0.1)
    return F.interpolate(masks[..., top:bottom, left:right], shape, mode="bilinear")


def process_mask_native_values(protos, masks_in, bboxes, shape, branch="auto"):
    """process_mask_native (ops.py:548-560) before `gt_(0.0)`."""
    masks = mask_logits(protos, masks_in)
    masks = scale_masks(masks[None], shape)[0]
    return crop_mask(masks, bboxes, branch)


def process_mask_native(protos, masks_in, bboxes, shape, branch="auto"):
    return process_mask_native_values(protos, masks_in, bboxes, shape, branch).gt_(0.0).byte()


def mask_cases():
    """(name, seed key, n masks, nm, (mh, mw), image shape (h, w), mode) of the per-op mask goldens: mode 'proto' = process_mask
    (upsample = False), 'up' = process_mask(upsample = True), 'native' = process_mask_native.  Boxes touch and cross the border."""
    return [
        ("proto_n12", "mask:a", 12, 32, (40, 48), (160, 192), "proto"),
        ("up_n12", "mask:a", 12, 32, (40, 48), (160, 192), "up"),
        ("native_n12", "mask:b", 12, 32, (40, 40), (120, 200), "native"),
        ("up_n64", "mask:c", 64, 32, (40, 40), (160, 160), "up"),
        ("native_n64", "mask:d", 64, 32, (32, 40), (90, 150), "native"),
    ]


def mask_inputs(key, n, nm, mhw, shape):
    """Procedural protos (nm, mh, mw), coefficients (n, nm) and xyxy boxes (n, 4) in image coordinates of `shape`, some of them
    touching or crossing the image border."""
    from ultralytics_pro_amd.utils import procedural as P
    mh, mw = mhw
    h, w = shape
    protos = P.uniform(f"{key}:protos", (nm, mh, mw), -1.0, 1.0)
    coef = P.uniform(f"{key}:coef", (n, nm), -1.0, 1.0)
    c = P.uniform(f"{key}:ctr", (n, 2), -0.1, 1.1) * torch.tensor([w, h], dtype=torch.float32)
    s = P.uniform(f"{key}:size", (n, 2), 0.05, 0.6) * torch.tensor([w, h], dtype=torch.float32)
    boxes = torch.cat([c - s / 2, c + s / 2], 1)
    boxes[0] = torch.tensor([0.0, 0.0, float(w), float(h)])  # the whole image
    if n > 1:
        boxes[1] = torch.tensor([-5.0, -3.0, w * 0.3, h * 0.4])  # crossing the top-left border
    return protos, coef, boxes


def mask_values(case):
    """(pre-threshold values, masks) of one mask case, crop_mask's comparison form (the GPU branch)."""
    name, key, n, nm, mhw, shape, mode = case
    protos, coef, boxes = mask_inputs(key, n, nm, mhw, shape)
    if mode == "native":
        v = process_mask_native_values(protos, coef, boxes, shape, branch="compare")
    else:
        v = process_mask_values(protos, coef, boxes, shape, upsample=mode == "up", branch="compare")
    return v, (v > 0).to(torch.uint8)
