"""ORACLE for image classification (test infrastructure, never on the product path).

CPU restatement, in plain torch f32 ops, of the reference's `Classify` head and `ClassificationModel`, composed with the existing
oracle pieces (oracle/modules.py, tests/yolo11_oracle.py) the way tests/segment_oracle.py is.  Citations are paths relative to the
reference's ultralytics/ package.  The GPU tests compare the HIP path against this module (the reference is not available there);
tests/test_classify_oracle.py pins it to the goldens tools/gen_golden_classify.py captured from the imported reference.
"""

from __future__ import annotations

import ast
import contextlib
from copy import deepcopy

import torch
import torch.nn as nn

from oracle import modules as om
from oracle import tasks as ot
from tests import yolo11_oracle as Y


class Classify(nn.Module):
    """Conv(c1, 1280, k, s, p, g) -> AdaptiveAvgPool2d(1) -> Dropout(0) -> Linear(1280, c2); eval returns (softmax, logits)
    (nn/modules/head.py:1481-1531)."""

    export = False

    def __init__(self, c1, c2, k=1, s=1, p=None, g=1):
        super().__init__()
        c_ = 1280
        self.conv = om.Conv(c1, c_, k, s, p, g)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.drop = nn.Dropout(p=0.0, inplace=True)
        self.linear = nn.Linear(c_, c2)

    def forward(self, x):
        if isinstance(x, list):
            x = torch.cat(x, 1)
        x = self.linear(self.drop(self.pool(self.conv(x)).flatten(1)))
        if self.training:
            return x
        y = x.softmax(1)
        return y if self.export else (y, x)


_MODULES = dict(Y._MODULES, Classify=Classify)
_BASE = set(Y._BASE) | {Classify}  # Classify is one of the reference's base_modules (nn/tasks.py:2446-2448)


def parse_model(d, ch):
    """tests/yolo11_oracle.py:parse_model for backbone rows plus the Classify row: args [nc] -> [c1, nc] (nn/tasks.py:2848-2851)."""
    d = deepcopy(d)
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
        m = getattr(nn, mname[3:]) if "nn." in mname else _MODULES[mname]
        args = list(args)
        for j, a in enumerate(args):
            if isinstance(a, str):
                with contextlib.suppress(ValueError):
                    args[j] = nc if a == "nc" else ast.literal_eval(a)
        n = max(round(n * depth), 1) if n > 1 else n
        if m in _BASE:
            c1, c2 = ch[f], args[0]
            if c2 != nc:
                c2 = ot.make_divisible(min(c2, max_channels) * width, 8)
            args = [c1, c2, *args[1:]]
            if m in Y._REPEAT:
                args.insert(2, n)
                n = 1
            if m is Y.C3k2 and scale in "mlx":
                args[3] = True
        elif m is om.Concat:
            c2 = sum(ch[x] for x in f)
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


class ClassificationModel(ot.DetectionModel):
    """nn/tasks.py:1516-1605 on the builder above: stride [1], names, the nc override.  BatchNorm keeps torch's defaults (the
    reference's `_from_yaml` does not run `initialize_weights`).  `cfg` is a model YAML name the product resolves or a loaded dict;
    forward, `_predict_once` and `fuse` are oracle/tasks.py's."""

    def __init__(self, cfg="yolov8n-cls.yaml", ch=3, nc=None):
        nn.Module.__init__(self)
        if not isinstance(cfg, dict):
            from ultralytics_pro_amd.nn.tasks import yaml_model_load  # YAML resolution only (the builder golden pins the rows)
            cfg = yaml_model_load(cfg)
        self.yaml = cfg
        ch = self.yaml["channels"] = self.yaml.get("channels", ch)
        if nc and nc != self.yaml["nc"]:
            self.yaml["nc"] = nc
        self.model, self.save = parse_model(self.yaml, ch=ch)
        self.stride = torch.Tensor([1])
        self.names = {i: f"{i}" for i in range(self.yaml["nc"])}
        self.eval()

    @staticmethod
    def reshape_outputs(model, nc):
        m = list(model.model.children())[-1]
        if m.linear.out_features != nc:
            m.linear = nn.Linear(m.linear.in_features, nc)


class ClassifyMetrics:
    """top-1 / top-5 accuracy from lists of per-batch (N, <= 5) predicted indices and (N,) targets (utils/metrics.py:1450-1501)."""

    keys = ["metrics/accuracy_top1", "metrics/accuracy_top5"]

    def __init__(self):
        self.top1 = self.top5 = 0

    def process(self, targets, pred):
        pred, targets = torch.cat(pred), torch.cat(targets)
        correct = (targets[:, None] == pred).float()
        acc = torch.stack((correct[:, 0], correct.max(1).values), dim=1)
        self.top1, self.top5 = acc.mean(0).tolist()

    @property
    def fitness(self):
        return (self.top1 + self.top5) / 2

    @property
    def results_dict(self):
        return dict(zip([*self.keys, "fitness"], [self.top1, self.top5, self.fitness]))


def head_cases():
    """(name, c1, (h, w), nc, batch) of the per-op `Classify` goldens (tests/golden/ops_classify.npz)."""
    return [("c256_1x1_nc3", 256, (1, 1), 3, 2), ("c32_7x7_nc10", 32, (7, 7), 10, 3), ("c256_5x9_nc10", 256, (5, 9), 10, 1),
            ("c32_5x9_nc1000", 32, (5, 9), 1000, 2)]


def head_case(case, cls=Classify):
    """(module with procedural weights, input) of one head case; `cls` = this oracle's, the reference's or the product's Classify."""
    from ultralytics_pro_amd.utils import procedural as P
    name, c1, (h, w), nc, b = case
    m = cls(c1, nc).eval()
    P.apply_procedural_weights(m, family="yolov8n-cls")
    return m, P.uniform(f"unit:classify:{name}", (b, c1, h, w), -1.0, 1.0)


def metrics_case():
    """Hand-made top-5 lists (two batches) and targets: 7 rows - rank 1 hits at rows 0, 3, 6, rank 2-5 hits at rows 1, 4, misses at 2, 5."""
    pred = [torch.tensor([[3, 1, 4, 0, 5], [9, 2, 6, 5, 3], [5, 8, 9, 7, 1], [2, 7, 1, 8, 0]], dtype=torch.int32),
            torch.tensor([[6, 0, 2, 4, 9], [1, 4, 7, 3, 6], [0, 3, 1, 2, 8]], dtype=torch.int32)]
    targets = [torch.tensor([3, 5, 0, 2], dtype=torch.int32), torch.tensor([9, 8, 0], dtype=torch.int32)]
    return pred, targets
