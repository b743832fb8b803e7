"""ORACLE for YOLO11 (test infrastructure, never on the product path).

CPU restatement, in plain torch f32 ops, of the reference modules YOLO11 adds on top of the v8 operator set, composed with the
existing oracle pieces (oracle/modules.py: Conv, C2f, C3, Bottleneck, SPPF, Concat, the Detect decode).  Citations are paths relative to
the reference's ultralytics/ package.  The GPU tests compare the HIP path against this module (the reference is not available there);
tests/test_yolo11_builder.py pins it to the goldens tools/gen_golden_yolo11.py captured from the imported reference.
"""

from __future__ import annotations

import ast
import contextlib
import math
from copy import deepcopy

import torch
import torch.nn as nn

from oracle import modules as om
from oracle import tasks as ot


class DWConv(om.Conv):
    """Depth-wise convolution: Conv with groups = gcd(c1, c2) (nn/modules/conv.py:411-425)."""

    def __init__(self, c1, c2, k=1, s=1, d=1, act=True):
        super().__init__(c1, c2, k, s, g=math.gcd(c1, c2), d=d, act=act)


class C3k(om.C3):
    """C3 with k x k Bottlenecks (nn/modules/block.py:1510-1530)."""

    def __init__(self, c1, c2, n=1, shortcut=True, g=1, e=0.5, k=3):
        super().__init__(c1, c2, n, shortcut, g, e)
        c_ = int(c2 * e)
        self.m = nn.Sequential(*(om.Bottleneck(c_, c_, shortcut, g, k=(k, k), e=1.0) for _ in range(n)))


class C3k2(om.C2f):
    """C2f whose inner blocks are C3k(c, c, 2) or Bottleneck(c, c) with e = 0.5 (nn/modules/block.py:1485-1507)."""

    def __init__(self, c1, c2, n=1, c3k=False, e=0.5, g=1, shortcut=True):
        super().__init__(c1, c2, n, shortcut, g, e)
        self.m = nn.ModuleList(C3k(self.c, self.c, 2, shortcut, g) if c3k else om.Bottleneck(self.c, self.c, shortcut, g) for _ in range(n))


class v10_Attention(nn.Module):  # noqa: N801
    """nn/modules/block.py:1668-1722: qkv 1x1 -> per head softmax(scale q^T k) applied to v, + pe(v) -> proj 1x1."""

    def __init__(self, dim, num_heads=8, attn_ratio=0.5):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = dim // num_heads
        self.key_dim = int(self.head_dim * attn_ratio)
        self.scale = self.key_dim ** -0.5
        h = dim + self.key_dim * num_heads * 2
        self.qkv = om.Conv(dim, h, 1, act=False)
        self.proj = om.Conv(dim, dim, 1, act=False)
        self.pe = om.Conv(dim, dim, 3, 1, g=dim, act=False)

    def core(self, qkv, H, W):
        """softmax(scale q^T k) applied to v, + pe(v): the part `upa_psa_attention` computes (:1711-1719)."""
        B = qkv.shape[0]
        N = H * W
        q, k, v = qkv.view(B, self.num_heads, self.key_dim * 2 + self.head_dim, N).split([self.key_dim, self.key_dim, self.head_dim], dim=2)
        attn = ((q.transpose(-2, -1) @ k) * self.scale).softmax(dim=-1)
        C = self.num_heads * self.head_dim
        return (v @ attn.transpose(-2, -1)).view(B, C, H, W) + self.pe(v.reshape(B, C, H, W))

    def probs(self, x):
        """The attention matrix (B, heads, N, N) for input x: lets a test check that the softmax is not degenerate."""
        B, _, H, W = x.shape
        q, k, _ = self.qkv(x).view(B, self.num_heads, self.key_dim * 2 + self.head_dim, H * W).split(
            [self.key_dim, self.key_dim, self.head_dim], dim=2)
        return ((q.transpose(-2, -1) @ k) * self.scale).softmax(dim=-1)

    def forward(self, x):
        _, _, H, W = x.shape
        return self.proj(self.core(self.qkv(x), H, W))


class PSABlock(nn.Module):
    """x + attn(x), then x + ffn(x) (nn/modules/block.py:1724-1766)."""

    def __init__(self, c, attn_ratio=0.5, num_heads=4, shortcut=True):
        super().__init__()
        self.attn = v10_Attention(c, attn_ratio=attn_ratio, num_heads=num_heads)
        self.ffn = nn.Sequential(om.Conv(c, c * 2, 1), om.Conv(c * 2, c, 1, act=False))
        self.add = shortcut

    def forward(self, x):
        x = x + self.attn(x) if self.add else self.attn(x)
        return x + self.ffn(x) if self.add else self.ffn(x)


class C2PSA(nn.Module):
    """cv1 -> split (a, b) -> b = PSABlocks(b) -> cv2(cat(a, b)) (nn/modules/block.py:1829-1881)."""

    def __init__(self, c1, c2, n=1, e=0.5):
        super().__init__()
        assert c1 == c2
        self.c = int(c1 * e)
        self.cv1 = om.Conv(c1, 2 * self.c, 1, 1)
        self.cv2 = om.Conv(2 * self.c, c1, 1)
        self.m = nn.Sequential(*(PSABlock(self.c, attn_ratio=0.5, num_heads=self.c // 64) for _ in range(n)))

    def forward(self, x):
        a, b = self.cv1(x).split((self.c, self.c), dim=1)
        return self.cv2(torch.cat((a, self.m(b)), 1))


class Detect(om.Detect):
    """Detect with the non-legacy class branch DW3x3 -> 1x1 -> DW3x3 -> 1x1 -> 1x1 (nn/modules/head.py:98-110); the box branch, forward
    and decode are the legacy ones (oracle/modules.py)."""

    def __init__(self, nc=80, ch=()):
        super().__init__(nc, ch)
        c3 = max(ch[0], min(self.nc, 100))
        self.cv3 = nn.ModuleList(
            nn.Sequential(nn.Sequential(DWConv(x, x, 3), om.Conv(x, c3, 1)), nn.Sequential(DWConv(c3, c3, 3), om.Conv(c3, c3, 1)),
                          nn.Conv2d(c3, self.nc, 1))
            for x in ch)


_MODULES = {m.__name__: m for m in (om.Conv, om.C2f, om.C3, om.SPPF, om.Bottleneck, om.Concat, C3k2, C2PSA)}
_BASE = {om.Conv, om.C2f, om.C3, om.SPPF, om.Bottleneck, C3k2, C2PSA}  # nn/tasks.py:2446-2710
_REPEAT = {om.C2f, om.C3, C3k2, C2PSA}  # nn/tasks.py:2711-2760


def parse_model(d, ch):
    """oracle/tasks.py:parse_model plus the YOLO11 rows: C3k2 turns the legacy Detect off and, for scales m / l / x, forces
    c3k = True (nn/tasks.py:2859-2863)."""
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
    for i, (f, n, m, args) in enumerate(d["backbone"] + d["head"]):
        m = getattr(nn, m[3:]) if "nn." in m else (Detect if m == "Detect" else _MODULES[m])
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
            if m in _REPEAT:
                args.insert(2, n)
                n = 1
            if m is C3k2:
                legacy = False
                if scale in "mlx":
                    args[3] = True
        elif m is om.Concat:
            c2 = sum(ch[x] for x in f)
        elif m is Detect:
            args.append([ch[x] for x in f])
            if legacy:
                m = om.Detect
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


class DetectionModel(ot.DetectionModel):
    """oracle/tasks.py:DetectionModel on the YOLO11 builder (stride discovery, bias init, BN eps, fuse and the layer loop unchanged)."""

    def __init__(self, cfg="yolov11n.yaml", ch=3, nc=None):
        nn.Module.__init__(self)
        self.yaml = cfg if isinstance(cfg, dict) else ot.yaml_model_load(cfg)
        if nc and nc != self.yaml["nc"]:
            self.yaml["nc"] = nc
        self.model, self.save = parse_model(self.yaml, ch=ch)
        self.names = {i: f"{i}" for i in range(self.yaml["nc"])}
        self.inplace = True
        self.end2end = False
        m = self.model[-1]
        s = 256  # nn/tasks.py:1315-1331, as in oracle/tasks.py
        self.eval()
        m.training = True
        with torch.no_grad():
            outs = self._predict_once(torch.zeros(1, ch, s, s))
        m.stride = torch.tensor([s / x.shape[-2] for x in outs])
        self.stride = m.stride
        m.bias_init()
        for mod in self.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.eps = 1e-3
                mod.momentum = 0.03
        self.eval()


def op_cases():
    """(name, oracle module factory, input shape) of the per-op goldens (tests/golden/ops_yolo11.npz): the reference classes take
    the same constructor arguments, so tools/gen_golden_yolo11.py builds the reference twin from the same row."""
    return [
        ("dwconv_s1", "DWConv", (64, 64, 3, 1), (2, 64, 9, 11)),
        ("dwconv_s2", "DWConv", (80, 80, 3, 2), (2, 80, 9, 11)),
        ("dwconv_c24", "DWConv", (24, 24, 3, 1), (1, 24, 5, 7)),
        ("c3k", "C3k", (64, 64, 2), (2, 64, 10, 10)),
        ("c3k2_bottleneck", "C3k2", (64, 64, 1, False, 0.25), (2, 64, 12, 12)),
        ("c3k2_c3k", "C3k2", (128, 128, 1, True), (2, 128, 8, 8)),
        ("v10_attention", "v10_Attention", (128, 2, 0.5), (2, 128, 10, 10)),
        ("psablock", "PSABlock", (128, 0.5, 2), (2, 128, 10, 10)),
        ("c2psa", "C2PSA", (256, 256, 1), (2, 256, 8, 8)),
    ]


ORACLE_CLASSES = {"DWConv": DWConv, "C3k": C3k, "C3k2": C3k2, "v10_Attention": v10_Attention, "PSABlock": PSABlock, "C2PSA": C2PSA}
