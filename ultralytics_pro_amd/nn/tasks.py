"""Graph builder and layer executor with the reference's API (ultralytics/nn/tasks.py): `parse_model` resolves YAML rows
by class NAME (tasks.py:2836-2842) to the HIP operator library, `BaseModel._predict_once` is the layer loop
(:1046-1085).  `DetectionModel.compile()` walks that loop once under hipGraph capture with static buffers and replays
it per batch - HIP graphs instead of a tracing compiler.
"""

from __future__ import annotations

import ast
import contextlib
import math
import re
from copy import deepcopy
from pathlib import Path

import torch
import torch.nn as nn
import yaml

from .. import _lib as L
from ..engine import runtime as R
from .modules import (C2f, C2PSA, C3, C3k2, SPPF, BoT3, Bottleneck, Classify, Concat, Conv, Detect, Pose, Segment)
from .modules.conv import VirtualUpsample
from .modules.resample import MaxPool2d, Upsample, ZeroPad2d

CFG_DIR = Path(__file__).resolve().parents[1] / "cfg" / "models"

_NN_STANDINS = {"Upsample": Upsample, "MaxPool2d": MaxPool2d, "ZeroPad2d": ZeroPad2d}


def _registry():
    reg = {m.__name__: m for m in (Conv, C2f, C3, SPPF, BoT3, Bottleneck, Concat, Detect, Segment, Pose, C3k2, C2PSA, Classify)}
    try:
        from .modules.rtdetr import RTDETRDecoder
        reg["RTDETRDecoder"] = RTDETRDecoder
    except ImportError:
        pass
    return reg


# Classify is a base module: its row [nc] becomes [c1, nc] (c2 == nc is left unscaled, tasks.py:2848-2851)
BASE_MODULES = {"Conv", "C2f", "C3", "SPPF", "BoT3", "Bottleneck", "C3k2", "C2PSA", "Classify"}  # subset of base_modules, tasks.py:2446-2710
REPEAT_MODULES = {"C2f", "C3", "C3k2", "C2PSA"}  # subset of repeat_modules (BoT3 is not one: SURVEY §8a row 15)


def make_divisible(x, divisor):
    """Nearest multiple of divisor not below x (utils/ops.py:137-150)."""
    return math.ceil(x / divisor) * divisor


def yaml_model_load(path):
    """Load a model YAML; 'yolov8n.yaml' resolves to yolov8.yaml with scale 'n', 'yolov8n-seg.yaml' to yolov8-seg.yaml,
    'yolov8n-cls.yaml' to yolov8-cls.yaml and 'yolov8n-pose.yaml' to yolov8-pose.yaml (tasks.py:3147-3185)."""
    path = Path(path)
    stem, scale = path.stem, ""
    m = re.match(r"^(yolo(?:v)?\d+)([nslmx])$", stem)
    seg = re.match(r"^(yolo(?:v)?\d+)([ntslmx])-seg$", stem)
    cls = re.match(r"^(yolo(?:v)?\d+)([nslmx])-cls$", stem)
    pose = re.match(r"^(yolo(?:v)?\d+)([nslmx])-pose$", stem)
    if m:
        stem, scale = m.group(1), m.group(2)
    elif seg:
        stem, scale = seg.group(1) + "-seg", seg.group(2)
    elif cls:
        stem, scale = cls.group(1) + "-cls", cls.group(2)
    elif pose:
        stem, scale = pose.group(1) + "-pose", pose.group(2)
    cands = [path] if path.is_file() else sorted(CFG_DIR.rglob(stem + ".yaml"))
    if not cands:
        raise FileNotFoundError(f"model YAML '{path}' not found under {CFG_DIR}")
    d = yaml.safe_load(cands[0].read_text())
    d["scale"] = scale
    d["yaml_file"] = str(path)
    return d


def parse_model(d, ch, verbose=False):
    """Parse a YOLO model.yaml dictionary into an nn.Sequential of HIP modules + sorted save list (tasks.py:2409-3146)."""
    d = deepcopy(d)
    reg = _registry()
    legacy = True  # v3/v5/v8 YAMLs never flip it (tasks.py:2424)
    max_channels = float("inf")
    nc, scales = d.get("nc"), d.get("scales")
    depth, width = d.get("depth_multiple", 1.0), d.get("width_multiple", 1.0)
    scale = d.get("scale")
    if scales:
        if not scale:
            scale = next(iter(scales.keys()))  # "no model scale passed. Assuming scale='n'" (tasks.py:2430-2433)
        depth, width, max_channels = scales[scale][:3]
    ch = [ch]
    layers, save, c2 = [], [], ch[-1]
    for i, (f, n, mname, args) in enumerate(d["backbone"] + d["head"]):
        if mname.startswith("nn."):
            if mname[3:] not in _NN_STANDINS:
                raise L.UpaError(f"'{mname}' has no HIP implementation (supported: {sorted(_NN_STANDINS)})")
            m = _NN_STANDINS[mname[3:]]
        elif mname in reg:
            m = reg[mname]
        else:
            raise L.UpaError(f"module '{mname}' is outside the hot-path operator set {sorted(reg)} (SURVEY §2)")
        args = list(args)
        for j, a in enumerate(args):
            if isinstance(a, str):
                with contextlib.suppress(ValueError):
                    args[j] = nc if a == "nc" else d.get("kpt_shape") if a == "kpt_shape" else ast.literal_eval(a)
        n = n_ = max(round(n * depth), 1) if n > 1 else n
        if mname in BASE_MODULES:
            c1, c2 = ch[f], args[0]
            if c2 != nc:
                c2 = make_divisible(min(c2, max_channels) * width, 8)
            args = [c1, c2, *args[1:]]
            if mname in REPEAT_MODULES:
                args.insert(2, n)
                n = 1
            if mname == "C3k2":  # YOLO11: the DWConv Detect class branch, C3k inner blocks for M/L/X (tasks.py:2859-2863)
                legacy = False
                if scale in "mlx":
                    args[3] = True
        elif mname == "Concat":
            c2 = sum(ch[x] for x in f)
        elif mname in ("Detect", "Segment", "Pose"):
            args.append([ch[x] for x in f])
            if mname == "Segment":  # npr (tasks.py:2990-2991)
                args[2] = make_divisible(min(args[2], max_channels) * width, 8)
            m.legacy = legacy
        elif mname == "RTDETRDecoder":
            args.insert(1, [ch[x] for x in f])
        else:
            c2 = ch[f]
        try:
            m_ = HipSequential(*(m(*args) for _ in range(n))) if n > 1 else m(*args)
        except L.UpaError as e:  # a refused Pose row names its layer (every other module's message stays as it was)
            if mname != "Pose":
                raise
            raise L.UpaError(f"layer {i} ({mname}{args!s}): {e}") from None
        t = f"{m.__module__}.{m.__name__}"
        m.np = sum(x.numel() for x in m_.parameters())
        m_.np = m.np
        m_.i, m_.f, m_.type = i, f, t
        if verbose:
            print(f"{i:>3}{f!s:>20}{n_:>3}{m_.np:10.0f}  {t:<45}{args!s:<30}")
        save.extend(x % i for x in ([f] if isinstance(f, int) else f) if x != -1)
        layers.append(m_)
        if i == 0:
            ch = []
        ch.append(c2)
    return nn.Sequential(*layers), sorted(save)


def _out_hw(m, h, w):
    """Spatial size of a layer's output for an (h, w) input (only stride-changing layers matter)."""
    for mm in (list(m) if isinstance(m, HipSequential) else [m]):
        if isinstance(mm, Conv):
            k, s, p = mm.conv.kernel_size[0], mm.conv.stride[0], mm.conv.padding[0]
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        elif isinstance(mm, MaxPool2d):
            k, s, p = mm.kernel_size, mm.stride, mm.padding
            h, w = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
        elif isinstance(mm, Upsample):
            h, w = 2 * h, 2 * w
        elif isinstance(mm, ZeroPad2d):
            h, w = h + mm.padding[2] + mm.padding[3], w + mm.padding[0] + mm.padding[1]
    return h, w


def _out_channels(m, ch):
    """Output channels of layer m given the per-layer list so far."""
    last = m[-1] if isinstance(m, HipSequential) else m
    if isinstance(last, Conv):
        return last.conv.out_channels
    if isinstance(last, (C2f, SPPF, C2PSA)):
        return last.cv2.conv.out_channels
    if isinstance(last, (C3, BoT3)):
        return last.cv3.conv.out_channels
    if isinstance(last, Bottleneck):
        return last.cv2.conv.out_channels
    if isinstance(last, Concat):
        return sum(ch[m.i - 1 if j == -1 else j] for j in m.f)
    src = m.f if isinstance(m.f, int) else m.f[0]
    return ch[m.i - 1 if src == -1 else src] if ch else 0


class HipSequential(nn.Sequential):
    """n > 1 repeats of a module (tasks.py:3113); the last repeat may write into a caller-provided view."""

    def forward(self, x, out=None):
        mods = list(self)
        for j, m in enumerate(mods):
            x = m(x, out=out) if (j == len(mods) - 1 and out is not None) else m(x)
        return x


_OUT_CAPABLE = (Conv, C2f, C3, SPPF, BoT3, Bottleneck, Upsample, MaxPool2d, HipSequential)


class BaseModel(nn.Module):
    """Base class: forward -> predict -> _predict_once (tasks.py:987-1134)."""

    def forward(self, x, *args, **kwargs):
        if isinstance(x, dict):
            # the reference computes the loss here (tasks.py:1003-1004); on the HIP path the train-mode forward, the loss and
            # the explicit backward live together in engine/trainer.py (no torch autograd), so a batch dict is its input
            raise L.UpaError("a batch dict is a training step: use ultralytics_pro_amd.engine.trainer.DetectionTrainer(model)"
                             ".step(batch['img'], batch) - forward, v8DetectionLoss and backward run there as HIP kernels")
        return self.predict(x, *args, **kwargs)

    def predict(self, x, profile=False, visualize=False, augment=False, embed=None):
        if augment or visualize or embed is not None or profile:
            raise L.UpaError("augment / visualize / embed / profile are outside the hot-path scope")
        return self._predict_once(x)

    opts = None  # _lib.Opts: dispatch overrides of THIS model's kernel calls (None = the options in force / library defaults)

    def _predict_once(self, x):
        """The layer loop (see `_predict_once_impl`), run under this model's dispatch options when it has any."""
        if self.opts is None:
            return self._predict_once_impl(x)
        with R.use_opts(self.opts):
            return self._predict_once_impl(x)

    def _predict_once_impl(self, x):
        """The layer loop: route `m.f`, run, save if in `save` (tasks.py:1046-1085).

        Concat-by-construction: a layer whose output feeds a `Concat` row writes straight into its channel slice of
        that Concat's buffer (`out=` view), so Upsample+Concat / Conv+Concat never copy (yolov8.yaml rows 10-21)."""
        place = self._concat_placement()
        y, cat_buf = [], {}
        det = self.model[-1] if isinstance(self.model[-1], Detect) else None
        det_level = {}
        if det is not None:
            det._pend().clear()
            det_level = {(det.i - 1 if j == -1 else j): k for k, j in enumerate(det.f)} if isinstance(det.f, list) else {}
            if det_level and torch.is_tensor(x) and x.dim() == 4:
                # the Detect input sizes follow statically from the image size: the head can decode each level into its
                # anchor range of the output the moment that level's feature map exists
                ih, iw = (x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else (x.shape[2], x.shape[3])
                hw = self._static_hw(int(ih), int(iw))
                srcs = sorted(det_level, key=lambda j: det_level[j])
                det.begin(int(x.shape[0]), [hw[j] for j in srcs], getattr(self, "compute_dtype", None) or x.dtype, x.device)
        fused_stem = self._stem_fusable(x, place)
        virt = {}  # concat layer index -> VirtualUpsample: an Upsample feeding that Concat which was not launched (see below)
        pooled = None  # (row index of a MaxPool2d that the previous Conv row already applied, its output)
        for m in self.model:
            if pooled is not None and m.i == pooled[0]:
                x, pooled = pooled[1], None
                y.append(x if m.i in self.save else None)
                continue
            if self._pool_fusable(m, place):  # Conv -> MaxPool2d(2, 2, 0): one launch, the conv output never reaches HBM
                xin = x if m.f == -1 else y[m.f]
                yp = m.forward_pool2(xin) if torch.is_tensor(xin) else None
                if yp is not None:
                    pooled = (m.i + 1, yp)
                    y.append(None)
                    continue
            if self._down_fusable(m, place):  # C2f(32, 32, n = 1) -> Conv(32, 64, 3, 2): one launch, the block's output never reaches HBM
                xin = x if m.f == -1 else y[m.f]
                yp = m.forward_down(xin, self.model[m.i + 1]) if torch.is_tensor(xin) else None
                if yp is not None:
                    pooled = (m.i + 1, yp)
                    y.append(None)
                    continue
            if fused_stem and m.i == 0:  # layers 0 and 1 run as ONE kernel: the stem output never reaches HBM
                x = self._fused_stem(x)
                y.append(None)
                continue
            if fused_stem and m.i == 1:
                y.append(x if 1 in self.save else None)
                continue
            if m.f != -1:
                x = y[m.f] if isinstance(m.f, int) else [x if j == -1 else y[j] for j in m.f]
            if m.i in place and torch.is_tensor(x):
                li, c0, c1, ctot = place[m.i]
                n, _, h, w = x.shape
                oh, ow = _out_hw(m, h, w)
                buf = cat_buf.get(li)
                if buf is None:
                    dt = getattr(self, "compute_dtype", None) if (x.shape[1] <= 4 and not R.is_nhwc_view(x)) else None
                    buf = R.alloc_nhwc(n, ctot, oh, ow, dt or x.dtype, x.device, key=(id(self.model[li]), "y"))
                    cat_buf[li] = buf
                if self._virtual_upsample_ok(m, li, c0, c1, x):
                    # Upsample -> Concat -> C2f: the C2f's cv1 reads the half-resolution tensor at (y/2, x/2) itself
                    # (upa_conv1x1_upcat); the upsampled copy (52 + 26 MB per step for yolov8n) is never written
                    virt[li] = VirtualUpsample(x, c1 - c0, (lambda m=m, x=x, dst=buf[:, c0:c1]: m(x, out=dst)))
                    x = buf[:, c0:c1]
                elif m.f == -1 and (m.i - 1) in virt:
                    x = m(x, out=buf[:, c0:c1], up=virt.pop(m.i - 1))
                else:
                    x = m(x, out=buf[:, c0:c1])
            elif isinstance(m, Concat) and m.i in cat_buf:
                buf, c0 = cat_buf[m.i], 0
                for t in x:  # anything not produced in place (none for the reference YAMLs) is copied by Concat rules
                    c = int(t.shape[1])
                    dst = buf[:, c0:c0 + c]
                    if not (t.data_ptr() == dst.data_ptr() and t.stride() == dst.stride()):
                        vs, vd = R.view_of(R.to_nhwc(t, buf.dtype)), R.view_of(dst)
                        L.check(L.lib().upa_copy_view(vs.ptr, vs.n, vs.h, vs.w, vs.c, vs.ld, vd.ptr, vd.ld, vs.dtype,
                                                      L.current_stream(t.device)), "copy_view")
                    c0 += c
                x = buf
            elif m.f == -1 and (m.i - 1) in virt:
                x = m(x, up=virt.pop(m.i - 1))
            else:
                x = m(x)
            if virt and not isinstance(m, (Upsample, Concat)):
                raise L.UpaError(f"virtual Upsample of Concat row(s) {sorted(virt)} was not consumed by row {m.i}")
            y.append(x if m.i in self.save else None)
            if m.i in det_level and torch.is_tensor(x):  # a Detect input is ready: start that level's branches now
                det.start_level(det_level[m.i], x)
        return x

    virtual_upsample = True

    def _virtual_upsample_ok(self, m, li: int, c0: int, c1: int, x) -> bool:
        """An Upsample row may stay unlaunched when it fills the LEADING channels of a Concat that only the next row reads,
        that row is a C2f or a C3 (whose 1x1 convs can read the half-resolution tensor), nothing else reads the Upsample row
        itself (a custom YAML may route it elsewhere: then it is materialised) and the data is bf16."""
        if not (self.virtual_upsample and isinstance(m, Upsample) and c0 == 0 and (c1 - c0) % 32 == 0
                and x.dtype == torch.bfloat16 and li not in self.save and m.i not in self.save and li + 1 < len(self.model)):
            return False
        nxt = self.model[li + 1]
        if isinstance(nxt, HipSequential):  # n > 1 repeats of a C3: only the first one reads the Concat
            return False
        if isinstance(nxt, C3) and type(nxt) is C3:  # both 1x1 convs of a C3 read the Concat (cv1 and cv2)
            return nxt.f == -1 and nxt.cv1.conv.kernel_size == (1, 1) and nxt.cv2.conv.kernel_size == (1, 1) and not self.training
        return isinstance(nxt, C2f) and nxt.f == -1 and nxt.cv1.conv.kernel_size == (1, 1) and not self.training

    def _static_hw(self, h: int, w: int):
        """Output (h, w) of every layer for an (h, w) image: a shape walk of the graph, no tensors (cached per size)."""
        cache = self.__dict__.setdefault("_hw_cache", {})
        out = cache.get((h, w))
        if out is None:
            out = []
            for m in self.model:
                f = m.f if isinstance(m.f, int) else m.f[0]
                ih, iw = (h, w) if not out else out[-1]
                if f != -1:
                    ih, iw = out[f]
                out.append(_out_hw(m, ih, iw))
            cache[(h, w)] = out
        return out

    fuse_pool = True  # Conv + MaxPool2d(2, 2, 0) rows as one launch where the conv kernel has the pooled epilogue (A/B switch)

    def _pool_fusable(self, m, place) -> bool:
        """Row m is a Conv whose ONLY reader is the next row, an nn.MaxPool2d(2, 2, 0) (yolov3-tiny.yaml rows 0-7): the pool can run in
        the conv's epilogue (`Conv.forward_pool2`; bf16 only - it returns None otherwise and the rows run separately)."""
        if not self.fuse_pool or type(m) is not Conv or m.i + 1 >= len(self.model) or isinstance(m.f, list):
            return False
        if getattr(self, "compute_dtype", None) != torch.bfloat16 or m.training:
            return False
        nxt = self.model[m.i + 1]
        if type(nxt) is not MaxPool2d or nxt.f != -1 or (nxt.kernel_size, nxt.stride, nxt.padding) != (2, 2, 0):
            return False
        return m.i not in self.save and m.i not in place and (m.i + 1) not in place

    fuse_down = True  # C2f(32, 32, n = 1) + the stride-2 Conv(32, 64, 3, 2) row behind it as one launch (A/B switch; upa_opts.no_c2f16_down too)

    def _down_fusable(self, m, place) -> bool:
        """Row m is a C2f whose ONLY reader is the next row, a stride-2 3x3 Conv (yolov8.yaml rows 2-3): `C2f.forward_down` may run both
        as one kernel (bf16, the 16-channel-half form only - it returns None otherwise and the rows run separately)."""
        if not self.fuse_down or type(m) is not C2f or m.i + 1 >= len(self.model) or isinstance(m.f, list):
            return False
        if getattr(self, "compute_dtype", None) != torch.bfloat16 or m.training or m.c != 16:
            return False
        nxt = self.model[m.i + 1]
        if type(nxt) is not Conv or nxt.f != -1 or nxt.conv.stride != (2, 2):
            return False
        return m.i not in self.save and m.i not in place and (m.i + 1) not in place

    def _stem_fusable(self, x, place) -> bool:
        """yolov8n's / yolov8s' / yolov5's first two rows (Conv(3,16,3|6,2) -> Conv(16,32,3,2) or Conv(3,32,3,2) -> Conv(32,64,3,2), SiLU,
        bf16 NCHW input, neither output used by a later row other than the next one): `upa_stem_conv_fused_c` runs them as one kernel
        (csrc/stem.hip)."""
        if self.__dict__.get("_no_stem_fusion") or len(self.model) < 3 or not torch.is_tensor(x):
            return False
        a, b = self.model[0], self.model[1]
        if not (type(a) is Conv and type(b) is Conv) or b.f != -1 or 0 in self.save or 0 in place or 1 in place:
            return False
        if getattr(self, "compute_dtype", None) != torch.bfloat16 or x.dtype != torch.bfloat16 or x.dim() != 4:
            return False
        ca, cb = a.conv, b.conv
        first = (ca.in_channels, ca.out_channels, ca.kernel_size, ca.stride, ca.padding)
        ok = first in ((3, 16, (3, 3), (2, 2), (1, 1)), (3, 16, (6, 6), (2, 2), (2, 2)), (3, 32, (3, 3), (2, 2), (1, 1)),
                       (3, 32, (3, 3), (1, 1), (1, 1))) and \
            (cb.in_channels, cb.out_channels, cb.kernel_size, cb.stride, cb.padding) == (first[1], 2 * first[1], (3, 3), (2, 2), (1, 1)) and \
            isinstance(a.act, nn.SiLU) and isinstance(b.act, nn.SiLU) and not a.training
        n, c, h, w = x.shape
        s0 = int(ca.stride[0])
        return bool(ok and c == 3 and x.is_contiguous() and x.data_ptr() % 16 == 0 and w % 8 == 0 and h % (2 * s0) == 0 and w % (2 * s0) == 0)

    def _fused_stem(self, x):
        a, b = self.model[0], self.model[1]
        pa = a._packed(a.conv, getattr(a, "bn", None), x.device, torch.bfloat16, True)
        pb = b._packed(b.conv, getattr(b, "bn", None), x.device, torch.bfloat16, False)
        n, _, h, w = x.shape
        c0, s0 = int(a.conv.out_channels), int(a.conv.stride[0])
        y = R.alloc_nhwc(n, 2 * c0, h // (2 * s0), w // (2 * s0), torch.bfloat16, x.device, key=(id(b), "y"))
        vy = R.view_of(y)
        L.check(L.lib().upa_stem_conv_fused_s(x.data_ptr(), n, h, w, int(a.conv.kernel_size[0]), s0, c0, pa.w.data_ptr(), pa.bias.data_ptr(),
                                              pb.w.data_ptr(), pb.bias.data_ptr(), vy.ptr, vy.ld, R.opts_ptr(),
                                              L.current_stream(x.device)), "stem_conv_fused")
        return y

    def _concat_placement(self):
        """{producer layer index: (concat layer index, c0, c1, c_total)} for producers that accept `out=`."""
        plan = self.__dict__.get("_cat_plan")
        if plan is None:
            plan, ch = {}, []
            for m in self.model:  # output channels per layer
                ch.append(_out_channels(m, ch))
            for m in self.model:
                if isinstance(m, Concat) and m.d == 1:
                    srcs = [(m.i - 1 if j == -1 else j) for j in m.f]
                    ctot, c0 = sum(ch[j] for j in srcs), 0
                    for j in srcs:
                        if j not in plan and isinstance(self.model[j], _OUT_CAPABLE) and srcs.count(j) == 1:
                            plan[j] = (m.i, c0, c0 + ch[j], ctot)
                        c0 += ch[j]
            self.__dict__["_cat_plan"] = plan
        return plan

    def fuse(self, verbose=True):
        """BN folding happens inside the HIP conv weights packing; kept for API parity (tasks.py:1120-1134)."""
        self._fused = True
        return self

    def is_fused(self, thresh=10):
        return bool(getattr(self, "_fused", False))

    # ---- compute dtype (the reference's `.half()`, autobackend.py:216: here bf16 storage / f32 accumulate) -----------
    def set_compute_dtype(self, dtype: torch.dtype):
        L.dtype_code(dtype)
        first = self.model[0]
        for m in first.modules():
            if isinstance(m, Conv):
                m.compute_dtype = dtype
                break
        self.compute_dtype = dtype
        self._graphs = {}
        return self

    # ---- hipGraph replay -----------------------------------------------------------------------------------------------
    def compile(self, example: torch.Tensor, post=None, micro_batches: int = 1, stream_priority: int = 0):
        """Capture `_predict_once(example)` (plus an optional post-processing callable) into a hipGraph.

        Returns a callable `run()`: copies nothing - the input is read from `example`'s storage at every replay
        (inputs already resident, as in a serving loop that writes frames into a fixed buffer).

        micro_batches > 1 splits the batch into that many sub-batches that are walked on separate HIP streams (parallel
        hipGraph branches): while one sub-batch's kernel drains (the 20x20 / 40x40 layers launch only a few hundred
        workgroups on 256 CUs) the other sub-batch's kernels fill the idle CUs.  `post` is applied per sub-batch and
        the results are returned as a list."""
        L.require_gpu(example, "compile")
        pool = R.BufferPool()
        if micro_batches > 1:
            if example.shape[0] % micro_batches:
                raise L.UpaError("batch must be divisible by micro_batches")
            step = example.shape[0] // micro_batches
            side = [torch.cuda.Stream(device=example.device, priority=stream_priority) for _ in range(micro_batches)]

            def body():
                main = torch.cuda.current_stream(example.device)
                fork = torch.cuda.Event()
                fork.record(main)
                outs = []
                for k in range(micro_batches):
                    side[k].wait_event(fork)
                    with torch.cuda.stream(side[k]), R.pool_tag(k + 1):
                        o = self._predict_once(example[k * step:(k + 1) * step])
                        outs.append(post(o) if post is not None else o)
                        ev = torch.cuda.Event()
                        ev.record(side[k])
                    main.wait_event(ev)
                return outs
        else:
            def body():
                out = self._predict_once(example)
                return post(out) if post is not None else out

        with torch.no_grad(), R.static_buffers(pool):
            body()  # warm-up: allocates every static buffer, packs weights, sets LDS attributes
            torch.cuda.synchronize(example.device)
            graph = R.HipGraph()
            result = graph.capture(body, device=example.device)
        torch.cuda.synchronize(example.device)

        def run():
            graph.replay(example.device)
            return result

        run.graph, run.pool, run.result = graph, pool, result
        return run


class DetectionModel(BaseModel):
    """YOLO detection model (tasks.py:1256-1340)."""

    def __init__(self, cfg="yolov8n.yaml", ch=3, nc=None, verbose=False):
        super().__init__()
        self.yaml = cfg if isinstance(cfg, dict) else yaml_model_load(cfg)
        if nc and nc != self.yaml["nc"]:
            self.yaml["nc"] = nc
        self.model, self.save = parse_model(deepcopy(self.yaml), ch=ch, verbose=verbose)
        self.names = {i: f"{i}" for i in range(self.yaml["nc"])}
        self.inplace = self.yaml.get("inplace", True)
        self.end2end = False
        self.compute_dtype = torch.float32
        m = self.model[-1]
        if isinstance(m, Detect):
            # The reference discovers strides with a 256x256 zero-image forward (tasks.py:1315-1331); the HIP build has
            # no CPU forward, so the same numbers come from the static shape walk of the graph.
            m.stride = torch.tensor([float(s) for s in self._infer_strides(ch)])
            self.stride = m.stride
            m.bias_init()
        else:
            self.stride = torch.Tensor([32])
        for mod in self.modules():  # initialize_weights (utils/torch_utils.py:463-473)
            if isinstance(mod, nn.BatchNorm2d):
                mod.eps = 1e-3
                mod.momentum = 0.03
        self.eval()

    def _infer_strides(self, ch=None):
        """Down-sampling factor of every Detect input from the layer strides (no tensors involved)."""
        scale = []
        for m in self.model:
            f = m.f
            if isinstance(m, Detect):
                return [scale[j] for j in f]
            fin = f if isinstance(f, int) else f[0]
            s = (scale[-1] if scale else 1.0) if fin == -1 else scale[fin]
            for mm in (list(m) if isinstance(m, HipSequential) else [m]):
                if isinstance(mm, Conv):
                    s *= mm.conv.stride[0]
                elif isinstance(mm, MaxPool2d):
                    s *= mm.stride
                elif isinstance(mm, Upsample):
                    s /= 2
            scale.append(s)
        return [32.0]


class SegmentationModel(DetectionModel):
    """YOLO segmentation model (tasks.py:1343-1365): a DetectionModel whose head is `Segment`.  Inference here; validation
    (box and mask mAP) is `engine.validator.SegmentationValidator`, training (v8SegmentationLoss) `engine.trainer.SegmentationTrainer`."""

    def __init__(self, cfg="yolov8n-seg.yaml", ch=3, nc=None, verbose=False):
        super().__init__(cfg=cfg, ch=ch, nc=nc, verbose=verbose)
        if not isinstance(self.model[-1], Segment):
            raise L.UpaError(f"SegmentationModel needs a Segment head, {cfg} ends in {type(self.model[-1]).__name__}")


class PoseModel(DetectionModel):
    """YOLO pose model (tasks.py:1368-1395): a DetectionModel whose head is `Pose`.  `data_kpt_shape` overrides the YAML's `kpt_shape`
    as in the reference.  Inference here; validation (box and pose mAP) is `engine.validator.PoseValidator`, training (v8PoseLoss)
    `engine.trainer.PoseTrainer`."""

    def __init__(self, cfg="yolov8n-pose.yaml", ch=3, nc=None, data_kpt_shape=(None, None), verbose=False):
        if not isinstance(cfg, dict):
            cfg = yaml_model_load(cfg)
        if any(data_kpt_shape) and list(data_kpt_shape) != list(cfg["kpt_shape"]):
            cfg["kpt_shape"] = data_kpt_shape
        super().__init__(cfg=cfg, ch=ch, nc=nc, verbose=verbose)
        if not isinstance(self.model[-1], Pose):
            raise L.UpaError(f"PoseModel needs a Pose head, {cfg.get('yaml_file', 'the given dict')} ends in {type(self.model[-1]).__name__}")
        self.kpt_shape = tuple(int(v) for v in self.model[-1].kpt_shape)


RTDETRDetectionModel = DetectionModel  # eval path differs only in the head module (tasks.py:1608)


class ClassificationModel(BaseModel):
    """YOLO classification model (tasks.py:1516-1605): backbone rows + a `Classify` head; eval forward returns `(probs, logits)`.
    The input is a float NCHW batch in [0, 1] (the reference's `classify_transforms` preprocessing is not part of this package).
    BatchNorm keeps torch's defaults (eps 1e-5), as in the reference: its `_from_yaml` does not run `initialize_weights`.
    The layer loop, `fuse()`, `set_compute_dtype` and `compile` are BaseModel's; no Detect preparation runs for a Classify tail."""

    def __init__(self, cfg="yolov8n-cls.yaml", ch=3, nc=None, verbose=False):
        super().__init__()
        self.yaml = cfg if isinstance(cfg, dict) else yaml_model_load(cfg)
        ch = self.yaml["channels"] = self.yaml.get("channels", ch)
        if nc and nc != self.yaml["nc"]:
            self.yaml["nc"] = nc
        elif not nc and not self.yaml.get("nc", None):
            raise ValueError("nc not specified. Must specify nc in model.yaml or function arguments.")
        self.model, self.save = parse_model(deepcopy(self.yaml), ch=ch, verbose=verbose)
        if not isinstance(self.model[-1], Classify):
            raise L.UpaError(f"ClassificationModel needs a Classify head, {cfg} ends in {type(self.model[-1]).__name__}")
        self.stride = torch.Tensor([1])  # no stride constraints
        self.names = {i: f"{i}" for i in range(self.yaml["nc"])}
        self.compute_dtype = torch.float32
        self.eval()

    @staticmethod
    def reshape_outputs(model, nc):
        """Give the model's `Classify` head `nc` outputs (tasks.py:1575-1586; the torchvision-backbone branches are not provided)."""
        name, m = list((model.model if hasattr(model, "model") else model).named_children())[-1]
        if not isinstance(m, Classify):
            raise L.UpaError(f"reshape_outputs: only a Classify head is supported, the last module is {type(m).__name__}")
        if m.linear.out_features != nc:
            m.linear = torch.nn.Linear(m.linear.in_features, nc)
            m.__dict__.pop("_pk_cache", None)
            if hasattr(model, "names"):
                model.names = {i: f"{i}" for i in range(nc)}
            if hasattr(model, "_graphs"):
                model._graphs = {}
