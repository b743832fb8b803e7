"""Training step of the detection model on the HIP path (BASELINE config 3).

Mirrors the reference's step - forward in train mode, `v8DetectionLoss`, `loss.sum() * world_size`, backward, gradient
all-reduce, `optimizer_step` = clip_grad_norm_(10) + SGD(nesterov) + EMA (ultralytics/engine/trainer.py:416-432,
:674-682, :891-950; utils/torch_utils.py:606-650; utils/loss.py:415-528) - without torch autograd: every layer has an
explicit forward that keeps what its explicit backward needs, all of it upa_* kernels (include/upa.h, "training step").

  Conv (conv -> BN(batch statistics) -> SiLU):  z = conv(x, W);  (mean, var) = stats(z);  y = act(bn(z)) (+ residual)
      backward: dz, dgamma, dbeta = bn_act_bwd(z, dy);  dW += wgrad(x, dz);  dx (+)= conv(dz, W^T flipped)
  C2f / Bottleneck / SPPF / Upsample / Concat / Detect: compositions of the above + pool / upsample backward kernels.

torch is used for memory, streams, views and torch.distributed (the gradient all-reduce over RCCL).  Parameters live
in one flat f32 buffer (grouped: biases | decayed weights | norm weights, trainer.py:917-926) so the optimizer is three
fused launches; `model.parameters()` are views into it, the state_dict stays the reference's.
`optimizer=` follows the reference's build_optimizer (trainer.py:891-950): SGD-Nesterov by default, Adam / AdamW as the same three
launches of upa_adam_ema behind one upa_adam_step_advance (second-moment buffer `V`, step count on the device), "auto" resolved from
`iterations` and the head's class count (`resolve_optimizer`).
The yolov8 module set is differentiable here (Conv, C2f, Bottleneck, SPPF, nn.Upsample, Concat, Detect), the yolov5-BoT3 set (the 6x6
stride-2 stem, bare C3, BoT3 = `MHSAT`: upa_mhsa_train_fwd / upa_mhsa_bwd) and, for classification, YOLO11's C3k2 (C3k inside) and C2PSA
(`AttentionT`: upa_psa_attention_train_fwd / _bwd, upa_dwconv2d_train_fwd / _bwd); other modules raise.  The non-legacy Detect head
of YOLO11 (depthwise class branch: `DWConvT`, upa_dwconv2d_bn_act_fwd / upa_dwconv_bn_act_bwd) trains with `yolo11=True` and raises
without it.

`ClassificationTrainer` is the same step with another tail (`_tail_op`): `ClassifyT` = the train-mode Classify head, global average
pool, exact-f32 linear, fused cross-entropy (v8ClassificationLoss, utils/loss.py:873-880) and their backward (include/upa.h, "image
classification training").

`SegmentationTrainer` is the detection step with the tail `SegmentT` = `DetectT` + the cv4 mask-coefficient chains + `ProtoT` (`ConvTransposeT`:
upa_conv_transpose2x2 / upa_conv_transpose2x2_bwd) and the mask term of v8SegmentationLoss (utils/loss.py:531-709) as upa_mask_loss on the
detection loss's per-anchor assignment (include/upa.h, "segmentation training"); the labels carry the overlap mask and `pack_mask_ids` maps the
kept gt rows to the values that mark them in it.
"""

from __future__ import annotations

import ctypes as C
import math

import numpy as np

import torch
import torch.nn as nn

from .. import _lib as L
from ..nn.modules import block as B
from ..nn.modules import conv as CV
from ..nn.modules import head as H
from ..nn.modules import resample as RS
from . import runtime as R

HYP = dict(lr=0.01, momentum=0.9, weight_decay=5e-4, max_norm=10.0, ema_decay=0.9999, ema_tau=2000.0,
           box=7.5, cls=0.5, dfl=1.5, beta2=0.999, adam_eps=1e-8)  # (beta2, adam_eps: Adam / AdamW only; `momentum` is their beta1)
OPTIMIZERS = ("SGD", "Adam", "AdamW", "auto")  # of the reference's build_optimizer names (trainer.py:930); the others are refused
# warm-up / accumulation schedule of the reference's training loop (engine/trainer.py:337-338, 392-413, 245; cfg/default.yaml)
SCHED = dict(nbs=64, warmup_epochs=3.0, warmup_momentum=0.8, warmup_bias_lr=0.1, lrf=0.01, epochs=100)
MAX_GT = 64        # initial gt-row capacity per image; grows with the data (the loss kernels take it at run time)
MAX_GT_CAP = 1024  # upa_detection_loss: LDS arrays of the assignment-resolve kernel


def _s(dev):
    return L.current_stream(dev)


class _Ctx:
    """Per-trainer scratch shared by all layers."""

    def __init__(self, device, dtype, wgrad_streams: int = 1):
        self.device, self.dtype = device, dtype
        self.code = L.dtype_code(dtype)
        self.es = 2 if dtype == torch.bfloat16 else 4
        self.E = 16 // self.es
        # channel-reduction scratch (per-block partial sums + combined sums), sized for c <= 1024
        self._ws = [torch.zeros(L.lib().upa_channel_reduce_workspace_bytes(1024) // 8, dtype=torch.float64, device=device) for _ in range(2)]
        # the Detect head's 40 x 40 / 20 x 20 levels run beside the 80 x 80 level on a second stream (`DetectT`): its own reduction
        # workspace (the reductions of one workspace must be stream-ordered)
        self.level_stream = torch.cuda.Stream(device=device)
        self._ws_sel = 0
        self.wgrad_ws = torch.empty(0, dtype=torch.uint8, device=device)  # weight-gradient partial sums (largest layer)
        # weight gradients run on a side stream (a parallel branch of the captured graph): a layer's dW only needs its
        # input and dz, so it overlaps the data-gradient / BN-backward chain of the layers in front of it
        # (wgrad_streams = 0: weight gradients on the main stream, no overlap - the A/B switch of that measurement)
        self.wgrad_streams = [torch.cuda.Stream(device=device) for _ in range(max(0, int(wgrad_streams)))]
        self.wgrad_wss = [self.wgrad_ws for _ in self.wgrad_streams]  # one partial-sum workspace per stream
        self.wgrad_rr = 0
        self.wgrad_pending = False


def _ctx_ws(self):
    return self._ws[self._ws_sel]


def _ctx_wgrad_ws_here(self):
    """The weight-gradient partial-sum workspace for a weight gradient launched on the CURRENT stream (`wgrad_streams = 0`): the main
    stream's, or - while `DetectT._fork_levels` runs the small Detect levels on the level stream - a second buffer of the same size:
    two streams must never write and reduce split-K partials in one buffer at the same time."""
    if self._ws_sel == 0:
        return self.wgrad_ws
    lv = self.__dict__.get("_wgrad_ws_level")
    if lv is None or lv.numel() < self.wgrad_ws.numel():
        lv = self.__dict__["_wgrad_ws_level"] = torch.empty(self.wgrad_ws.numel(), dtype=torch.uint8, device=self.device)
    return lv


_Ctx.ws = property(_ctx_ws)
_Ctx.wgrad_ws_here = property(_ctx_wgrad_ws_here)


def _new(n, c, h, w, dtype, dev, key):
    return R.alloc_nhwc(n, c, h, w, dtype, dev, key)


class ConvT:
    """Train-mode forward/backward of one conv (+ BatchNorm2d + activation, or + bias for the plain head outputs)."""

    def __init__(self, ctx: _Ctx, conv: nn.Conv2d, bn, act_code: int, name: str, no_dgrad: bool = False):
        """`no_dgrad`: the layer's input needs no gradient (the model's first layer).  Only such a layer may be yolov5's 6x6 stride-2 pad-2
        stem: its weight gradient has a kernel of its own and no transposed weights are packed for it."""
        if conv.groups != 1 or conv.dilation != (1, 1) or conv.kernel_size[0] != conv.kernel_size[1]:
            raise L.UpaError(f"training supports square kernels, groups=1, dilation=1 only ({name})")
        self.ctx, self.conv, self.bn, self.act, self.name = ctx, conv, bn, act_code, name
        self.k, self.s, self.p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        self.stem6 = bool(no_dgrad) and (self.k, self.s, self.p) == (6, 2, 2) and conv.in_channels == 3
        if (self.k not in (1, 3) or self.s not in (1, 2)) and not self.stem6:
            raise L.UpaError(f"training supports k in (1,3), stride in (1,2) ({name}: k={self.k} s={self.s})")
        self.cout, self.cin = conv.out_channels, conv.in_channels
        dev, code = ctx.device, ctx.code
        nb = L.lib().upa_conv_packed_weight_bytes(self.cout, self.cin, self.k, code)
        self.wp = torch.empty(nb, dtype=torch.uint8, device=dev)          # forward layout
        self.wpt = None
        if not self.stem6:
            nbt = L.lib().upa_conv_packed_weight_bytes(self.cin, self.cout, self.k, code)
            self.wpt = torch.empty(nbt, dtype=torch.uint8, device=dev)    # transposed + flipped (data gradient)
        if bn is not None:
            self.mean = torch.empty(self.cout, dtype=torch.float32, device=dev)
            self.var = torch.empty(self.cout, dtype=torch.float32, device=dev)
        self.phase = None
        if self.s == 2 and self.k == 3 and self.p == 1:
            # data gradient by output parity: four 2x2 kernels, stacked along the output channels into ONE cout -> 4 * cin conv
            # (V is [phase][cin][cout][2][2] = a (4 cin, cout, 2, 2) weight): dz is read once and the four phases are one launch
            nph = L.lib().upa_conv_packed_weight_bytes(4 * self.cin, self.cout, 2, code)
            self.phase_v = torch.empty(4 * self.cin * self.cout * 4, dtype=torch.float32, device=dev)
            self.phase = torch.empty(nph, dtype=torch.uint8, device=dev)
        self.x = self.z = None
        nws = L.lib().upa_conv2d_wgrad_workspace_bytes(self.cin, self.cout, self.k)
        if nws > ctx.wgrad_ws.numel():
            ctx.wgrad_ws = torch.empty(nws, dtype=torch.uint8, device=dev)  # shared by all layers (stream ordered)
            ctx.wgrad_wss = [ctx.wgrad_ws if j == 0 else torch.empty(nws, dtype=torch.uint8, device=dev)
                             for j in range(len(ctx.wgrad_streams))]

    def pack(self):
        lib, c = L.lib(), self.ctx
        w = self.conv.weight
        L.check(lib.upa_pack_conv_weight_dev(w.data_ptr(), self.cout, self.cin, self.k, c.code, 0, self.wp.data_ptr(),
                                             _s(c.device)), "pack_dev")
        if self.wpt is None:
            pass
        elif self.phase is None:
            L.check(lib.upa_pack_conv_weight_dev(w.data_ptr(), self.cout, self.cin, self.k, c.code, 1, self.wpt.data_ptr(),
                                                 _s(c.device)), "pack_dev_t")
        else:
            L.check(lib.upa_dgrad_s2_phase_weights(w.data_ptr(), self.cout, self.cin, self.phase_v.data_ptr(), _s(c.device)),
                    "phase_weights")
            L.check(lib.upa_pack_conv_weight_dev(self.phase_v.data_ptr(), 4 * self.cin, self.cout, 2, c.code, 0,
                                                 self.phase.data_ptr(), _s(c.device)), "pack_phase")

    def pack_descs(self):
        """(w_ptr, out_ptr, cout, cin, k, dtype, transpose_flip) of every repack `pack()` launches, for the batched form
        (upa_pack_conv_weights_batched); a stride-2 conv's phase kernels are read from `phase_v`, which
        `pack_phase_weights()` must have refreshed first."""
        c, w = self.ctx, self.conv.weight
        d = [(w.data_ptr(), self.wp.data_ptr(), self.cout, self.cin, self.k, c.code, 0)]
        if self.wpt is None:
            pass
        elif self.phase is None:
            d.append((w.data_ptr(), self.wpt.data_ptr(), self.cout, self.cin, self.k, c.code, 1))
        else:
            d.append((self.phase_v.data_ptr(), self.phase.data_ptr(), 4 * self.cin, self.cout, 2, c.code, 0))
        return d

    def pack_phase_weights(self):
        if self.phase is not None:
            L.check(L.lib().upa_dgrad_s2_phase_weights(self.conv.weight.data_ptr(), self.cout, self.cin,
                                                       self.phase_v.data_ptr(), _s(self.ctx.device)), "phase_weights")

    def _conv(self, x, wp, cout, k, s, p, out, bias=None, residual=None):
        vx, vy = R.view_of(x), R.view_of(out)
        rp, rld = (None, 0)
        if residual is not None:
            vr = R.view_of(residual)
            rp, rld = vr.ptr, vr.ld
        L.check(L.lib().upa_conv2d_bias_act(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, wp.data_ptr(),
                                            None if bias is None else bias.data_ptr(), vy.ptr, cout, vy.ld, rp, rld, k, s, p,
                                            L.ACT_NONE, vx.dtype, R.opts_ptr(), _s(x.device)), f"conv2d[{self.name}]")

    @staticmethod
    def _momentum(bn) -> float:
        if bn.momentum is None:
            raise L.UpaError("BatchNorm2d(momentum=None) (cumulative moving average) is not supported by the training step: the running "
                             "statistics kernel takes a fixed momentum (nn.BatchNorm2d default 0.1; the reference's YAMLs set 0.03)")
        return float(bn.momentum)

    def forward(self, x, out=None, residual=None):
        c, lib = self.ctx, L.lib()
        n, _, h, w = x.shape
        oh, ow = (h + 2 * self.p - self.k) // self.s + 1, (w + 2 * self.p - self.k) // self.s + 1
        self.x = x
        if self.bn is None:  # plain nn.Conv2d with bias: y = conv(x) + b
            y = out if out is not None else _new(n, self.cout, oh, ow, c.dtype, c.device, (id(self), "y"))
            self._conv(x, self.wp, self.cout, self.k, self.s, self.p, y, bias=self.conv.bias)
            return y
        z = _new(n, self.cout, oh, ow, c.dtype, c.device, (id(self), "z"))
        vx, vz = R.view_of(x), R.view_of(z)
        npix = vz.n * vz.h * vz.w
        bn = self.bn
        # conv + batch statistics + normalisation / activation in ONE call: on the kernels with a statistics epilogue the sums come from
        # the convolution's own workgroups (no pass over z), elsewhere the library runs conv -> reduce -> combine itself
        y = out if out is not None else _new(n, self.cout, oh, ow, c.dtype, c.device, (id(self), "y"))
        vy = R.view_of(y)
        rp, rld = (None, 0)
        if residual is not None:
            vr = R.view_of(residual)
            rp, rld = vr.ptr, vr.ld
        L.check(lib.upa_conv2d_bn_act_fwd(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, self.wp.data_ptr(), vz.ptr, self.cout, vz.ld,
                                          self.k, self.s, self.p, self._momentum(bn), self.mean.data_ptr(), self.var.data_ptr(),
                                          bn.running_mean.data_ptr(), bn.running_var.data_ptr(), bn.weight.data_ptr(),
                                          bn.bias.data_ptr(), float(bn.eps), self.act, vy.ptr, vy.ld, rp, rld, c.ws.data_ptr(),
                                          vx.dtype, R.opts_ptr(), _s(c.device)), f"conv2d_bn_act_fwd[{self.name}]")
        self.z = z
        return y

    def backward(self, dy, dx=None, accumulate=False):
        """dy: gradient of this layer's output (NHWC view). dx: view receiving / accumulating the input gradient."""
        c, lib = self.ctx, L.lib()
        if dx is not None and self.wpt is None:
            raise L.UpaError(f"{self.name}: the 6x6 stride-2 stem has no data gradient on HIP (first layer only)")
        vdy = R.view_of(dy)
        npix = vdy.n * vdy.h * vdy.w
        st = _s(c.device)
        if self.bn is not None and self.s == 1 and self.phase is None:
            # the common form in ONE library call: BN + activation backward, the weight gradient (on the side stream, behind an event),
            # the data gradient
            vz, vx = R.view_of(self.z), R.view_of(self.x)
            dz = _new(vz.n, vz.c, vz.h, vz.w, c.dtype, c.device, (id(self), "dz"))
            vdz = R.view_of(dz)
            bn = self.bn
            side_p, ws = None, c.wgrad_ws_here
            if c.wgrad_streams:
                j = c.wgrad_rr % len(c.wgrad_streams)
                c.wgrad_rr += 1
                side_p, ws = c.wgrad_streams[j].cuda_stream, c.wgrad_wss[j]
                c.wgrad_pending = True
            vdx = None if dx is None else R.view_of(dx)
            L.check(lib.upa_conv_bn_act_bwd(vx.ptr, vx.n, vx.h, vx.w, self.cin, vx.ld, vz.ptr, vdy.ptr, self.cout, vz.ld, vdy.ld,
                                            self.mean.data_ptr(), self.var.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(),
                                            float(bn.eps), self.act, vdz.ptr, vdz.ld, bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(),
                                            c.ws.data_ptr(), self.conv.weight.grad.data_ptr(), ws.data_ptr(), ws.numel(), side_p,
                                            None if dx is None else self.wpt.data_ptr(), None if dx is None else vdx.ptr,
                                            0 if dx is None else vdx.ld, int(accumulate), self.k, self.p, vz.dtype, R.opts_ptr(), st),
                    f"conv_bn_act_bwd[{self.name}]")
            return
        if self.bn is None:
            dz = dy
            L.check(lib.upa_channel_sum(vdy.ptr, npix, vdy.c, vdy.ld, self.conv.bias.grad.data_ptr(), 1, c.ws.data_ptr(),
                                        vdy.dtype, st), "bias_grad")
        else:
            vz = R.view_of(self.z)
            dz = _new(vz.n, vz.c, vz.h, vz.w, c.dtype, c.device, (id(self), "dz"))
            vdz = R.view_of(dz)
            bn = self.bn
            L.check(lib.upa_bn_act_bwd(vz.ptr, vdy.ptr, npix, vz.c, vz.ld, vdy.ld, self.mean.data_ptr(), self.var.data_ptr(),
                                       bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps), self.act, vdz.ptr, vdz.ld,
                                       bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(), 1, c.ws.data_ptr(), vz.dtype, st),
                    "bn_act_bwd")
        vx, vdz = R.view_of(self.x), R.view_of(dz)
        if not c.wgrad_streams:
            L.check(lib.upa_conv2d_wgrad(vx.ptr, vx.n, vx.h, vx.w, self.cin, vx.ld, vdz.ptr, self.cout, vdz.ld,
                                         self.conv.weight.grad.data_ptr(), self.k, self.s, self.p, 1, vx.dtype,
                                         c.wgrad_ws_here.data_ptr(), c.wgrad_ws_here.numel(), st), f"wgrad[{self.name}]")
        else:
            j = c.wgrad_rr % len(c.wgrad_streams)
            c.wgrad_rr += 1
            side, ws = c.wgrad_streams[j], c.wgrad_wss[j]
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(c.device))  # dz is ready
            side.wait_event(ev)
            L.check(lib.upa_conv2d_wgrad(vx.ptr, vx.n, vx.h, vx.w, self.cin, vx.ld, vdz.ptr, self.cout, vdz.ld,
                                         self.conv.weight.grad.data_ptr(), self.k, self.s, self.p, 1, vx.dtype,
                                         ws.data_ptr(), ws.numel(), side.cuda_stream), f"wgrad[{self.name}]")
            c.wgrad_pending = True
        if dx is None:
            return
        if self.phase is not None:
            # stride 2: the four 2x2 stride-1 correlations over dz (one per output parity) as one conv with 4 * cin output
            # channels + one interleave pass over its four channel blocks
            vdx = R.view_of(dx)
            rc = lib.upa_conv2d_dgrad_s2(vdz.ptr, vdz.n, vdz.h, vdz.w, self.cout, vdz.ld, self.phase.data_ptr(), vdx.ptr, vdx.h, vdx.w,
                                         self.cin, vdx.ld, int(accumulate), vdx.dtype, R.opts_ptr(), st)
            if rc != L.UPA_EUNSUPPORTED:  # one launch: the phase conv's epilogue writes dx's interleaved pixels itself
                L.check(rc, "conv2d_dgrad_s2")
                return
            t = _new(vdz.n, 4 * self.cin, vdz.h + 1, vdz.w + 1, c.dtype, c.device, (id(self), "phases"))
            self._conv(dz, self.phase, 4 * self.cin, 2, 1, 1, t)
            ts = [R.view_of(t[:, ph * self.cin:(ph + 1) * self.cin]) for ph in range(4)]  # raw pointers: `t` outlives the launch below
            vdx = R.view_of(dx)
            L.check(lib.upa_interleave2x(ts[0].ptr, ts[1].ptr, ts[2].ptr, ts[3].ptr, vdz.n, vdz.h + 1, vdz.w + 1, self.cin, ts[0].ld,
                                         vdx.ptr, vdx.h, vdx.w, vdx.ld, int(accumulate), vdx.dtype, st), "interleave2x")
            return
        src = dz
        if self.s == 2:  # other stride-2 shapes: zero-insert dz, then a stride-1 correlation with the flipped weights
            up = _new(vx.n, self.cout, vx.h, vx.w, c.dtype, c.device, (id(self), "dz_up"))
            vu = R.view_of(up)
            L.check(lib.upa_dilate2x(vdz.ptr, vdz.n, vdz.h, vdz.w, vdz.c, vdz.ld, vu.ptr, vu.h, vu.w, vu.ld, vdz.dtype, st),
                    "dilate2x")
            src = up
        self._conv(src, self.wpt, self.cin, self.k, 1, self.k - 1 - self.p, dx, residual=dx if accumulate else None)


class DWConvT:
    """Train-mode forward/backward of one DWConv (conv.py:411-425: depthwise 3x3, stride 1, pad 1 + BatchNorm2d + SiLU | none) - the class
    branch of the non-legacy Detect head (head.py:98-110).  The `ConvT` surface; the weight stays the module's (C, 1, 3, 3) f32 master
    weight, so there is nothing to pack.
      fused (default): upa_dwconv2d_bn_act_fwd / upa_dwconv_bn_act_bwd - the statistics come out of the convolution's workgroups and dz
                       lives in LDS only;
      composed:        upa_dwconv2d_train_fwd, upa_bn_stats, upa_bn_finalize, upa_bn_act_fwd / upa_bn_act_bwd (dz stored), upa_dwconv2d_bwd.
    A fused entry that answers UPA_EUNSUPPORTED falls through to the composed form.  All workspaces follow the context's per-stream
    selection (`ctx.ws`, `_dw_ws`): the small Detect levels run on the level stream beside level 0."""

    fused = True  # (False: the composed form.  The A/B of tools/bench_yolo11_train.py, DESIGN section 6: 9.60 against 9.86 ms per step)

    @staticmethod
    def check(conv: nn.Conv2d, bn, act_code: int, name: str, nc=None):
        """The refusals, from the module alone (`DetectionTrainer` runs them before anything touches the device)."""
        c = conv.in_channels
        if not (conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
                and conv.groups == c == conv.out_channels and conv.bias is None and bn is not None):
            raise L.UpaError(f"{name}: training supports a depthwise conv with k 3, stride 1, pad 1, groups = cin = cout + BatchNorm only "
                             f"(got k={tuple(conv.kernel_size)} s={tuple(conv.stride)} cin={c} cout={conv.out_channels} "
                             f"groups={conv.groups})")
        if c % 8 != 0:
            why = "" if nc is None else f" (the head's class-branch width is c3 = max(ch[0], min(nc, 100)) with nc = {nc})"
            raise L.UpaError(f"{name}: the depthwise training kernels take channel counts that are multiples of 8, got {c}{why}")
        if act_code not in (L.ACT_NONE, L.ACT_SILU):
            raise L.UpaError(f"{name}: training supports SiLU or no activation behind a depthwise conv")

    def __init__(self, ctx: _Ctx, conv: nn.Conv2d, bn, act_code: int, name: str, nc=None):
        self.check(conv, bn, act_code, name, nc)
        c = conv.in_channels
        self.ctx, self.conv, self.bn, self.act, self.name = ctx, conv, bn, act_code, name
        self.k, self.s, self.p = 3, 1, 1
        self.cin = self.cout = c
        self.mean = torch.empty(c, dtype=torch.float32, device=ctx.device)
        self.var = torch.empty(c, dtype=torch.float32, device=ctx.device)
        self.x = self.z = None

    def convs(self):
        return [self]

    # the trainer's weight-repack hooks: the kernels read the master weight
    def pack(self):
        pass

    def pack_descs(self):
        return []

    def pack_phase_weights(self):
        pass

    def _dw_ws(self, nbytes):
        """`nbytes` of workspace for a launch on the CURRENT stream: one buffer per size and per stream selection of the context."""
        c = self.ctx
        return R.alloc_plain((max(int(nbytes), 16),), torch.uint8, c.device, ("dw_ws", c._ws_sel))

    def forward(self, x, out=None):
        c, lib = self.ctx, L.lib()
        n, ch, h, w = x.shape
        st = _s(c.device)
        self.x = x
        z = _new(n, ch, h, w, c.dtype, c.device, (id(self), "z"))
        y = out if out is not None else _new(n, ch, h, w, c.dtype, c.device, (id(self), "y"))
        vx, vz, vy = R.view_of(x), R.view_of(z), R.view_of(y)
        bn, wt = self.bn, self.conv.weight
        self.z = z
        if self.fused:
            ws = self._dw_ws(lib.upa_dwconv2d_bn_act_fwd_workspace_bytes(n, h, w, ch))
            rc = lib.upa_dwconv2d_bn_act_fwd(vx.ptr, n, h, w, ch, vx.ld, wt.data_ptr(), vz.ptr, vz.ld, ConvT._momentum(bn),
                                             self.mean.data_ptr(), self.var.data_ptr(), bn.running_mean.data_ptr(),
                                             bn.running_var.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps), self.act,
                                             vy.ptr, vy.ld, ws.data_ptr(), ws.numel(), vx.dtype, st)
            if rc != L.UPA_EUNSUPPORTED:
                L.check(rc, f"dwconv2d_bn_act_fwd[{self.name}]")
                return y
        npix = n * h * w
        L.check(lib.upa_dwconv2d_train_fwd(vx.ptr, n, h, w, ch, vx.ld, wt.data_ptr(), vz.ptr, vz.ld, vx.dtype, st),
                f"dwconv2d_train_fwd[{self.name}]")
        L.check(lib.upa_bn_stats(vz.ptr, npix, ch, vz.ld, c.ws.data_ptr(), vz.dtype, st), f"bn_stats[{self.name}]")
        L.check(lib.upa_bn_finalize(c.ws.data_ptr(), npix, ch, ConvT._momentum(bn), self.mean.data_ptr(), self.var.data_ptr(),
                                    bn.running_mean.data_ptr(), bn.running_var.data_ptr(), st), f"bn_finalize[{self.name}]")
        L.check(lib.upa_bn_act_fwd(vz.ptr, npix, ch, vz.ld, self.mean.data_ptr(), self.var.data_ptr(), bn.weight.data_ptr(),
                                   bn.bias.data_ptr(), float(bn.eps), self.act, vy.ptr, vy.ld, None, 0, vz.dtype, st),
                f"bn_act_fwd[{self.name}]")
        return y

    def backward(self, dy, dx=None, accumulate=False):
        c, lib = self.ctx, L.lib()
        st = _s(c.device)
        vx, vz, vdy = R.view_of(self.x), R.view_of(self.z), R.view_of(dy)
        n, h, w, ch = vz.n, vz.h, vz.w, vz.c
        vdx = None if dx is None else R.view_of(dx)
        bn, wt = self.bn, self.conv.weight
        if self.fused:
            ws = self._dw_ws(lib.upa_dwconv_bn_act_bwd_workspace_bytes(n, h, w, ch))
            rc = lib.upa_dwconv_bn_act_bwd(vx.ptr, n, h, w, ch, vx.ld, vz.ptr, vdy.ptr, vz.ld, vdy.ld, self.mean.data_ptr(),
                                           self.var.data_ptr(), bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps), self.act,
                                           bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(), c.ws.data_ptr(), wt.data_ptr(),
                                           wt.grad.data_ptr(), 1, None if dx is None else vdx.ptr, 0 if dx is None else vdx.ld,
                                           int(accumulate), ws.data_ptr(), ws.numel(), vz.dtype, st)
            if rc != L.UPA_EUNSUPPORTED:
                L.check(rc, f"dwconv_bn_act_bwd[{self.name}]")
                return
        npix = n * h * w
        dz = _new(n, ch, h, w, c.dtype, c.device, (id(self), "dz"))
        vdz = R.view_of(dz)
        L.check(lib.upa_bn_act_bwd(vz.ptr, vdy.ptr, npix, ch, vz.ld, vdy.ld, self.mean.data_ptr(), self.var.data_ptr(),
                                   bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps), self.act, vdz.ptr, vdz.ld,
                                   bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(), 1, c.ws.data_ptr(), vz.dtype, st),
                f"bn_act_bwd[{self.name}]")
        ws = self._dw_ws(lib.upa_dwconv2d_bwd_workspace_bytes(ch))
        L.check(lib.upa_dwconv2d_bwd(vx.ptr, vdz.ptr, n, h, w, ch, vx.ld, vdz.ld, wt.data_ptr(), None if dx is None else vdx.ptr,
                                     0 if dx is None else vdx.ld, int(accumulate), wt.grad.data_ptr(), 1, ws.data_ptr(), ws.numel(),
                                     vz.dtype, st), f"dwconv2d_bwd[{self.name}]")


class _Seq:
    """Helpers shared by the composite layers."""

    def __init__(self, ctx):
        self.ctx = ctx


class BottleneckT(_Seq):
    def __init__(self, ctx, m: B.Bottleneck, name):
        super().__init__(ctx)
        self.cv1 = ConvT(ctx, m.cv1.conv, m.cv1.bn, m.cv1._act_code(), name + ".cv1")
        self.cv2 = ConvT(ctx, m.cv2.conv, m.cv2.bn, m.cv2._act_code(), name + ".cv2")
        self.add = m.add

    def convs(self):
        return [self.cv1, self.cv2]

    def forward(self, x, out=None):
        t = self.cv1.forward(x)
        return self.cv2.forward(t, out=out, residual=x if self.add else None)

    def backward(self, dy, dx, accumulate):
        c = self.ctx
        vt = R.view_of(self.cv2.x)
        dt = _new(vt.n, vt.c, vt.h, vt.w, c.dtype, c.device, (id(self), "dt"))
        self.cv2.backward(dy, dt, False)
        self.cv1.backward(dt, dx, accumulate)
        if self.add:  # y = x + f(x): the shortcut passes dy straight through
            add_into(c, dy, dx)


def add_into(ctx, src, dst):
    """dst += src (NHWC views)."""
    vs, vd = R.view_of(src), R.view_of(dst)
    L.check(L.lib().upa_add_view(vd.ptr, vd.ld, vs.ptr, vs.ld, vd.ptr, vd.ld, vd.n, vd.h, vd.w, vd.c, vd.dtype, _s(ctx.device)),
            "add_view")


def copy_into(ctx, src, dst):
    vs, vd = R.view_of(src), R.view_of(dst)
    L.check(L.lib().upa_copy_view(vs.ptr, vs.n, vs.h, vs.w, vs.c, vs.ld, vd.ptr, vd.ld, vs.dtype, _s(ctx.device)), "copy_view")


class C2fT(_Seq):
    def __init__(self, ctx, m: B.C2f, name):
        super().__init__(ctx)
        self.c = m.c
        self.cv1 = ConvT(ctx, m.cv1.conv, m.cv1.bn, m.cv1._act_code(), name + ".cv1")
        self.cv2 = ConvT(ctx, m.cv2.conv, m.cv2.bn, m.cv2._act_code(), name + ".cv2")
        self.m = [BottleneckT(ctx, b, f"{name}.m.{i}") for i, b in enumerate(m.m)]

    def convs(self):
        return [self.cv1, self.cv2] + [cv for b in self.m for cv in b.convs()]

    def forward(self, x, out=None):
        c, k = self.ctx, self.c
        n, _, h, w = x.shape
        cat = _new(n, (2 + len(self.m)) * k, h, w, c.dtype, c.device, (id(self), "cat"))
        self.cv1.forward(x, out=cat[:, :2 * k])
        for i, b in enumerate(self.m):
            b.forward(cat[:, (1 + i) * k:(2 + i) * k], out=cat[:, (2 + i) * k:(3 + i) * k])
        self.cat = cat
        return self.cv2.forward(cat, out=out)

    def backward(self, dy, dx, accumulate):
        c, k = self.ctx, self.c
        n, ct, h, w = self.cat.shape
        g = _new(n, ct, h, w, c.dtype, c.device, (id(self), "gcat"))
        self.cv2.backward(dy, g, False)
        for i in reversed(range(len(self.m))):
            self.m[i].backward(g[:, (2 + i) * k:(3 + i) * k], g[:, (1 + i) * k:(2 + i) * k], True)
        self.cv1.backward(g[:, :2 * k], dx, accumulate)


class SPPFT(_Seq):
    def __init__(self, ctx, m: B.SPPF, name):
        super().__init__(ctx)
        self.cv1 = ConvT(ctx, m.cv1.conv, m.cv1.bn, m.cv1._act_code(), name + ".cv1")
        self.cv2 = ConvT(ctx, m.cv2.conv, m.cv2.bn, m.cv2._act_code(), name + ".cv2")
        self.k = m.m.kernel_size if isinstance(m.m.kernel_size, int) else m.m.kernel_size[0]

    def convs(self):
        return [self.cv1, self.cv2]

    def forward(self, x, out=None):
        c = self.ctx
        n, _, h, w = x.shape
        cm = self.cv1.cout
        cat = _new(n, 4 * cm, h, w, c.dtype, c.device, (id(self), "cat"))
        self.cv1.forward(x, out=cat[:, :cm])
        if self.k == 5:  # the three chained MaxPool2d(5, 1, 2) (block.py:402-406) as one launch (5 / 9 / 13 windows)
            v = [R.view_of(cat[:, i * cm:(i + 1) * cm]) for i in range(4)]
            L.check(L.lib().upa_sppf_pool3(v[0].ptr, v[0].n, v[0].h, v[0].w, v[0].c, v[0].ld, v[1].ptr, v[2].ptr, v[3].ptr, v[0].ld,
                                           v[0].dtype, _s(c.device)), "sppf_pool3")
        else:
            for i in range(3):
                vs, vd = R.view_of(cat[:, i * cm:(i + 1) * cm]), R.view_of(cat[:, (i + 1) * cm:(i + 2) * cm])
                L.check(L.lib().upa_maxpool2d(vs.ptr, vs.n, vs.h, vs.w, vs.c, vs.ld, vd.ptr, vd.h, vd.w, vd.ld, self.k, 1,
                                              self.k // 2, 0, vs.dtype, _s(c.device)), "maxpool2d")
        self.cat = cat
        return self.cv2.forward(cat, out=out)

    def backward(self, dy, dx, accumulate):
        c = self.ctx
        n, ct, h, w = self.cat.shape
        cm = ct // 4
        g = _new(n, ct, h, w, c.dtype, c.device, (id(self), "gcat"))
        self.cv2.backward(dy, g, False)
        for i in (2, 1, 0):
            vx, vdy, vdx = R.view_of(self.cat[:, i * cm:(i + 1) * cm]), R.view_of(g[:, (i + 1) * cm:(i + 2) * cm]), \
                R.view_of(g[:, i * cm:(i + 1) * cm])
            nws = L.lib().upa_maxpool2d_bwd_workspace_bytes(vx.n, vx.h, vx.w, vx.c, self.k, 1, self.k // 2)
            ws = R.alloc_plain((nws,), torch.uint8, c.device, (id(self), "argmax"))
            L.check(L.lib().upa_maxpool2d_bwd(vx.ptr, vdy.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, vdy.ld, self.k, 1, self.k // 2,
                                              vdx.ptr, vdx.ld, 1, vx.dtype, ws.data_ptr(), nws, _s(c.device)), "maxpool2d_bwd")
        self.cv1.backward(g[:, :cm], dx, accumulate)


class C3T(_Seq):
    """Train-mode C3 / C3k (block.py:237-262, :1510-1530): cv3(cat(m(cv1(x)), cv2(x))).  cv2 and the last inner Bottleneck write their
    halves of one concat buffer; the gradient of the buffer is sliced the same way."""

    def __init__(self, ctx, m: B.C3, name):
        super().__init__(ctx)
        self.cv1 = ConvT(ctx, m.cv1.conv, m.cv1.bn, m.cv1._act_code(), name + ".cv1")
        self.cv2 = ConvT(ctx, m.cv2.conv, m.cv2.bn, m.cv2._act_code(), name + ".cv2")
        self.cv3 = ConvT(ctx, m.cv3.conv, m.cv3.bn, m.cv3._act_code(), name + ".cv3")
        self.c_ = self.cv1.cout
        self.m = [self._inner(ctx, b, f"{name}.m.{i}") for i, b in enumerate(m.m)]

    def _inner(self, ctx, b, name):
        if not isinstance(b, B.Bottleneck):
            raise L.UpaError(f"{name}: {type(b).__name__} inside a C3 has no training path on HIP")
        return BottleneckT(ctx, b, name)

    def convs(self):
        return [self.cv1, self.cv2, self.cv3] + [cv for b in self.m for cv in b.convs()]

    def forward(self, x, out=None):
        c, k = self.ctx, self.c_
        n, _, h, w = x.shape
        cat = _new(n, 2 * k, h, w, c.dtype, c.device, (id(self), "cat"))
        t = self.cv1.forward(x, out=None if self.m else cat[:, :k])
        for i, b in enumerate(self.m):
            t = b.forward(t, out=cat[:, :k] if i == len(self.m) - 1 else None)
        self.cv2.forward(x, out=cat[:, k:])
        self.cat = cat
        return self.cv3.forward(cat, out=out)

    def backward(self, dy, dx, accumulate):
        c, k = self.ctx, self.c_
        n, ct, h, w = self.cat.shape
        g = _new(n, ct, h, w, c.dtype, c.device, (id(self), "gcat"))
        self.cv3.backward(dy, g, False)
        gt = g[:, :k]
        for i in reversed(range(len(self.m))):  # a Bottleneck's dx must not be its dy (the shortcut adds dy after dx is written)
            gp = _new(n, k, h, w, c.dtype, c.device, (id(self), "gm", i))
            self.m[i].backward(gt, gp, False)
            gt = gp
        self.cv1.backward(gt, dx, accumulate)
        self.cv2.backward(g[:, k:], dx, True)


MHSA_HEAD_DIMS = (4, 8, 16, 32, 64)  # the head widths upa_mhsa / upa_mhsa_train_fwd / upa_mhsa_bwd build


class MHSAT(_Seq):
    """Train-mode MHSA (block.py:6020-6062): softmax(q^T k) applied to v, unscaled, (+ BottleneckTransformer's residual in the epilogue).
    forward:  query / key / value = three plain ConvT (bias, no BN) writing the channel slices [q | k | v] of one buffer ->
              upa_mhsa_train_fwd (y, lse).
    backward: upa_mhsa_bwd writes [dq | dk | dv] -> the three convs' backward, their data gradients accumulated into one dx.
    Saved: qkv and lse (D is recomputed by the kernel, so the output is not kept)."""

    def __init__(self, ctx, m: B.MHSA, name):
        super().__init__(ctx)
        if getattr(m, "pos", False):
            raise L.UpaError(f"{name}: MHSA(pos_emb=True) has no training path on HIP")
        self.c, self.heads = m.query.out_channels, int(m.heads)
        self.d = self.c // self.heads
        if self.c % self.heads or self.d not in MHSA_HEAD_DIMS:
            raise L.UpaError(f"{name}: MHSA with {self.c} channels over {self.heads} heads: the attention kernels build head widths "
                             f"{MHSA_HEAD_DIMS}")
        self.qkv = [ConvT(ctx, cv, None, L.ACT_NONE, f"{name}.{tag}") for tag, cv in (("query", m.query), ("key", m.key), ("value", m.value))]
        self.name = name

    def convs(self):
        return list(self.qkv)

    def _rows(self, t):
        """(q, k, v pointers, pitch) of a [q | k | v] buffer."""
        v = R.view_of(t)
        step = self.c * self.ctx.es
        return v.ptr, v.ptr + step, v.ptr + 2 * step, v.ld

    def forward(self, x, out=None, residual=None):
        c, lib = self.ctx, L.lib()
        dev, st = c.device, _s(c.device)
        n, _, h, w = x.shape
        ch = self.c
        qkv = _new(n, 3 * ch, h, w, c.dtype, dev, (id(self), "qkv"))
        for i, cv in enumerate(self.qkv):
            cv.forward(x, out=qkv[:, i * ch:(i + 1) * ch])
        y = out if out is not None else _new(n, ch, h, w, c.dtype, dev, (id(self), "y"))
        lse = R.alloc_plain((n * self.heads * h * w,), torch.float32, dev, (id(self), "lse"))
        vy = R.view_of(y)
        rp, rld = (None, 0)
        if residual is not None:
            vr = R.view_of(residual)
            rp, rld = vr.ptr, vr.ld
        qp, kp, vp, ld = self._rows(qkv)
        L.check(lib.upa_mhsa_train_fwd(qp, kp, vp, ld, n, h * w, self.heads, self.d, 1.0, rp, rld, vy.ptr, vy.ld, lse.data_ptr(), c.code, st),
                f"mhsa_train_fwd[{self.name}]")
        self.qkv_y, self.lse = qkv, lse
        return y

    def backward(self, dy, dx, accumulate):
        c, lib = self.ctx, L.lib()
        dev, st = c.device, _s(c.device)
        n, _, h, w = self.qkv_y.shape
        ch = self.c
        dqkv = _new(n, 3 * ch, h, w, c.dtype, dev, (id(self), "dqkv"))
        nws = lib.upa_mhsa_bwd_workspace_bytes(n, h * w, self.heads)
        ws = R.alloc_plain((nws,), torch.uint8, dev, (id(self), "bwd_ws"))
        qp, kp, vp, ld = self._rows(self.qkv_y)
        dqp, dkp, dvp, ldd = self._rows(dqkv)
        vdy = R.view_of(dy)
        L.check(lib.upa_mhsa_bwd(qp, kp, vp, ld, self.lse.data_ptr(), vdy.ptr, vdy.ld, dqp, dkp, dvp, ldd, n, h * w, self.heads, self.d, 1.0,
                                 ws.data_ptr(), nws, c.code, st), f"mhsa_bwd[{self.name}]")
        for i, cv in enumerate(self.qkv):
            cv.backward(dqkv[:, i * ch:(i + 1) * ch], dx, accumulate or i > 0)


class BottleneckTransformerT(_Seq):
    """Train-mode BottleneckTransformer (block.py:6065-6092): x + MHSA(cv1(x)); the add is the attention kernel's epilogue, its gradient
    goes through `add_into` as in BottleneckT.  `fc1` is not part of the function (`DetectionTrainer._dead_parameters`)."""

    def __init__(self, ctx, m: B.BottleneckTransformer, name):
        super().__init__(ctx)
        cv1 = getattr(m, "cv1", None)
        if not (isinstance(m, B.BottleneckTransformer) and isinstance(cv1, CV.Conv) and len(m.cv2) == 1 and isinstance(m.cv2[0], B.MHSA)
                and cv1.conv.kernel_size == (1, 1) and cv1.conv.stride == (1, 1)):
            raise L.UpaError(f"{name}: {type(m).__name__} outside the BoT3 configuration (1x1 cv1, one MHSA, stride 1) has no training path "
                             "on HIP")
        self.cv1 = ConvT(ctx, cv1.conv, cv1.bn, cv1._act_code(), name + ".cv1")
        self.attn = MHSAT(ctx, m.cv2[0], name + ".cv2.0")
        self.add = bool(m.shortcut)

    def convs(self):
        return [self.cv1] + self.attn.convs()

    def forward(self, x, out=None):
        return self.attn.forward(self.cv1.forward(x), out=out, residual=x if self.add else None)

    def backward(self, dy, dx, accumulate):
        """dx must not be dy's buffer (the shortcut adds dy after dx is written)."""
        c = self.ctx
        vt = R.view_of(self.attn.qkv[0].x)
        dt = _new(vt.n, vt.c, vt.h, vt.w, c.dtype, c.device, (id(self), "dt"))
        self.attn.backward(dy, dt, False)
        self.cv1.backward(dt, dx, accumulate)
        if self.add:
            add_into(c, dy, dx)


class BoT3T(C3T):
    """Train-mode BoT3 (block.py:6095-6109): C3's graph and concat buffer with BottleneckTransformers inside."""

    def _inner(self, ctx, b, name):
        return BottleneckTransformerT(ctx, b, name)


class C3k2T(C2fT):
    """Train-mode C3k2 (block.py:1485-1507): C2f's graph with Bottleneck(c, c, e=0.5) (c3k=False) or C3k(c, c, 2) (c3k=True) inside."""

    def __init__(self, ctx, m: B.C3k2, name):
        _Seq.__init__(self, ctx)
        self.c = m.c
        self.cv1 = ConvT(ctx, m.cv1.conv, m.cv1.bn, m.cv1._act_code(), name + ".cv1")
        self.cv2 = ConvT(ctx, m.cv2.conv, m.cv2.bn, m.cv2._act_code(), name + ".cv2")
        self.m = []
        for i, b in enumerate(m.m):
            if isinstance(b, B.C3):
                self.m.append(C3T(ctx, b, f"{name}.m.{i}"))
            elif isinstance(b, B.Bottleneck):
                self.m.append(BottleneckT(ctx, b, f"{name}.m.{i}"))
            else:
                raise L.UpaError(f"{name}.m.{i}: {type(b).__name__} inside a C3k2 has no training path on HIP")


class AttentionT(_Seq):
    """Train-mode v10_Attention (block.py:1668-1722): proj(softmax(scale q^T k) v + pe(v)) (+ the block's residual).
    forward:  qkv ConvT (no act) -> upa_psa_attention_train_fwd (o, lse) -> pe: upa_dwconv2d_train_fwd on each head's v slice of qkv
              (no gather copy) -> batch statistics -> upa_bn_act_fwd with o as its residual (t = o + bn(pe)) -> proj ConvT.
    backward: proj -> dt; dt is the gradient of BOTH o and pe's BatchNorm output (the sum node, no copy): upa_bn_act_bwd (pe's BN) ->
              upa_psa_attention_bwd writes dqkv -> upa_dwconv2d_bwd accumulates pe's data gradient into the dv slices and pe's weight
              gradient -> qkv ConvT.backward."""

    def __init__(self, ctx, m: B.v10_Attention, name):
        super().__init__(ctx)
        self.heads, self.kd, self.hd, self.scale = m.num_heads, m.key_dim, m.head_dim, float(m.scale)
        if self.kd != 32 or self.hd != 64:
            raise L.UpaError(f"{name}: training supports key_dim 32 / head_dim 64 (every YOLO11 scale), got {self.kd} / {self.hd}")
        pe = m.pe
        if not (pe.conv.groups == pe.conv.in_channels == pe.conv.out_channels and pe.conv.kernel_size == (3, 3) and pe.conv.stride == (1, 1)
                and pe.conv.padding == (1, 1) and pe.conv.dilation == (1, 1) and pe.conv.bias is None and isinstance(pe.act, nn.Identity)):
            raise L.UpaError(f"{name}.pe: training supports a depthwise 3x3, stride 1, pad 1 conv + BatchNorm without activation, got {pe}")
        self.qkv = ConvT(ctx, m.qkv.conv, m.qkv.bn, m.qkv._act_code(), name + ".qkv")
        self.proj = ConvT(ctx, m.proj.conv, m.proj.bn, m.proj._act_code(), name + ".proj")
        self.pe = pe
        self.c = self.heads * self.hd
        dev = ctx.device
        self.pe_mean = torch.empty(self.c, dtype=torch.float32, device=dev)
        self.pe_var = torch.empty(self.c, dtype=torch.float32, device=dev)
        self.dw_ws = torch.empty(L.lib().upa_dwconv2d_bwd_workspace_bytes(self.hd), dtype=torch.uint8, device=dev)

    def convs(self):
        return [self.qkv, self.proj]  # pe's depthwise weight is read in the module's own layout: no MFMA repack

    def _v(self, t, hh):
        """Head hh's v channels of a qkv-shaped tensor."""
        c0 = hh * (2 * self.kd + self.hd) + 2 * self.kd
        return R.view_of(t[:, c0:c0 + self.hd])

    def forward(self, x, out=None, residual=None):
        c, lib = self.ctx, L.lib()
        dev, st = c.device, _s(c.device)
        n, _, h, w = x.shape
        qkv = self.qkv.forward(x)
        o = _new(n, self.c, h, w, c.dtype, dev, (id(self), "o"))
        lse = R.alloc_plain((n * self.heads * h * w,), torch.float32, dev, (id(self), "lse"))
        vq, vo = R.view_of(qkv), R.view_of(o)
        L.check(lib.upa_psa_attention_train_fwd(vq.ptr, vq.ld, n, h, w, self.heads, self.kd, self.hd, self.scale, vo.ptr, vo.ld,
                                                lse.data_ptr(), vq.dtype, st), "psa_attention_train_fwd")
        z = _new(n, self.c, h, w, c.dtype, dev, (id(self), "zpe"))
        wt = self.pe.conv.weight
        for hh in range(self.heads):
            vv, vz = self._v(qkv, hh), R.view_of(z[:, hh * self.hd:(hh + 1) * self.hd])
            L.check(lib.upa_dwconv2d_train_fwd(vv.ptr, n, h, w, self.hd, vv.ld, wt.data_ptr() + hh * self.hd * 9 * 4, vz.ptr, vz.ld,
                                               vq.dtype, st), "dwconv2d_train_fwd")
        bn = self.pe.bn
        vz = R.view_of(z)
        npix = n * h * w
        L.check(lib.upa_bn_stats(vz.ptr, npix, self.c, vz.ld, c.ws.data_ptr(), vz.dtype, st), "bn_stats[pe]")
        L.check(lib.upa_bn_finalize(c.ws.data_ptr(), npix, self.c, ConvT._momentum(bn), self.pe_mean.data_ptr(), self.pe_var.data_ptr(),
                                    bn.running_mean.data_ptr(), bn.running_var.data_ptr(), st), "bn_finalize[pe]")
        t = _new(n, self.c, h, w, c.dtype, dev, (id(self), "t"))
        vt = R.view_of(t)
        L.check(lib.upa_bn_act_fwd(vz.ptr, npix, self.c, vz.ld, self.pe_mean.data_ptr(), self.pe_var.data_ptr(), bn.weight.data_ptr(),
                                   bn.bias.data_ptr(), float(bn.eps), L.ACT_NONE, vt.ptr, vt.ld, vo.ptr, vo.ld, vz.dtype, st),
                "bn_act_fwd[pe]")
        self.qkv_y, self.o, self.lse, self.z = qkv, o, lse, z
        return self.proj.forward(t, out=out, residual=residual)

    def backward(self, dy, dx, accumulate):
        c, lib = self.ctx, L.lib()
        dev, st = c.device, _s(c.device)
        n, _, h, w = self.o.shape
        npix = n * h * w
        dt = _new(n, self.c, h, w, c.dtype, dev, (id(self), "dt"))
        self.proj.backward(dy, dt, False)
        bn = self.pe.bn
        dz = _new(n, self.c, h, w, c.dtype, dev, (id(self), "dzpe"))
        vz, vdt, vdz = R.view_of(self.z), R.view_of(dt), R.view_of(dz)
        L.check(lib.upa_bn_act_bwd(vz.ptr, vdt.ptr, npix, self.c, vz.ld, vdt.ld, self.pe_mean.data_ptr(), self.pe_var.data_ptr(),
                                   bn.weight.data_ptr(), bn.bias.data_ptr(), float(bn.eps), L.ACT_NONE, vdz.ptr, vdz.ld,
                                   bn.weight.grad.data_ptr(), bn.bias.grad.data_ptr(), 1, c.ws.data_ptr(), vz.dtype, st), "bn_act_bwd[pe]")
        qkv = self.qkv_y
        dqkv = _new(n, qkv.shape[1], h, w, c.dtype, dev, (id(self), "dqkv"))
        vq, vo, vdq = R.view_of(qkv), R.view_of(self.o), R.view_of(dqkv)
        L.check(lib.upa_psa_attention_bwd(vq.ptr, vq.ld, vo.ptr, vo.ld, self.lse.data_ptr(), vdt.ptr, vdt.ld, vdq.ptr, vdq.ld, n, h, w,
                                          self.heads, self.kd, self.hd, self.scale, None, 0, vq.dtype, st), "psa_attention_bwd")
        wt = self.pe.conv.weight
        for hh in range(self.heads):
            vv, vg, vdv = self._v(qkv, hh), R.view_of(dz[:, hh * self.hd:(hh + 1) * self.hd]), self._v(dqkv, hh)
            off = hh * self.hd * 9 * 4
            L.check(lib.upa_dwconv2d_bwd(vv.ptr, vg.ptr, n, h, w, self.hd, vv.ld, vg.ld, wt.data_ptr() + off, vdv.ptr, vdv.ld, 1,
                                         wt.grad.data_ptr() + off, 1, self.dw_ws.data_ptr(), self.dw_ws.numel(), vq.dtype, st),
                    "dwconv2d_bwd[pe]")
        self.qkv.backward(dqkv, dx, accumulate)


class PSABlockT(_Seq):
    """Train-mode PSABlock (block.py:1724-1766): u = x + attn(x), y = u + ffn(u); both adds in the last conv's epilogue, their
    gradients through `add_into` as in BottleneckT."""

    def __init__(self, ctx, m: B.PSABlock, name):
        super().__init__(ctx)
        self.attn = AttentionT(ctx, m.attn, name + ".attn")
        self.ffn = [ConvT(ctx, f.conv, f.bn, f._act_code(), f"{name}.ffn.{i}") for i, f in enumerate(m.ffn)]
        self.add = m.add

    def convs(self):
        return self.attn.convs() + self.ffn

    def forward(self, x, out=None):
        c = self.ctx
        n, ch, h, w = x.shape
        u = _new(n, ch, h, w, c.dtype, c.device, (id(self), "u"))
        self.attn.forward(x, out=u, residual=x if self.add else None)
        return self.ffn[1].forward(self.ffn[0].forward(u), out=out, residual=u if self.add else None)

    def backward(self, dy, dx, accumulate):
        """dx may be dy's own buffer when not accumulating: dy is last read before the attention's qkv conv writes dx."""
        c = self.ctx
        vf = R.view_of(self.ffn[1].x)
        df = _new(vf.n, vf.c, vf.h, vf.w, c.dtype, c.device, (id(self), "df"))
        n, ch, h, w = dy.shape
        du = _new(n, ch, h, w, c.dtype, c.device, (id(self), "du"))
        self.ffn[1].backward(dy, df, False)
        self.ffn[0].backward(df, du, False)
        if self.add:
            add_into(c, dy, du)
        self.attn.backward(du, dx, accumulate)
        if self.add:
            add_into(c, du, dx)


class C2PSAT(_Seq):
    """Train-mode C2PSA (block.py:1829-1881): cv1 -> [a | b], b through the PSABlocks, cv2(cat(a, b')).  In train mode b must survive
    (the first block's qkv conv needs it for its weight gradient), so cv2 reads a second 2c buffer: the last block writes its b half,
    a is copied.  The gradient of that buffer is cv1's output gradient: its a half as it is, its b half rewritten by the blocks."""

    def __init__(self, ctx, m: B.C2PSA, name):
        super().__init__(ctx)
        self.c = m.c
        self.cv1 = ConvT(ctx, m.cv1.conv, m.cv1.bn, m.cv1._act_code(), name + ".cv1")
        self.cv2 = ConvT(ctx, m.cv2.conv, m.cv2.bn, m.cv2._act_code(), name + ".cv2")
        self.m = [PSABlockT(ctx, b, f"{name}.m.{i}") for i, b in enumerate(m.m)]
        if not self.m:
            raise L.UpaError(f"{name}: a C2PSA without PSABlocks has no training path on HIP")

    def convs(self):
        return [self.cv1, self.cv2] + [cv for b in self.m for cv in b.convs()]

    def forward(self, x, out=None):
        c, k = self.ctx, self.c
        n, _, h, w = x.shape
        ab = self.cv1.forward(x)
        cat = _new(n, 2 * k, h, w, c.dtype, c.device, (id(self), "cat"))
        copy_into(c, ab[:, :k], cat[:, :k])
        b = ab[:, k:]
        for i, blk in enumerate(self.m):
            b = blk.forward(b, out=cat[:, k:] if i == len(self.m) - 1 else None)
        return self.cv2.forward(cat, out=out)

    def backward(self, dy, dx, accumulate):
        c, k = self.ctx, self.c
        vc = R.view_of(self.cv2.x)
        g = _new(vc.n, 2 * k, vc.h, vc.w, c.dtype, c.device, (id(self), "gcat"))
        self.cv2.backward(dy, g, False)
        gcur = g[:, k:]
        for i in reversed(range(len(self.m))):  # the first block writes b's gradient back into g's b half (PSABlockT.backward: dx may be dy)
            gp = g[:, k:] if i == 0 else _new(vc.n, k, vc.h, vc.w, c.dtype, c.device, (id(self), "gb", i))
            self.m[i].backward(gcur, gp, False)
            gcur = gp
        self.cv1.backward(g, dx, accumulate)


class _Node:
    """One row of the model YAML inside the training graph."""

    def __init__(self, i, f, kind, op):
        self.i, self.f, self.kind, self.op = i, f, kind, op
        self.y = None       # forward output
        self.g = None       # gradient buffer of the output
        self.g_ready = False


class GradScaler:
    """`torch.amp.GradScaler("cuda", enabled=amp)` of the reference (engine/trainer.py:301-302; used at :429 scale(loss).backward(),
    :676 unscale_, :678 step, :679 update, :593 / :824-825 state_dict) with its state ON THE DEVICE: {scale, growth tracker, found_inf}.
    The loss kernels multiply their gradients by the scale (upa_detection_loss_scaled), the optimizer kernel divides it out again, clips
    on the unscaled norm and skips an overflowing step (upa_sgd_nesterov_ema_scaled), `upa_grad_scaler_update` adjusts the scale - the
    host never reads it, so a scaled step stays one hipGraph.  Defaults = torch's (init 2**16, growth 2, backoff 0.5, interval 2000).
    bf16 has f32's exponent range and needs no loss scaling; the scaler exists because the reference's AMP loop has one
    (`DetectionTrainer(..., amp_scaler=True)`)."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self.enabled = bool(enabled)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.state = torch.tensor([float(init_scale), 0.0, 0.0, 0.0], dtype=torch.float32, device=device)

    def ptr(self):
        return self.state.data_ptr() if self.enabled else None

    def update(self, sumsq, stream):
        if self.enabled:
            L.check(L.lib().upa_grad_scaler_update(self.state.data_ptr(), sumsq.data_ptr(), self.growth_factor, self.backoff_factor,
                                                   self.growth_interval, stream), "grad_scaler_update")

    def get_scale(self) -> float:  # (host synchronisation: logging / tests only)
        return float(self.state[0].item()) if self.enabled else 1.0

    def carried_scale(self, after_update: bool) -> float:
        """The scale the gradients in the flat buffer were multiplied by: the current one before `update()` ran for them, the one
        `update()` saved (state[3]) after - on a step where the scale grew or backed off the two differ by that factor."""
        if not self.enabled:
            return 1.0
        return float(self.state[3 if after_update else 0].item())

    def found_inf(self) -> bool:
        return bool(self.state[2].item() != 0.0) if self.enabled else False

    def state_dict(self):
        if not self.enabled:
            return {}
        st = self.state.cpu()
        return {"scale": float(st[0]), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(st[1])}

    def load_state_dict(self, sd):
        if not self.enabled or not sd:
            return
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self.state.copy_(torch.tensor([float(sd["scale"]), float(sd["_growth_tracker"]), 0.0, 0.0]))


def resolve_optimizer(name, iterations, nc):
    """`build_optimizer`'s choice (engine/trainer.py:891-950) as (name, hyp overrides, auto?): the name is case-insensitive; "auto" takes
    SGD(lr 0.01, momentum 0.9) for more than 10 000 iterations and AdamW(lr round(0.002 * 5 / (4 + nc), 6), beta1 0.9) otherwise,
    whatever `hyp` says, and forces warmup_bias_lr = 0 (the third element: `set_schedule` reads it)."""
    known = {x.lower(): x for x in OPTIMIZERS}
    got = known.get(str(name).lower())
    if got is None:
        raise L.UpaError(f"optimizer={name!r} has no fused step on HIP: supported are {', '.join(OPTIMIZERS)} (Adamax, NAdam, RAdam and "
                         "RMSProp of the reference's list are not built)")
    if got != "auto":
        return got, {}, False
    if iterations is None:
        raise L.UpaError("optimizer='auto' needs iterations= (the number of optimizer iterations of the run: auto picks SGD above 10000, "
                         "AdamW otherwise); or name one of SGD, Adam, AdamW")
    if iterations > 10000:
        return "SGD", dict(lr=0.01, momentum=0.9), True
    return "AdamW", dict(lr=round(0.002 * 5 / (4 + nc), 6), momentum=0.9), True


def _head_nc(model) -> int:
    """Number of classes of the model's head (the reference's `self.data["nc"]`)."""
    tail = model.model[-1] if hasattr(model, "model") and len(model.model) else None
    if isinstance(tail, H.Classify):
        return int(tail.linear.out_features)
    if tail is not None and hasattr(tail, "nc"):
        return int(tail.nc)
    raise L.UpaError(f"optimizer='auto' reads the number of classes from the model's head, got {type(tail).__name__}")


class DetectionTrainer:
    """One-process-per-GPU trainer for a DetectionModel (reference: engine/trainer.py BaseTrainer._do_train inner loop).
    `optimizer`: "SGD" (default: SGD-Nesterov), "Adam", "AdamW" (lr and beta1 = `momentum` from `hyp`, plus `beta2`, `adam_eps`) or
    "auto" with `iterations` (`resolve_optimizer`); `optimizer_name` is the resolved one."""

    _segment_ok = False  # (SegmentationTrainer: True)

    def __init__(self, model, dtype=torch.bfloat16, hyp=None, device=None, world_size=1, ema=True, wgrad_streams: int = 1,
                 amp_scaler: bool = False, optimizer: str = "SGD", iterations=None, yolo11: bool = False):
        self.optimizer_name, opt_hyp, self._auto_optimizer = resolve_optimizer(
            optimizer, iterations, _head_nc(model) if str(optimizer).lower() == "auto" and iterations is not None else 0)
        # the non-legacy Detect head (YOLO11: depthwise class branch, `DWConvT`) trains on request only: `yolo11=True`
        if not self._segment_ok and any(isinstance(m, H.Segment) for m in model.modules()):
            raise L.UpaError("segmentation models (Segment head) have no training path on HIP in DetectionTrainer (v8DetectionLoss only): "
                             "train them with SegmentationTrainer")
        for m in model.modules():
            if isinstance(m, H.Detect) and not m.legacy_cls:
                if not yolo11:
                    raise L.UpaError(f"{type(m).__name__} (YOLO11, non-legacy head with a depthwise class branch) has no training path "
                                     "on HIP unless it is asked for: pass yolo11=True to train a YOLO11 detection model")
                for i, seq in enumerate(m.cv3):  # the depthwise convs' refusals, before anything touches the device
                    for j in (0, 1):
                        dw = seq[j][0]
                        DWConvT.check(dw.conv, getattr(dw, "bn", None), dw._act_code(), f"model.{getattr(m, 'i', '?')}.cv3.{i}.{j}.0", nc=m.nc)
        self.model = model
        self.hyp = dict(HYP, **(hyp or {}))
        self.hyp.update(opt_hyp)  # auto ignores lr0 and momentum of the arguments, as the reference does
        self.adam = self.optimizer_name in ("Adam", "AdamW")
        self.device = torch.device(device or "cuda:0")
        self.dtype = dtype
        self.world_size = world_size
        self.ctx = _Ctx(self.device, dtype, wgrad_streams)
        self.scaler = GradScaler(self.device, enabled=amp_scaler)  # trainer.py:301-302
        self.pool = R.BufferPool()
        self.updates = 0
        self.first_step = True
        self._scaler_updated = False
        self._graphs = None
        self._capturing = False
        self._issue_buckets = False
        self._imgsz = None
        self.gt_d = self.ngt_d = None
        self.schedule = None      # set_schedule(): warm-up interpolation + gradient accumulation of the reference's loop
        self.ni = 0               # iteration counter (the reference's `ni = i + nb * epoch`)
        self.last_opt_step = -1   # trainer.py:386
        self.max_gt = MAX_GT  # rows per image of the padded gt tensor (the reference pads to counts.max(), loss.py:445-461)
        model.to(self.device)
        self._flatten_parameters(ema)
        self._build_graph()

    # ---- parameters ---------------------------------------------------------------------------------------------------
    def _flatten_parameters(self, ema):
        """Flat f32 buffers [biases | decayed weights | norm weights] with model.parameters() viewing into them."""
        from ..parallel import flat_parameter_layout
        layout, meta = flat_parameter_layout(self.model)
        dead = self._dead_parameters()
        if dead:
            # parameters outside the function get no place in the three optimizer groups: they are laid out BEHIND the last group, where no
            # optimizer launch, no gradient norm and no all-reduce reaches (all of them end at the last group's end).  The live parameters
            # keep their relative order, so a model without dead parameters has exactly the layout it always had.
            live = [row for row in meta if id(row[3]) not in dead]
            gone = [row for row in meta if id(row[3]) in dead]
            layout2, meta2, off = [], [], 0
            for start, n, wd in layout:
                rows = [r for r in meta if start <= r[1] < start + n and id(r[3]) not in dead]
                g0 = off
                for name, _, cnt, p in rows:
                    meta2.append((name, off, cnt, p))
                    off += cnt
                layout2.append((g0, off - g0, wd))
            self._dead_meta = []
            for name, _, cnt, p in gone:
                self._dead_meta.append((name, off, cnt, p))
                off += cnt
            assert len(meta2) == len(live)
            layout, meta = layout2, meta2
            total = off
        else:
            self._dead_meta = []
            total = sum(n for _, n, _ in layout)
        dev = self.device
        self.P = torch.empty(total, dtype=torch.float32, device=dev)
        self.G = torch.zeros(total, dtype=torch.float32, device=dev)
        self.M = torch.zeros(total, dtype=torch.float32, device=dev)  # SGD: momentum buffer; Adam / AdamW: exp_avg
        self.V = self.opt_step_dev = None
        if self.adam:  # exp_avg_sq and the step count (torch's state["step"]), device-side: see upa_adam_step_advance
            self.V = torch.zeros(total, dtype=torch.float32, device=dev)
            self.opt_step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        for _name, off, n, p in list(meta) + self._dead_meta:
            self.P[off:off + n].copy_(p.detach().reshape(-1))  # plumbing: one-time gather of the initial weights
            p.data = self.P[off:off + n].view(p.shape)
            p.grad = self.G[off:off + n].view(p.shape)
        self.groups = [(start, n, self.hyp["weight_decay"] if wd else 0.0) for start, n, wd in layout]
        self._param_meta = [(name, off, n) for name, off, n, _ in meta]  # flat order: gradient buckets are cut by layer from it
        self.E = self.P.clone() if ema else None  # ModelEMA copy of the parameters
        bufs = [b for b in self.model.buffers() if b.dtype.is_floating_point]
        nb = sum(b.numel() for b in bufs)
        self.RB = torch.empty(max(nb, 1), dtype=torch.float32, device=dev)
        off = 0
        for b in bufs:
            n = b.numel()
            self.RB[off:off + n].copy_(b.detach().reshape(-1))
            b.data = self.RB[off:off + n].view(b.shape)
            off += n
        self.nbuf = nb
        self.ERB = self.RB.clone() if ema else None
        self.sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        self.sumsq_ws = torch.zeros(L.lib().upa_sumsq_workspace_bytes() // 8, dtype=torch.float64, device=dev)
        self.ema_d_dev = torch.zeros(1, dtype=torch.float32, device=dev)

    def _dead_parameters(self):
        """ids of the parameters the model's forward never reads: `BottleneckTransformer.fc1` (block.py:6088, kept for the state_dict).
        Under autograd their `.grad` stays None and the reference's optimizer skips them - no weight decay, no momentum, and the EMA copy
        stays equal to them.  Here they live behind the optimizer groups of the flat buffers (`_flatten_parameters`), so every step leaves
        them, and their EMA copies, bit-unchanged."""
        return {id(p) for m in self.model.modules() if isinstance(m, B.BottleneckTransformer) for p in m.fc1.parameters()}

    # ---- graph --------------------------------------------------------------------------------------------------------
    def _build_graph(self):
        ctx = self.ctx
        self.nodes = []
        self.convs = []
        self._pack_table, self._pack_n = None, 0
        for m in self.model.model:
            name = f"model.{m.i}"
            tail = self._tail_op(m, name)
            if tail is not None:
                op, kind = tail
            elif isinstance(m, B.C3k2):  # (a C2f subclass: before it)
                op, kind = C3k2T(ctx, m, name), "c2f"
            elif isinstance(m, B.C2PSA):
                op, kind = C2PSAT(ctx, m, name), "c2f"
            elif isinstance(m, B.C2f):
                op, kind = C2fT(ctx, m, name), "c2f"
            elif isinstance(m, B.BoT3):
                op, kind = BoT3T(ctx, m, name), "c3"
            elif isinstance(m, B.C3) and not isinstance(m, B.C3k):  # (C3k: a C3 subclass that only lives inside a C3k2)
                op, kind = C3T(ctx, m, name), "c3"
            elif isinstance(m, B.SPPF):
                op, kind = SPPFT(ctx, m, name), "sppf"
            elif isinstance(m, CV.Conv):
                op, kind = ConvT(ctx, m.conv, m.bn, m._act_code(), name, no_dgrad=(m.i == 0 and m.f == -1)), "conv"
            elif isinstance(m, CV.Concat):
                op, kind = None, "concat"
            elif isinstance(m, RS.Upsample):
                op, kind = None, "upsample"
            else:
                raise L.UpaError(f"{type(m).__name__} (layer {m.i}) has no training path on HIP yet")
            if op is not None:
                self.convs += op.convs() if hasattr(op, "convs") else [op]
            self.nodes.append(_Node(m.i, m.f, kind, op))
        self.detect = self.nodes[-1].op
        self._plan_concats()

    def _tail_op(self, m, name):
        """(op, kind) of the module that ends the graph and owns the loss (`forward(x)`, `loss_backward(labels, batch_size)`), None for
        every other module.  The hook a trainer of another task overrides (`ClassificationTrainer`)."""
        if isinstance(m, H.Detect):
            return DetectT(self.ctx, m, name, self), "detect"
        return None

    def _plan_concats(self):
        """nn.Concat without copies: a layer whose output feeds exactly one Concat writes it straight into its channel slice of the
        Concat's buffer (every kernel takes a pixel stride), and in backward that slice of the Concat's gradient IS the layer's
        gradient buffer when the Concat is the first consumer the reverse walk meets.  {producer index: (concat index, first
        channel, channels, channels of the concat)}."""
        cout = {}
        for nd in self.nodes[:-1]:
            src = (lambda j: j if j != -1 else nd.i - 1)
            if nd.kind == "conv":
                cout[nd.i] = nd.op.cout
            elif nd.kind in ("c2f", "sppf"):
                cout[nd.i] = nd.op.cv2.cout
            elif nd.kind == "c3":
                cout[nd.i] = nd.op.cv3.cout
            elif nd.kind == "upsample":
                cout[nd.i] = cout[src(nd.f)]
            elif nd.kind == "concat":
                cout[nd.i] = sum(cout[src(j)] for j in nd.f)
        self._cat_slot = {}
        for nd in self.nodes[:-1]:
            if nd.kind != "concat":
                continue
            idx = [j if j != -1 else nd.i - 1 for j in nd.f]
            c0 = 0
            for j in idx:
                if j not in self._cat_slot and idx.count(j) == 1 and self.nodes[j].i == j and \
                        self.nodes[j].kind in ("conv", "c2f", "c3", "sppf", "upsample"):
                    self._cat_slot[j] = (nd.i, c0, cout[j], cout[nd.i])
                c0 += cout[j]

    # ---- one step -----------------------------------------------------------------------------------------------------
    def _input_nhwc(self, img):
        """(N,3,H,W) f32 NCHW image batch -> NHWC view padded to one 16-byte channel group (pad channels stay zero)."""
        n, c, h, w = img.shape
        E = self.ctx.E
        zeroed = self.__dict__.setdefault("_img_zeroed", set())
        buf = self.pool.get(("img", n, h, w), (n, h, w, E), self.dtype, self.device)
        if (n, h, w) not in zeroed:
            buf.zero_()  # one-time: the pad channels are never written again
            zeroed.add((n, h, w))
        L.check(L.lib().upa_nchw_to_nhwc(img.data_ptr(), n, c, h, w, buf.data_ptr(), E, self.ctx.code, _s(self.device)),
                "nchw_to_nhwc")
        return buf.permute(0, 3, 1, 2)

    def _pack_weights(self):
        """Repack every conv's master weights into the MFMA fragment layouts (forward, data gradient) - one launch for the
        whole model plus one per stride-2 conv (its four phase kernels).  The descriptor table is built once: the master
        weights are views of the flat parameter buffer and the packed buffers are owned by the layers."""
        for cv in self.convs:
            cv.pack_phase_weights()
        if self._pack_table is None:
            rows = [d for cv in self.convs for d in cv.pack_descs()]
            rows += [d for nd in self.nodes if hasattr(nd.op, "extra_pack_descs") for d in nd.op.extra_pack_descs()]
            t = np.zeros(len(rows), dtype=np.dtype([("w", "<u8"), ("out", "<u8"), ("cout", "<i4"), ("cin", "<i4"), ("k", "<i4"),
                                                    ("dtype", "<i4"), ("tf", "<i4"), ("reserved", "<i4")]))
            for i, r in enumerate(rows):
                t[i] = r + (0,)
            self._pack_table = torch.from_numpy(t.view(np.uint8).copy()).to(self.device)
            self._pack_n = len(rows)
        L.check(L.lib().upa_pack_conv_weights_batched(self._pack_table.data_ptr(), self._pack_n, _s(self.device)), "pack_batched")

    def forward_backward(self, img, labels):
        """img: (N,3,H,W) float32 NCHW on the device; labels: the reference's batch dict (batch_idx, cls, bboxes; `SegmentationTrainer`: masks
        as well).  Fills the flat gradient buffer; returns loss_items on the device ((3,) box, cls, dfl; `SegmentationTrainer`: (4,) box, seg, cls, dfl)."""
        ctx, dev = self.ctx, self.device
        L.require_gpu(img, "train")
        self.model.train()
        self._scaler_updated = False  # the gradients this call produces carry the scaler's CURRENT scale
        if labels is not None:
            # the labels go up BEFORE the forward launches (stream-ordered behind the previous step's loss kernels): packing them on the
            # host overlaps the GPU's work on the previous step instead of standing between this step's forward and its loss
            self._imgsz = (int(img.shape[2]), int(img.shape[3]))
            self._upload_labels(labels, int(img.shape[0]))
            labels = None
        with R.static_buffers(self.pool):
            self._pack_weights()
            x = self._input_nhwc(img.float().contiguous() if img.dtype != torch.float32 else img.contiguous())
            # the stem sees E input channels: 3 real + zero padding (the packed weights are zero there as well)
            ys = []
            for nd in self.nodes:
                xin = x if nd.f == -1 else (ys[nd.f] if isinstance(nd.f, int) else [x if j == -1 else ys[j] for j in nd.f])
                nd.xin = xin
                out = None
                slot = self._cat_slot.get(nd.i)
                if slot is not None:  # this layer's output lives in its slice of the Concat's buffer
                    cat_i, c0, cj, ctot = slot
                    n, _, h, w = xin.shape
                    if nd.kind == "conv":
                        h, w = (h + 2 * nd.op.p - nd.op.k) // nd.op.s + 1, (w + 2 * nd.op.p - nd.op.k) // nd.op.s + 1
                    elif nd.kind == "upsample":
                        h, w = 2 * h, 2 * w
                    out = _new(n, ctot, h, w, ctx.dtype, dev, (id(self.nodes[cat_i]), "y"))[:, c0:c0 + cj]
                if nd.kind in ("conv", "c2f", "c3", "sppf"):
                    y = nd.op.forward(xin, out=out)
                elif nd.kind == "upsample":
                    n, c, h, w = xin.shape
                    y = out if out is not None else _new(n, c, 2 * h, 2 * w, ctx.dtype, dev, (id(nd), "y"))
                    vs, vd = R.view_of(xin), R.view_of(y)
                    L.check(L.lib().upa_upsample2x(vs.ptr, vs.n, vs.h, vs.w, vs.c, vs.ld, vd.ptr, vd.ld, vs.dtype, _s(dev)),
                            "upsample2x")
                elif nd.kind == "concat":
                    n, _, h, w = xin[0].shape
                    y = _new(n, sum(int(t.shape[1]) for t in xin), h, w, ctx.dtype, dev, (id(nd), "y"))
                    c0 = 0
                    for j, t in zip(nd.f, xin):
                        j = j if j != -1 else nd.i - 1
                        if self._cat_slot.get(j, (None,))[0] != nd.i:  # not written in place by its producer
                            copy_into(ctx, t, y[:, c0:c0 + t.shape[1]])
                        c0 += t.shape[1]
                else:  # the tail (Detect; Classify in ClassificationTrainer)
                    y = nd.op.forward(xin)
                nd.y = y
                nd.g = None
                nd.g_ready = False
                x = y
                ys.append(y)
            items = self.detect.loss_backward(labels, img.shape[0])
            self._bucket_hook(self.nodes[-1].i)
            # ---- backward over the layer list in reverse
            for nd in reversed(self.nodes[:-1]):
                if nd.g is None:
                    self._bucket_hook(nd.i)
                    continue  # output unused by the loss
                dy = nd.g
                if nd.kind in ("conv", "c2f", "c3", "sppf"):
                    if nd.i == 0:
                        nd.op.backward(dy, None, False)
                    else:
                        src = self.nodes[nd.f] if nd.f != -1 else self.nodes[nd.i - 1]
                        dx, acc = self._grad_of(src)
                        nd.op.backward(dy, dx, acc)
                elif nd.kind == "upsample":
                    src = self.nodes[nd.f] if nd.f != -1 else self.nodes[nd.i - 1]
                    dx, acc = self._grad_of(src)
                    vdy, vdx = R.view_of(dy), R.view_of(dx)
                    L.check(L.lib().upa_upsample2x_bwd(vdy.ptr, vdx.n, vdx.h, vdx.w, vdx.c, vdy.ld, vdx.ptr, vdx.ld, int(acc),
                                                       vdx.dtype, _s(dev)), "upsample2x_bwd")
                elif nd.kind == "concat":
                    c0 = 0
                    for j in nd.f:
                        src = self.nodes[j] if j != -1 else self.nodes[nd.i - 1]
                        cj = int(src.y.shape[1])
                        if src.g is None:   # the Concat is the first consumer met: its slice IS the gradient buffer, later ones accumulate
                            src.g = dy[:, c0:c0 + cj]
                        else:
                            add_into(ctx, dy[:, c0:c0 + cj], src.g)
                        c0 += cj
                self._bucket_hook(nd.i)
            self._join_wgrad()
        return items

    def _join_wgrad(self):
        ctx = self.ctx
        if ctx.wgrad_streams and ctx.wgrad_pending:
            for side in ctx.wgrad_streams:
                ev = torch.cuda.Event()
                ev.record(side)
                torch.cuda.current_stream(self.device).wait_event(ev)
            ctx.wgrad_pending = False

    def _grad_of(self, node):
        """(gradient buffer of node's output, accumulate?) - the first producer writes, later ones accumulate."""
        if node.g is None:
            n, c, h, w = node.y.shape
            node.g = _new(n, c, h, w, self.ctx.dtype, self.device, (id(node), "g"))
            return node.g, False
        return node.g, True

    def grad_sumsq(self):
        off_end = self.groups[-1][0] + self.groups[-1][1]
        L.check(L.lib().upa_sumsq(self.G.data_ptr(), off_end, self.sumsq.data_ptr(), 0, self.sumsq_ws.data_ptr(),
                                  _s(self.device)), "sumsq")
        return self.sumsq

    # ---- gradient exchange -------------------------------------------------------------------------------------------
    def gradient_buckets(self, target_bytes: int = 16 << 20):
        """Layer spans, last layer first, of at least `target_bytes` of f32 gradients each (DDP's bucket_cap_mb idea; yolov8s:
        three spans of its 44.7 MB), as (first layer of the span, [flat ranges]).  Within each optimizer group the parameters
        lie in layer order, so a span of layers is ONE contiguous range per group.  A span is complete - every gradient kernel
        of its layers enqueued - once the backward walk has passed its first layer."""
        from ..parallel import gradient_bucket_table
        return gradient_bucket_table(self._param_meta, self.groups, target_bytes)

    def enable_overlapped_allreduce(self, target_bytes: int = 16 << 20):
        """Issue the gradient all-reduce per bucket DURING backward on a communication stream (eager steps only: a collective
        cannot sit inside the captured backward graph, so `compile()`d multi-GPU steps keep the single all-reduce between their
        two graphs).  Returns the bucket table [(first layer, [ranges])]."""
        from ..parallel import BucketedAllReduce
        table = self.gradient_buckets(target_bytes)
        self._bucket_first = {first: k for k, (first, _) in enumerate(table)}
        self._buckets = BucketedAllReduce(self.G, [r for _, r in table])
        ntot = self.groups[-1][0] + self.groups[-1][1]
        assert self._buckets.covered() == ntot, "gradient buckets must cover the flat buffer exactly once"
        self._exposed = []
        return table

    def _bucket_hook(self, layer_i: int):
        """Called by the backward walk after layer `layer_i` has enqueued its gradient kernels."""
        b = self.__dict__.get("_buckets")
        if b is None or not self._issue_buckets or layer_i not in self._bucket_first:
            return
        evs = []
        for st in [torch.cuda.current_stream(self.device)] + list(self.ctx.wgrad_streams):
            ev = torch.cuda.Event()
            ev.record(st)
            evs.append(ev)
        b.issue(self._bucket_first[layer_i], evs)

    def all_reduce_gradients(self):
        """Batch-DP exchange step: SUM all-reduce of the flat f32 gradient buffer over RCCL - one collective, or
        the buckets `enable_overlapped_allreduce` issued during backward (then only the wait is left here, and the time the
        optimizer had to wait for them is recorded: `allreduce_exposed_ms`).
        The reference multiplies the loss by world_size and lets DDP average the gradients (trainer.py:424-425), i.e.
        every rank ends up with sum_over_ranks d(loss_rank) - exactly the SUM of the unscaled per-rank gradients."""
        if self.world_size > 1:
            b = self.__dict__.get("_buckets")
            if b is not None and b.issued:
                main = torch.cuda.current_stream(self.device)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(main)
                # a span the walk never hooked (parameters outside `model.<N>.*`: layer -1, or a layer without gradient) goes now:
                # backward has finished on the HOST side only, so the communication stream is ordered behind the main stream and
                # every weight-gradient stream first, exactly as `_bucket_hook` does
                late = [k for k in range(len(b.buckets)) if k not in b.issued]
                if late:
                    evs = []
                    for st in [main] + list(self.ctx.wgrad_streams):
                        ev = torch.cuda.Event()
                        ev.record(st)
                        evs.append(ev)
                    for k in late:
                        b.issue(k, evs)
                b.wait()
                e1.record(main)
                self._exposed.append((e0, e1))
                return
            from ..parallel import allreduce_gradients_
            n = self.groups[-1][0] + self.groups[-1][1]
            allreduce_gradients_(self.G[:n])

    def allreduce_exposed_ms(self):
        """Mean time (ms) the main stream spent waiting for the overlapped all-reduce after backward had finished, over the
        steps since the last call (None if nothing was recorded).  Synchronises."""
        ex = self.__dict__.get("_exposed") or []
        if not ex:
            return None
        torch.cuda.synchronize(self.device)
        ms = [a.elapsed_time(b) for a, b in ex]
        self._exposed = []
        return sum(ms) / len(ms)

    def set_schedule(self, batches_per_epoch: int, global_batch: int | None = None, **overrides):
        """Enable the reference's warm-up and gradient accumulation (engine/trainer.py:337-338, 392-413):
        nw = max(round(warmup_epochs * nb), 100) iterations over which the bias learning rate falls from warmup_bias_lr to
        lr0 * lf(epoch), every other learning rate rises from 0, the momentum rises from warmup_momentum and `accumulate`
        grows from 1 to nbs / batch; afterwards the optimizer steps every max(round(nbs / batch), 1) iterations with
        weight_decay * batch * accumulate / nbs.  `global_batch` = the reference's `batch_size` (all ranks together)."""
        sc = dict(SCHED, **overrides)
        if self._auto_optimizer:
            sc["warmup_bias_lr"] = 0.0  # trainer.py:917, whichever optimizer auto resolved to
        sc["nb"] = int(batches_per_epoch)
        sc["global_batch"] = global_batch
        self.schedule = sc
        if self._graphs is not None and len(self._graphs) == 1:
            raise L.UpaError("set_schedule() before compile(): the optimizer has to stay outside the captured graph")
        return self

    def schedule_at(self, ni: int, batch_size: int):
        """(accumulate, [lr biases, lr decayed weights, lr norm weights], momentum, weight_decay) of iteration ni."""
        h, sc = self.hyp, self.schedule
        if sc is None:
            return 1, [h["lr"]] * 3, h["momentum"], h["weight_decay"]
        gb = sc["global_batch"] or batch_size * self.world_size
        acc0 = max(round(sc["nbs"] / gb), 1)
        wd = h["weight_decay"] * gb * acc0 / sc["nbs"]
        lf = max(1 - (ni // sc["nb"]) / sc["epochs"], 0) * (1.0 - sc["lrf"]) + sc["lrf"]
        nw = max(round(sc["warmup_epochs"] * sc["nb"]), 100) if sc["warmup_epochs"] > 0 else -1
        lr = h["lr"] * lf
        if ni <= nw:
            xi = [0, nw]
            acc = max(1, int(np.interp(ni, xi, [1, sc["nbs"] / gb]).round()))
            lrs = [float(np.interp(ni, xi, [sc["warmup_bias_lr"] if j == 0 else 0.0, lr])) for j in range(3)]
            # Adam's param groups have no "momentum" key, so the reference's warm-up leaves beta1 alone (trainer.py:411)
            mom = h["momentum"] if self.adam else float(np.interp(ni, xi, [sc["warmup_momentum"], h["momentum"]]))
            return acc, lrs, mom, wd
        return acc0, [lr, lr, lr], h["momentum"], wd

    def optimizer_step(self, lrs=None, momentum=None, weight_decay=None):
        h = self.hyp
        lib, st = L.lib(), _s(self.device)
        self.grad_sumsq()
        self.updates += 1
        d = h["ema_decay"] * (1 - math.exp(-self.updates / h["ema_tau"]))
        dp = None
        if self._capturing:  # a replayed graph reads the decay of the current step from device memory
            dp = self.ema_d_dev.data_ptr()
        lrs = [h["lr"]] * 3 if lrs is None else lrs
        mom = h["momentum"] if momentum is None else momentum
        if self.adam:  # the count moves first (not on a step the scaler skips): the three launches read the same t
            L.check(lib.upa_adam_step_advance(self.opt_step_dev.data_ptr(), self.sumsq.data_ptr(), self.scaler.ptr(), st), "adam_step_advance")
        for gi, (start, n, wd) in enumerate(self.groups):
            if n == 0:
                continue
            if wd and weight_decay is not None:
                wd = weight_decay
            o = 4 * start
            if self.adam:
                L.check(lib.upa_adam_ema(self.P.data_ptr() + o, self.G.data_ptr() + o, self.M.data_ptr() + o, self.V.data_ptr() + o,
                                         (self.E.data_ptr() + o) if self.E is not None else None, n, self.sumsq.data_ptr(),
                                         h["max_norm"], lrs[gi], mom, h["beta2"], h["adam_eps"], wd,
                                         int(self.optimizer_name == "AdamW"), self.opt_step_dev.data_ptr(), d, dp, 1, self.scaler.ptr(),
                                         st), "adam")
                continue
            if self.scaler.enabled:  # unscale_ + clip + scaler.step in the same kernel (the momentum buffers start at zero, so the
                # first-step form b = g equals momentum * 0 + g: a skipped first step needs no special case)
                L.check(lib.upa_sgd_nesterov_ema_scaled(self.P.data_ptr() + o, self.G.data_ptr() + o, self.M.data_ptr() + o,
                                                        (self.E.data_ptr() + o) if self.E is not None else None, n,
                                                        self.sumsq.data_ptr(), h["max_norm"], lrs[gi], mom, wd, 0, d, dp, 1,
                                                        self.scaler.ptr(), st), "sgd_scaled")
                continue
            L.check(lib.upa_sgd_nesterov_ema(self.P.data_ptr() + o, self.G.data_ptr() + o, self.M.data_ptr() + o,
                                             (self.E.data_ptr() + o) if self.E is not None else None, n,
                                             self.sumsq.data_ptr(), h["max_norm"], lrs[gi], mom, wd,
                                             int(self.first_step), d, dp, 1, st), "sgd")
        if self.ERB is not None and self.nbuf:
            L.check(lib.upa_ema_update(self.ERB.data_ptr(), self.RB.data_ptr(), self.nbuf, d, dp, st), "ema_buffers")
        self.scaler.update(self.sumsq, st)  # trainer.py:679
        self._scaler_updated = True  # (`grad_norm()` now divides by the scale the update saved, not by the new one)
        self.first_step = False
        # parameters and BN buffers were just rewritten through raw pointers: no `_version` moved, so every packed-weight
        # cache of the inference path (Conv / Detect / C2f) is told explicitly
        CV.bump_weights_generation()

    @property
    def opt_step(self):
        """Adam / AdamW: the optimizer's step count (torch's state["step"]; skipped AMP steps do not count), read from the device
        (a host synchronisation: logging / tests / checkpoints only).  None under SGD, which keeps none."""
        return None if self.opt_step_dev is None else int(self.opt_step_dev.item())

    def optimizer_state(self):
        """Views of the flat optimizer state in parameter-buffer order: SGD {"momentum_buffer"}; Adam / AdamW {"exp_avg", "exp_avg_sq",
        "step"} - what a checkpoint has to keep next to the parameters and the EMA."""
        if not self.adam:
            return {"momentum_buffer": self.M}
        return {"exp_avg": self.M, "exp_avg_sq": self.V, "step": self.opt_step}

    def step(self, img, labels):
        """One training step. After `compile()` the step is replayed as hipGraphs (one graph on a single GPU; forward +
        backward | all-reduce | optimizer on several)."""
        if self._graphs is not None:
            return self._replay(img, labels)
        # buckets go out during backward only on an iteration that ends in an optimizer step (gradient accumulation adds
        # several backward passes into the flat buffer before it is exchanged once)
        acc = self.schedule_at(self.ni, img.shape[0])[0]
        self._issue_buckets = self.world_size > 1 and self.ni - self.last_opt_step >= acc
        items = self.forward_backward(img, labels)
        self._issue_buckets = False
        self._maybe_optimize(img.shape[0])
        return items

    def _maybe_optimize(self, batch_size: int, graph=None):
        """trainer.py:399-413 + 428-431: warm-up state of this iteration; the optimizer steps once `accumulate` iterations
        have added their gradients to the flat buffer (each backward accumulates; the step zeroes it).  The gradient
        all-reduce happens once per optimizer step: the sum of the per-iteration all-reduces DDP would do."""
        acc, lrs, mom, wd = self.schedule_at(self.ni, batch_size)
        if self.ni - self.last_opt_step >= acc:
            self.all_reduce_gradients()
            if graph is not None:
                graph.replay(self.device)
            else:
                self.optimizer_step(lrs, mom, wd if self.schedule is not None else None)
            self.last_opt_step = self.ni
        self.ni += 1

    def compile(self, img, labels, warm_steps=2):
        """Capture the step (fixed shapes) once eager steps have allocated every static buffer and passed the first-step
        branch of the optimizer (`warm_steps` of them are run here on the given batch; pass 0 if >= 1 step already ran).
        Host-side inputs (image batch, labels, EMA decay) are copied into static device buffers before each replay;
        everything else is upa_* launches recorded once."""
        for _ in range(warm_steps):
            self.step(img, labels)
        if self.first_step:
            raise L.UpaError("compile(): run at least one eager step first (the optimizer's first step differs)")
        torch.cuda.synchronize(self.device)
        self._static_img = self.pool.get(("img_in",) + tuple(img.shape), tuple(img.shape), torch.float32, self.device)
        self._static_img.copy_(img)
        self._upload_labels(labels, img.shape[0])
        self._capturing = True
        try:
            g1 = R.HipGraph()
            if self.schedule is not None:
                # warm-up changes lr / momentum every iteration and accumulation skips optimizer steps: the forward +
                # backward is the graph, the three fused optimizer launches stay eager
                self._items = g1.capture(lambda: self.forward_backward(self._static_img, None), device=self.device)
                self._graphs = (g1, None)
            elif self.world_size == 1:
                def whole():
                    it = self.forward_backward(self._static_img, None)
                    self.optimizer_step()
                    return it
                self._items = g1.capture(whole, device=self.device)
                self._graphs = (g1,)
            else:
                g2 = R.HipGraph()
                self._items = g1.capture(lambda: self.forward_backward(self._static_img, None), device=self.device)
                g2.capture(self.optimizer_step, device=self.device)
                self._graphs = (g1, g2)
        finally:
            self._capturing = False
        if self._graphs[-1] is not None:
            self.updates -= 1  # a captured optimizer_step counted an update, but the capture itself executed nothing
        return self

    def _replay(self, img, labels):
        h = self.hyp
        self._static_img.copy_(img, non_blocking=True)
        self._upload_labels(labels, img.shape[0])

        def stage_decay():
            # the decay of THIS optimizer step travels as a kernel argument of a stream-ordered fill (no pinned host slot
            # that a later step could overwrite while an earlier copy is still queued when the host runs replays ahead)
            self.updates += 1
            self.ema_d_dev.fill_(h["ema_decay"] * (1 - math.exp(-self.updates / h["ema_tau"])))

        CV.bump_weights_generation()  # a replayed optimizer writes the weights through raw pointers as well
        if len(self._graphs) == 1:  # forward + backward + optimizer in one graph (single GPU, no schedule)
            stage_decay()
            self._graphs[0].replay(self.device)
            self.last_opt_step = self.ni
            self.ni += 1
            return self._items
        self._graphs[0].replay(self.device)
        if self._graphs[1] is None:  # schedule active: eager optimizer (it counts the update itself)
            self._maybe_optimize(img.shape[0])
        else:
            acc, _, _, _ = self.schedule_at(self.ni, img.shape[0])
            if self.ni - self.last_opt_step >= acc:
                stage_decay()
            self._maybe_optimize(img.shape[0], graph=self._graphs[1])
        return self._items

    def _upload_labels(self, labels, batch_size):
        imgsz_h, imgsz_w = self._imgsz
        gt, ngt = pack_targets(labels, batch_size, imgsz_h, imgsz_w, nc=self.detect.nc)
        need = int(gt.shape[1])
        if self.gt_d is None or self.gt_d.shape[0] != batch_size or need > self.gt_d.shape[1]:
            if self._graphs is not None or self._capturing:
                raise L.UpaError(f"a batch needs {need} gt rows per image but the compiled step holds {self.max_gt}: set "
                                 f"trainer.max_gt >= {need} (<= {MAX_GT_CAP}) before compile()")
            self.max_gt = max(self.max_gt, need)
            self.gt_d = torch.zeros(batch_size, self.max_gt, 5, dtype=torch.float32, device=self.device)
            self.ngt_d = torch.zeros(batch_size, dtype=torch.int32, device=self.device)
        # through PINNED staging buffers (a ring of four, each guarded by the event of its last copy): a copy from pageable memory makes the
        # host wait for the stream, and the step's launches then trail the GPU by the time `pack_targets` + the copy took (0.45 ms of idle
        # GPU per yolov8s step in the kernel trace, tools/experiments/r05_train_gaps.py)
        rows = int(self.gt_d.shape[1])
        ring = self.__dict__.setdefault("_label_ring", [None] * 4)
        self._label_slot = (self.__dict__.get("_label_slot", -1) + 1) % len(ring)
        ent = ring[self._label_slot]
        if ent is None or ent[0].shape != (batch_size, rows, 5):
            ent = [torch.zeros(batch_size, rows, 5, dtype=torch.float32).pin_memory(), torch.zeros(batch_size, dtype=torch.int32).pin_memory(), None]
            ring[self._label_slot] = ent
        if ent[2] is not None:
            ent[2].synchronize()
        ent[0][:, :need].copy_(gt)
        ent[1].copy_(ngt)
        self.gt_d.copy_(ent[0], non_blocking=True)  # (rows past an image's count are never read: n_gt bounds them)
        self.ngt_d.copy_(ent[1], non_blocking=True)
        ent[2] = torch.cuda.Event()
        ent[2].record(torch.cuda.current_stream(self.device))

    def grad_norm(self) -> float:
        """Norm of the (unscaled) gradients in the flat buffer."""
        return float(torch.sqrt(self.grad_sumsq())[0]) / self.scaler.carried_scale(self._scaler_updated)

    # ---- the replicate steps of the multi-rank loop ------------------------------------------------------------------------
    def sync_ema_buffers(self, src: int = 0):
        """Rank `src`'s EMA float buffers (BatchNorm running mean / variance) on every rank, to be called before a validate that is
        sharded over the ranks (engine/trainer.py:695-698).  The parameters need nothing: after the gradient all-reduce every rank
        applies the same update, so P, M and the EMA parameters E are equal by construction; the BatchNorm running statistics are
        NOT (every rank normalises with its own shard's batch statistics, there is no SyncBN - trainer.py:253-258 only wraps in DDP,
        which broadcasts buffers rank 0 -> all at each forward), so without this the ranks would validate different models.  The
        reference loops over `ema.buffers()`; the EMA buffers live in ONE flat f32 tensor here (`ERB`), so it is one broadcast.
        The live model's buffers (`RB`) get the same treatment - DDP's `broadcast_buffers` (default True) keeps them rank 0's."""
        from ..parallel import broadcast_
        if self.nbuf:
            if self.ERB is not None:
                broadcast_(self.ERB[:self.nbuf], src)
            broadcast_(self.RB[:self.nbuf], src)

    def broadcast_stop(self, stop: bool, src: int = 0) -> bool:
        """The early-stopping decision of rank `src` on every rank (engine/trainer.py:505-508): all ranks must leave the epoch loop
        together or the next collective hangs."""
        from ..parallel import broadcast_flag
        return broadcast_flag(stop, src, self.device)

    def ema_state_dict(self):
        """The EMA weights under the reference's state_dict keys (for validation / checkpoints)."""
        out = {}
        for k, p in self.model.named_parameters():
            if p.requires_grad and self.E is not None:
                off = (p.data_ptr() - self.P.data_ptr()) // 4
                out[k] = self.E[off:off + p.numel()].view(p.shape)
            else:
                out[k] = p.detach()
        for k, b in self.model.named_buffers():
            if b.dtype.is_floating_point and self.ERB is not None:
                off = (b.data_ptr() - self.RB.data_ptr()) // 4
                out[k] = self.ERB[off:off + b.numel()].view(b.shape)
            else:
                out[k] = b
        return out


class DetectT(_Seq):
    """Train-mode Detect (head.py:116-126 returns the raw per-level maps) + v8DetectionLoss + its gradient."""

    def __init__(self, ctx, m: H.Detect, name, trainer):
        super().__init__(ctx)
        self.m, self.tr = m, trainer
        self.nl, self.nc, self.reg_max, self.no = m.nl, m.nc, m.reg_max, m.no
        self.br = []
        for i in range(m.nl):
            row = []
            for tag, seq in (("cv2", m.cv2[i]), ("cv3", m.cv3[i])):
                if tag == "cv3" and not m.legacy_cls:
                    # head.py:101-110: Sequential(DWConv, Conv 1x1), Sequential(DWConv, Conv 1x1), Conv2d 1x1
                    ops = []
                    for j in (0, 1):
                        dw, pw = seq[j][0], seq[j][1]
                        ops.append(DWConvT(ctx, dw.conv, dw.bn, dw._act_code(), f"{name}.{tag}.{i}.{j}.0", nc=m.nc))
                        ops.append(ConvT(ctx, pw.conv, pw.bn, pw._act_code(), f"{name}.{tag}.{i}.{j}.1"))
                    row.append(ops + [ConvT(ctx, seq[2], None, L.ACT_NONE, f"{name}.{tag}.{i}.2")])
                    continue
                row.append([ConvT(ctx, seq[0].conv, seq[0].bn, seq[0]._act_code(), f"{name}.{tag}.{i}.0"),
                            ConvT(ctx, seq[1].conv, seq[1].bn, seq[1]._act_code(), f"{name}.{tag}.{i}.1"),
                            ConvT(ctx, seq[2], None, L.ACT_NONE, f"{name}.{tag}.{i}.2")])
            self.br.append(row)

    def convs(self):
        return [cv for row in self.br for seq in row for cv in seq]

    def forward(self, xs):
        c = self.ctx
        dev = c.device
        nb = 4 * self.reg_max
        self.xs = list(xs)
        self.raw, self.raw32 = [None] * len(xs), [None] * len(xs)

        def level(i, x):
            n, _, h, w = x.shape
            raw = _new(n, self.no, h, w, c.dtype, dev, (id(self), "raw", i))
            for k, (seq, out) in enumerate(zip(self.br[i], (raw[:, :nb], raw[:, nb:]))):
                t = x
                for op in seq[:-1]:
                    t = op.forward(t)
                seq[-1].forward(t, out=out)
            self.raw[i] = raw
            if c.dtype == torch.float32:
                self.raw32[i] = raw
            else:  # the loss reads f32 maps
                r32 = _new(n, self.no, h, w, torch.float32, dev, (id(self), "raw32", i))
                vs, vd = R.view_of(raw), R.view_of(r32)
                L.check(L.lib().upa_cast_view(vs.ptr, vs.dtype, vs.ld, vd.ptr, vd.dtype, vd.ld, vs.n * vs.h * vs.w, vs.c,
                                              _s(dev)), "cast_view")
                self.raw32[i] = r32
            self._level_more(i, x)

        # The levels are independent chains (head.py:116-126).  The 40 x 40 / 20 x 20 levels are strings of 5-15 us launches (a few
        # hundred workgroups each): on a second stream they run beside the 80 x 80 level's chip-filling launches instead of after them.
        self._fork_levels(lambda: level(0, xs[0]), lambda: [level(i, xs[i]) for i in range(1, len(xs))], len(xs) > 1)
        return self.raw

    def _fork_levels(self, first, rest, fork: bool):
        """`first()` on the current stream, `rest()` on the context's level stream (own reduction workspace), joined at the end."""
        c = self.ctx
        if not (fork and self.fork_levels):
            first()
            rest()
            return
        main = torch.cuda.current_stream(c.device)
        ev = torch.cuda.Event()
        ev.record(main)
        c.level_stream.wait_event(ev)
        c._ws_sel = 1
        try:
            with torch.cuda.stream(c.level_stream):
                rest()
                done = torch.cuda.Event()
                done.record(c.level_stream)
        finally:
            c._ws_sel = 0
        first()
        main.wait_event(done)

    fork_levels = True  # (False: every level on the main stream, as before round 5 - the A/B switch)

    # the hooks of a head with more branches on the same level inputs (`SegmentT`)
    def _level_more(self, i, x):
        """Further train-mode branches of level i's input x, run on that level's stream."""

    def _more_losses(self, items, wsb, batch_size, n_anchors, max_gt):
        """Further loss terms on the detection loss's workspace (its per-anchor assignment); returns the step's loss items."""
        return items

    def _level_more_bwd(self, i, dx):
        """Backward of `_level_more`'s branches, accumulated into dx (level i's input gradient, already written)."""

    def loss_backward(self, labels, batch_size):
        """v8DetectionLoss (utils/loss.py:471-528) + gradient; then backward through the head into the neck outputs."""
        c, tr = self.ctx, self.tr
        dev = c.device
        lib = L.lib()
        h = tr.hyp
        imgsz_h = int(self.raw[0].shape[2] * float(self.m.stride[0]))
        imgsz_w = int(self.raw[0].shape[3] * float(self.m.stride[0]))
        tr._imgsz = (imgsz_h, imgsz_w)
        if labels is not None:  # None: already uploaded into the static buffers (graph replay)
            tr._upload_labels(labels, batch_size)
        gt_d, ngt_d = tr.gt_d, tr.ngt_d
        max_gt = int(gt_d.shape[1])
        grads32 = []
        for i, r in enumerate(self.raw32):
            n, ch, hh, ww = r.shape
            grads32.append(_new(n, ch, hh, ww, torch.float32, dev, (id(self), "graw32", i)))
        nl = self.nl
        FP = C.c_void_p * nl
        feats = FP(*[R.view_of(r).ptr for r in self.raw32])
        grads = FP(*[R.view_of(g).ptr for g in grads32])
        IA = C.c_int * nl
        hs = IA(*[int(r.shape[2]) for r in self.raw32])
        ws = IA(*[int(r.shape[3]) for r in self.raw32])
        lds = IA(*[R.view_of(r).ld for r in self.raw32])
        strides = (C.c_float * nl)(*[float(s) for s in self.m.stride])
        A = sum(int(r.shape[2]) * int(r.shape[3]) for r in self.raw32)
        nbytes = lib.upa_detection_loss_workspace_bytes(batch_size, A, max_gt)
        wsb = tr.pool.get(("loss_ws", batch_size, A, max_gt), (nbytes,), torch.uint8, dev)
        items = tr.pool.get(("loss_items",), (3,), torch.float32, dev)
        L.check(lib.upa_detection_loss_scaled(C.cast(feats, C.c_void_p), C.cast(grads, C.c_void_p), C.cast(hs, C.c_void_p),
                                              C.cast(ws, C.c_void_p), C.cast(lds, C.c_void_p), C.cast(strides, C.c_void_p), nl,
                                              batch_size, self.nc, self.reg_max, gt_d.data_ptr(), ngt_d.data_ptr(), max_gt,
                                              h["box"], h["cls"], h["dfl"], 1.0, tr.scaler.ptr(), items.data_ptr(), wsb.data_ptr(),
                                              nbytes, _s(dev)), "detection_loss")
        items = self._more_losses(items, wsb, batch_size, A, max_gt)
        nb = 4 * self.reg_max

        def level_bwd(i):
            g32 = grads32[i]
            if c.dtype == torch.float32:
                graw = g32
            else:
                n, ch, hh, ww = g32.shape
                graw = _new(n, ch, hh, ww, c.dtype, dev, (id(self), "graw", i))
                vs, vd = R.view_of(g32), R.view_of(graw)
                L.check(lib.upa_cast_view(vs.ptr, vs.dtype, vs.ld, vd.ptr, vd.dtype, vd.ld, vs.n * vs.h * vs.w, vs.c, _s(dev)),
                        "cast_view")
            # feature map feeding level i: route the gradient into the producing node
            src = tr.nodes[self.m.f[i]]
            dx, acc = tr._grad_of(src)
            for k, (seq, dy) in enumerate(zip(self.br[i], (graw[:, :nb], graw[:, nb:]))):
                g = dy
                for j in range(len(seq) - 1, 0, -1):  # the chain's inner gradients: one buffer per op input
                    vt = R.view_of(seq[j].x)
                    d = _new(vt.n, vt.c, vt.h, vt.w, c.dtype, dev, (id(self), "d", i, k, j))
                    seq[j].backward(g, d, False)
                    g = d
                seq[0].backward(g, dx, acc or k > 0)
            self._level_more_bwd(i, dx)

        # as in the forward pass: the small levels' chains beside the 80 x 80 level's (they write the gradients of different neck outputs)
        self._fork_levels(lambda: level_bwd(0), lambda: [level_bwd(i) for i in range(1, nl)], nl > 1)
        return items


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
        raise L.UpaError(f"label class {float(bad[0]):g} is outside [0, {nc}) of the model's classes")
    per = [((bi == j) & keep).nonzero().view(-1) for j in range(batch_size)]
    most = max([int(ix.numel()) for ix in per] + [1])
    rows = max(min_rows, (most + 63) // 64 * 64)
    if rows > MAX_GT_CAP:
        raise L.UpaError(f"an image has {most} boxes; the loss kernels hold at most {MAX_GT_CAP} per image")
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
            raise L.UpaError(f"image {j} keeps {int(kept.numel())} boxes but the gt rows hold {rows}")
        mid[j, :kept.numel()] = (kept + 1).to(torch.int32)
    return mid


MASK_ID_MAX = 255  # upa_mask_loss reads the overlap mask as uint8 (the reference's dataset builds it as uint8 as well, data/utils.py)


class ConvTransposeT:
    """Train-mode nn.ConvTranspose2d(c_, c_, 2, 2, 0, bias=True), Proto's upsample (block.py:257-276): upa_conv_transpose2x2 with the
    weight packed on the device from the f32 master weight (`pack_phase_weights`, once per step with every other repack), and
    upa_conv_transpose2x2_bwd (dx, dW, db).  The `ConvT` surface for the trainer's repack hooks."""

    @staticmethod
    def check(m, name):
        if not (isinstance(m, nn.ConvTranspose2d) and m.kernel_size == (2, 2) and m.stride == (2, 2) and m.padding == (0, 0)
                and m.output_padding == (0, 0) and m.groups == 1 and m.dilation == (1, 1) and m.bias is not None):
            raise L.UpaError(f"{name}: training supports ConvTranspose2d(k 2, stride 2, pad 0, groups 1, bias=True) only")

    def __init__(self, ctx: _Ctx, m: nn.ConvTranspose2d, name: str):
        self.check(m, name)
        self.ctx, self.m, self.name = ctx, m, name
        self.cin, self.cout = m.in_channels, m.out_channels
        lib = L.lib()
        self.wp = torch.empty(lib.upa_conv_transpose2x2_packed_weight_bytes(self.cin, self.cout, ctx.code), dtype=torch.uint8, device=ctx.device)
        self.nws = lib.upa_conv_transpose2x2_bwd_workspace_bytes(self.cin, self.cout)
        self.ws = torch.empty(self.nws, dtype=torch.uint8, device=ctx.device)
        self.x = None

    def convs(self):
        return [self]

    def pack(self):
        c = self.ctx
        L.check(L.lib().upa_pack_conv_transpose2x2_weight_dev(self.m.weight.data_ptr(), self.cin, self.cout, c.code, self.wp.data_ptr(),
                                                              _s(c.device)), f"pack_conv_transpose[{self.name}]")

    pack_phase_weights = pack  # (the per-step hook `_pack_weights` calls on every op before the batched repack)

    def pack_descs(self):
        return []

    def forward(self, x, out=None):
        c = self.ctx
        n, _, h, w = x.shape
        self.x = x
        y = out if out is not None else _new(n, self.cout, 2 * h, 2 * w, c.dtype, c.device, (id(self), "y"))
        vx, vy = R.view_of(x), R.view_of(y)
        L.check(L.lib().upa_conv_transpose2x2(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, self.wp.data_ptr(), self.m.bias.data_ptr(), vy.ptr,
                                              self.cout, vy.ld, vx.dtype, _s(c.device)), f"conv_transpose2x2[{self.name}]")
        return y

    def backward(self, dy, dx=None, accumulate=False):
        c = self.ctx
        vx, vdy = R.view_of(self.x), R.view_of(dy)
        vdx = None if dx is None else R.view_of(dx)
        L.check(L.lib().upa_conv_transpose2x2_bwd(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, vdy.ptr, self.cout, vdy.ld, self.m.weight.data_ptr(),
                                                  None if dx is None else vdx.ptr, 0 if dx is None else vdx.ld, int(accumulate),
                                                  self.m.weight.grad.data_ptr(), self.m.bias.grad.data_ptr(), 1, self.ws.data_ptr(), self.nws,
                                                  vx.dtype, _s(c.device)), f"conv_transpose2x2_bwd[{self.name}]")


class ProtoT(_Seq):
    """Train-mode Proto (block.py:257-276): cv3(cv2(upsample(cv1(x))))."""

    def __init__(self, ctx, m: B.Proto, name):
        super().__init__(ctx)
        self.cv1 = ConvT(ctx, m.cv1.conv, m.cv1.bn, m.cv1._act_code(), name + ".cv1")
        self.up = ConvTransposeT(ctx, m.upsample, name + ".upsample")
        self.cv2 = ConvT(ctx, m.cv2.conv, m.cv2.bn, m.cv2._act_code(), name + ".cv2")
        self.cv3 = ConvT(ctx, m.cv3.conv, m.cv3.bn, m.cv3._act_code(), name + ".cv3")

    def convs(self):
        return [self.cv1, self.up, self.cv2, self.cv3]

    def forward(self, x, out=None):
        return self.cv3.forward(self.cv2.forward(self.up.forward(self.cv1.forward(x))), out=out)

    def backward(self, dy, dx, accumulate):
        c = self.ctx
        g = dy
        for i, op in ((3, self.cv3), (2, self.cv2), (1, self.up)):
            vt = R.view_of(op.x)
            d = _new(vt.n, vt.c, vt.h, vt.w, c.dtype, c.device, (id(self), "d", i))
            op.backward(g, d, False)
            g = d
        self.cv1.backward(g, dx, accumulate)


class SegmentT(DetectT):
    """Train-mode Segment (head.py:790-837 returns the raw maps, the mask coefficients and the prototypes) + v8SegmentationLoss
    (utils/loss.py:531-709) + its gradient: `DetectT` with, per level, the cv4 chain (Conv 3x3, Conv 3x3, Conv2d 1x1 -> nm) and, on
    level 0's input, `ProtoT`.  The mask term is upa_mask_loss on the detection loss's workspace (the per-anchor assignment is read in
    place); cv4 and Proto backpropagate into the same neck gradients as cv2 / cv3.  Loss items: (box, seg, cls, dfl)."""

    def __init__(self, ctx, m: H.Segment, name, trainer):
        super().__init__(ctx, m, name, trainer)
        self.nm = m.nm
        self.cv4 = [[ConvT(ctx, seq[0].conv, seq[0].bn, seq[0]._act_code(), f"{name}.cv4.{i}.0"),
                     ConvT(ctx, seq[1].conv, seq[1].bn, seq[1]._act_code(), f"{name}.cv4.{i}.1"),
                     ConvT(ctx, seq[2], None, L.ACT_NONE, f"{name}.cv4.{i}.2")] for i, seq in enumerate(m.cv4)]
        self.proto = ProtoT(ctx, m.proto, name + ".proto")
        self.mc = [None] * m.nl
        self.p = None

    def convs(self):
        return super().convs() + [cv for seq in self.cv4 for cv in seq] + self.proto.convs()

    def _level_more(self, i, x):
        t = x
        for op in self.cv4[i]:
            t = op.forward(t)
        self.mc[i] = t
        if i == 0:
            self.p = self.proto.forward(x)

    def _more_losses(self, items, wsb, batch_size, n_anchors, max_gt):
        c, tr, lib = self.ctx, self.tr, L.lib()
        dev = c.device
        nl = self.nl
        vp = R.view_of(self.p)
        self.dmc = [_new(*[int(v) for v in t.shape], c.dtype, dev, (id(self), "dmc", i)) for i, t in enumerate(self.mc)]
        self.dp = _new(vp.n, vp.c, vp.h, vp.w, c.dtype, dev, (id(self), "dproto"))
        vdp = R.view_of(self.dp)
        vm, vd = [R.view_of(t) for t in self.mc], [R.view_of(t) for t in self.dmc]
        FP, IA = C.c_void_p * nl, C.c_int * nl
        coefs, dcoefs = FP(*[v.ptr for v in vm]), FP(*[v.ptr for v in vd])
        hs, ws = IA(*[v.h for v in vm]), IA(*[v.w for v in vm])
        lds, ldds = IA(*[v.ld for v in vm]), IA(*[v.ld for v in vd])
        masks_d, mid_d = tr.masks_d, tr.mid_d
        if tuple(masks_d.shape) != (batch_size, vp.h, vp.w) or tuple(mid_d.shape) != (batch_size, max_gt):
            raise L.UpaError(f"mask buffers {tuple(masks_d.shape)} / {tuple(mid_d.shape)} do not match the step: prototypes "
                             f"{(batch_size, vp.h, vp.w)}, gt rows {(batch_size, max_gt)}")
        asg = lib.upa_detection_loss_assignment(wsb.data_ptr(), batch_size, n_anchors, max_gt)
        nws = lib.upa_mask_loss_workspace_bytes(batch_size, n_anchors)
        mws = tr.pool.get(("mask_loss_ws", batch_size, n_anchors), (nws,), torch.uint8, dev)
        items4 = tr.pool.get(("loss_items4",), (4,), torch.float32, dev)
        imgsz_h, imgsz_w = tr._imgsz
        L.check(lib.upa_mask_loss(vp.ptr, batch_size, vp.h, vp.w, self.nm, vp.ld, C.cast(coefs, C.c_void_p), C.cast(dcoefs, C.c_void_p),
                                  C.cast(hs, C.c_void_p), C.cast(ws, C.c_void_p), C.cast(lds, C.c_void_p), C.cast(ldds, C.c_void_p), nl,
                                  asg, 2, tr.gt_d.data_ptr(), tr.ngt_d.data_ptr(), max_gt, mid_d.data_ptr(), masks_d.data_ptr(),
                                  imgsz_h, imgsz_w, tr.hyp["box"], 1.0, tr.scaler.ptr(), items4.data_ptr() + 4, vdp.ptr, vdp.ld,
                                  mws.data_ptr(), nws, c.code, _s(dev)), "mask_loss")
        # (box, seg, cls, dfl), loss.py:541: box and [cls, dfl] of the detection items around the seg item written above
        L.check(lib.upa_copy_rows(items.data_ptr(), 1, 1, 3, items4.data_ptr(), 4, _s(dev)), "copy_rows")
        L.check(lib.upa_copy_rows(items.data_ptr() + 4, 1, 2, 3, items4.data_ptr() + 8, 4, _s(dev)), "copy_rows")
        return items4

    def _level_more_bwd(self, i, dx):
        c = self.ctx
        seq, g = self.cv4[i], self.dmc[i]
        for j in range(len(seq) - 1, 0, -1):
            vt = R.view_of(seq[j].x)
            d = _new(vt.n, vt.c, vt.h, vt.w, c.dtype, c.device, (id(self), "d4", i, j))
            seq[j].backward(g, d, False)
            g = d
        seq[0].backward(g, dx, True)
        if i == 0:
            self.proto.backward(self.dp, dx, True)


class ClassifyT(_Seq):
    """Train-mode Classify (head.py:1523-1529 returns the raw logits) + v8ClassificationLoss (utils/loss.py:873-880) + its gradient:
    ConvT (in output-channel slices, `_conv_parts`) -> upa_global_avgpool_fwd -> upa_linear, then upa_cross_entropy_fwd_bwd -> upa_linear_bwd -> upa_global_avgpool_bwd ->
    ConvT.backward.  The pooled rows, the logits and their gradients are float32 in both trainer modes and the linear layer is exact
    float32 (as the inference head keeps it, `Classify` docstring); only the (B, 1280, h, w) activation and its gradient carry the
    trainer's dtype.  `Dropout(p = 0)` is the identity and never runs."""

    def __init__(self, ctx, m: H.Classify, name, trainer):
        super().__init__(ctx)
        self.m, self.tr = m, trainer
        self.nc, self.c_ = m.linear.out_features, m.linear.in_features
        self.ncp = (self.nc + 3) // 4 * 4  # logits rows are 16-byte multiples (upa_linear's stores); pad columns carry zero weights
        self.parts = self._conv_parts(ctx, m.conv, name + ".conv")
        dev = ctx.device
        nb = L.lib().upa_conv_packed_weight_bytes(self.nc, self.c_, 1, L.UPA_F32)
        self.wl = torch.empty(nb, dtype=torch.uint8, device=dev)            # upa_linear's packed float32 weight, rebuilt every step
        self.bias_pad = torch.zeros(self.ncp, dtype=torch.float32, device=dev)

    MAX_BN_CHANNELS = 1024  # the channel reductions of csrc/train.hip take c <= 256 * (16 / element size); the context's scratch is sized for it

    @classmethod
    def _conv_parts(cls, ctx, cv, name):
        """The head's Conv(c1, 1280, 1) as [(first channel, last channel, ConvT)] over equal output-channel slices of at most 1024
        channels: BatchNorm is per channel, so a Conv is exactly the concatenation of its output-channel slices, and 1280 channels are
        past what the per-channel reduction kernels take in one call.  A slice sees the layer's parameters, gradients and running
        statistics through views of the flat buffers (rows a..b of the OIHW weight are contiguous)."""
        from types import SimpleNamespace as NS
        conv, bn = cv.conv, cv.bn
        cout = conv.out_channels
        nparts = next((k for k in range(-(-cout // cls.MAX_BN_CHANNELS), cout + 1)
                       if cout % k == 0 and (cout // k) % 16 == 0 and cout // k <= cls.MAX_BN_CHANNELS), None)
        if nparts is None:
            raise L.UpaError(f"{name}: {cout} output channels do not split into equal 16-channel-aligned slices of <= {cls.MAX_BN_CHANNELS}")
        if nparts == 1:
            return [(0, cout, ConvT(ctx, conv, bn, cv._act_code(), name))]

        def sl(p, a, b):  # rows a..b of a parameter with its gradient view; buffers have no gradient
            v = p.data[a:b]
            if getattr(p, "grad", None) is not None:
                v.grad = p.grad[a:b]
            return v

        step, parts = cout // nparts, []
        for j in range(nparts):
            a, b = j * step, (j + 1) * step
            c = NS(weight=sl(conv.weight, a, b), bias=None, groups=conv.groups, dilation=conv.dilation, kernel_size=conv.kernel_size,
                   stride=conv.stride, padding=conv.padding, out_channels=b - a, in_channels=conv.in_channels)
            n = NS(weight=sl(bn.weight, a, b), bias=sl(bn.bias, a, b), running_mean=sl(bn.running_mean, a, b),
                   running_var=sl(bn.running_var, a, b), eps=bn.eps, momentum=bn.momentum)
            parts.append((a, b, ConvT(ctx, c, n, cv._act_code(), f"{name}[{a}:{b}]")))
        return parts

    def convs(self):
        return [p for _, _, p in self.parts]

    def extra_pack_descs(self):
        """The linear layer's row of the trainer's batched pack table: its master weight is an (nc, 1280, 1, 1) 1x1 kernel."""
        return [(self.m.linear.weight.data_ptr(), self.wl.data_ptr(), self.nc, self.c_, 1, L.UPA_F32, 0)]

    def forward(self, x):
        c, lib = self.ctx, L.lib()
        dev, st = c.device, _s(c.device)
        n, _, h, w = x.shape
        self.y = _new(n, self.c_, h, w, c.dtype, dev, (id(self), "y"))
        for a, b, part in self.parts:
            part.forward(x, out=self.y[:, a:b])
        vy = R.view_of(self.y)
        self.pooled = R.alloc_plain((n, self.c_), torch.float32, dev, (id(self), "pooled"))
        L.check(lib.upa_global_avgpool_fwd(vy.ptr, vy.n, vy.h, vy.w, vy.c, vy.ld, self.pooled.data_ptr(), self.c_, vy.dtype, st),
                "global_avgpool_fwd")
        lin = self.m.linear
        bias = None
        if lin.bias is not None:  # the bias row padded to ncp (the flat parameter buffer has other parameters behind it)
            L.check(lib.upa_copy_rows(lin.bias.data_ptr(), 1, self.nc, self.nc, self.bias_pad.data_ptr(), self.ncp, st), "copy_rows")
            bias = self.bias_pad.data_ptr()
        self.logits = R.alloc_plain((n, self.ncp), torch.float32, dev, (id(self), "logits"))
        L.check(lib.upa_linear(self.pooled.data_ptr(), n, self.c_, self.c_, self.wl.data_ptr(), bias, self.logits.data_ptr(), self.ncp,
                               self.ncp, None, 0, L.ACT_NONE, st), "linear")
        return self.logits[:, :self.nc]

    def loss_backward(self, labels, batch_size):
        """F.cross_entropy(logits, cls, reduction="mean") and the whole backward of the head; returns the (1,) unscaled loss."""
        c, tr, lib = self.ctx, self.tr, L.lib()
        dev, st = c.device, _s(c.device)
        if labels is not None:  # None: already uploaded into the static buffer (graph replay)
            tr._upload_labels(labels, batch_size)
        n = batch_size
        nws = lib.upa_cross_entropy_workspace_bytes(n)
        ws = tr.pool.get(("ce_ws", n), (nws,), torch.uint8, dev)
        items = tr.pool.get(("loss_items",), (1,), torch.float32, dev)
        dlogits = R.alloc_plain((n, self.ncp), torch.float32, dev, (id(self), "dlogits"))
        L.check(lib.upa_cross_entropy_fwd_bwd(self.logits.data_ptr(), n, self.nc, self.ncp, tr.cls_d.data_ptr(), tr.scaler.ptr(),
                                              items.data_ptr(), dlogits.data_ptr(), self.ncp, ws.data_ptr(), nws, st), "cross_entropy")
        lin = self.m.linear
        dpooled = R.alloc_plain((n, self.c_), torch.float32, dev, (id(self), "dpooled"))
        L.check(lib.upa_linear_bwd(self.pooled.data_ptr(), n, self.c_, self.c_, dlogits.data_ptr(), self.nc, self.ncp,
                                   lin.weight.data_ptr(), lin.weight.grad.data_ptr(),
                                   None if lin.bias is None else lin.bias.grad.data_ptr(), dpooled.data_ptr(), self.c_, 1, st),
                "linear_bwd")
        vy = R.view_of(self.y)
        dy = _new(vy.n, vy.c, vy.h, vy.w, c.dtype, dev, (id(self), "dy"))
        vdy = R.view_of(dy)
        L.check(lib.upa_global_avgpool_bwd(dpooled.data_ptr(), self.c_, vdy.n, vdy.h, vdy.w, vdy.c, vdy.ptr, vdy.ld, 0, vdy.dtype, st),
                "global_avgpool_bwd")
        f = self.m.f
        src = tr.nodes[f] if f != -1 else tr.nodes[self.m.i - 1]
        dx, acc = tr._grad_of(src)
        for j, (a, b, part) in enumerate(self.parts):
            part.backward(dy[:, a:b], dx, acc or j > 0)
        return items


def pack_cls_targets(labels, batch_size, nc):
    """`batch["cls"]` of the reference's classification batch - (B,) integer class ids (models/yolo/classify/train.py
    preprocess_batch) - as a host int32 tensor.  A label outside [0, nc) is refused here (torch's cross_entropy fails on the host with
    an index error; the kernel would make the row NaN)."""
    cls = labels["cls"] if isinstance(labels, dict) else labels
    cls = torch.as_tensor(cls).detach().view(-1).cpu()
    if cls.dtype.is_floating_point or cls.dtype == torch.bool:
        raise L.UpaError(f"classification labels must be integer class ids, got {cls.dtype}")
    if cls.numel() != batch_size:
        raise L.UpaError(f"{cls.numel()} labels for a batch of {batch_size} images")
    cls = cls.long()
    bad = (cls < 0) | (cls >= nc)
    if bool(bad.any()):
        raise L.UpaError(f"label class {int(cls[bad][0])} is outside [0, {nc}) of the model's classes")
    return cls.to(torch.int32)


class ClassificationTrainer(DetectionTrainer):
    """One-process-per-GPU trainer for a ClassificationModel (reference: models/yolo/classify/train.py on engine/trainer.py's loop; the
    loss is v8ClassificationLoss, utils/loss.py:873-880).  The graph walk, `step`, `compile` / replay, `set_schedule`, `optimizer_step`,
    GradScaler, EMA, `sync_ema_buffers` and `all_reduce_gradients` are DetectionTrainer's; the tail of the graph is `ClassifyT` and the
    labels are the batch's `cls` vector.  The loss is a mean over the rank's batch, so the SUM all-reduce of the per-rank gradients is
    what the reference's `loss * world_size` under DDP's average gives.  `step()` returns the (1,) unscaled loss.
    The yolov8-cls module set (Conv, C2f, Classify) trains by default; YOLO11's (C3k2, C2PSA) trains on request, `yolo11=True`: without
    it a YOLO11 model is refused as before, so a caller that relies on that refusal keeps it.  The optimizer is the detection step's:
    SGD-Nesterov by default, Adam / AdamW / auto on request (`optimizer=`, `iterations=`)."""

    def __init__(self, model, dtype=torch.bfloat16, hyp=None, device=None, world_size=1, ema=True, wgrad_streams: int = 1,
                 amp_scaler: bool = False, yolo11: bool = False, optimizer: str = "SGD", iterations=None):
        tail = model.model[-1] if hasattr(model, "model") and len(model.model) else None
        if not isinstance(tail, H.Classify):
            raise L.UpaError(f"ClassificationTrainer needs a model that ends in a Classify head, got {type(tail).__name__}")
        for m in model.modules():
            if isinstance(m, (B.C3k2, B.C2PSA)) and not yolo11:
                raise L.UpaError(f"{type(m).__name__} (YOLO11) trains on request only: ClassificationTrainer(..., yolo11=True) enables the "
                                 "C3k2 / C2PSA training path")
            if isinstance(m, B.v10_Attention) and (m.key_dim, m.head_dim) != (32, 64):
                raise L.UpaError(f"v10_Attention with key_dim {m.key_dim} / head_dim {m.head_dim} has no training path on HIP (32 / 64, every "
                                 "YOLO11 scale)")
            if isinstance(m, nn.Dropout) and m.p > 0:
                raise L.UpaError(f"Dropout(p={m.p:g}) has no training path on HIP (the reference trains with dropout=0.0; no device RNG)")
        self.cls_d = None
        super().__init__(model, dtype=dtype, hyp=hyp, device=device, world_size=world_size, ema=ema, wgrad_streams=wgrad_streams,
                         amp_scaler=amp_scaler, optimizer=optimizer, iterations=iterations)

    def _tail_op(self, m, name):
        if isinstance(m, H.Classify):
            return ClassifyT(self.ctx, m, name, self), "classify"
        if isinstance(m, H.Detect):
            raise L.UpaError(f"{type(m).__name__} (layer {m.i}) is not a classification tail: use DetectionTrainer")
        return None

    def _upload_labels(self, labels, batch_size):
        cls = pack_cls_targets(labels, batch_size, self.detect.nc)
        if self.cls_d is None or self.cls_d.shape[0] != batch_size:
            if self._graphs is not None or self._capturing:
                raise L.UpaError(f"a batch of {batch_size} images but the compiled step holds {int(self.cls_d.shape[0])}")
            self.cls_d = torch.zeros(batch_size, dtype=torch.int32, device=self.device)
        # through a ring of pinned staging buffers, each guarded by the event of its last copy, as the detection labels go
        ring = self.__dict__.setdefault("_label_ring", [None] * 4)
        self._label_slot = (self.__dict__.get("_label_slot", -1) + 1) % len(ring)
        ent = ring[self._label_slot]
        if ent is None or ent[0].shape[0] != batch_size:
            ent = [torch.zeros(batch_size, dtype=torch.int32).pin_memory(), None]
            ring[self._label_slot] = ent
        if ent[1] is not None:
            ent[1].synchronize()
        ent[0].copy_(cls)
        self.cls_d.copy_(ent[0], non_blocking=True)
        ent[1] = torch.cuda.Event()
        ent[1].record(torch.cuda.current_stream(self.device))


class SegmentationTrainer(DetectionTrainer):
    """One-process-per-GPU trainer for a SegmentationModel (reference: models/yolo/segment/train.py on engine/trainer.py's loop; the loss
    is v8SegmentationLoss, utils/loss.py:531-709).  Everything but the tail and the labels is DetectionTrainer's: the graph walk, `step`,
    `compile` / replay, `set_schedule`, every optimizer, GradScaler, EMA and the multi-rank path.  The tail is `SegmentT`; the labels
    additionally carry `"masks"`, the (B, mh, mw) overlap mask at prototype resolution (instance p of an image painted as p + 1, later
    instances over earlier ones - what the reference's dataset delivers with overlap_mask=True, mask_ratio=4).  `step()` returns the
    (4,) loss items (box, seg, cls, dfl).
    Refused, by the constructor or the label upload, before any launch: overlap_mask=False (per-instance mask stacks); masks that are not
    at prototype resolution (the reference's F.interpolate fallback, loss.py:604-605, is not built); instance ids above 255 (the mask is
    read as uint8); a YOLO11 Segment head (depthwise class branch), with or without yolo11=True."""

    _segment_ok = True

    def __init__(self, model, dtype=torch.bfloat16, hyp=None, device=None, world_size=1, ema=True, wgrad_streams: int = 1,
                 amp_scaler: bool = False, optimizer: str = "SGD", iterations=None, yolo11: bool = False, overlap_mask: bool = True):
        tail = model.model[-1] if hasattr(model, "model") and len(model.model) else None
        if not isinstance(tail, H.Segment):
            raise L.UpaError(f"SegmentationTrainer needs a model that ends in a Segment head, got {type(tail).__name__}")
        if not overlap_mask:
            raise L.UpaError("overlap_mask=False (one mask plane per instance) has no training path on HIP: the mask loss reads the "
                             "overlap mask (overlap_mask=True, the reference's default)")
        if not tail.legacy_cls:
            if not yolo11:
                raise L.UpaError("Segment (YOLO11, non-legacy head with a depthwise class branch) has no training path on HIP unless it is "
                                 "asked for with yolo11=True - and SegmentationTrainer does not build it yet")
            raise L.UpaError("Segment (YOLO11, non-legacy head with a depthwise class branch): SegmentationTrainer builds the yolov8 "
                             "Segment head only")
        ConvTransposeT.check(tail.proto.upsample, f"model.{getattr(tail, 'i', '?')}.proto.upsample")
        self.masks_d = self.mid_d = None
        super().__init__(model, dtype=dtype, hyp=hyp, device=device, world_size=world_size, ema=ema, wgrad_streams=wgrad_streams,
                         amp_scaler=amp_scaler, optimizer=optimizer, iterations=iterations, yolo11=yolo11)

    def _tail_op(self, m, name):
        if isinstance(m, H.Segment):
            return SegmentT(self.ctx, m, name, self), "detect"
        return None

    @staticmethod
    def check_masks(labels, batch_size, mh, mw):
        """The refusals of the label upload, on the host: returns the (B, mh, mw) uint8 overlap mask."""
        if not isinstance(labels, dict) or "masks" not in labels:
            raise L.UpaError('segmentation labels need "masks": the (B, mh, mw) overlap mask at prototype resolution')
        masks = torch.as_tensor(labels["masks"]).detach().cpu()
        if masks.dim() != 3 or masks.shape[0] != batch_size:
            raise L.UpaError(f"masks of shape {tuple(masks.shape)} for a batch of {batch_size} images: the overlap mask is (B, mh, mw) "
                             "(overlap_mask=False stacks, one plane per instance, are not built)")
        if tuple(masks.shape[-2:]) != (mh, mw):
            raise L.UpaError(f"masks are {tuple(masks.shape[-2:])} but the prototypes are {(mh, mw)}: masks must come at prototype "
                             "resolution (mask_ratio=4, the reference's dataset default); the F.interpolate fallback is not built")
        if masks.numel():
            lo, hi = float(masks.min()), float(masks.max())
            if lo < 0 or hi > MASK_ID_MAX or (masks.dtype.is_floating_point and bool((masks != masks.round()).any())):
                raise L.UpaError(f"mask values span [{lo:g}, {hi:g}]: instance ids must be integers in [0, {MASK_ID_MAX}] (the mask loss "
                                 "reads the overlap mask as uint8)")
        return masks.to(torch.uint8).contiguous()

    def _upload_labels(self, labels, batch_size):
        imgsz_h, imgsz_w = self._imgsz
        s0 = float(self.detect.m.stride[0])
        mh, mw = int(imgsz_h / s0) * 2, int(imgsz_w / s0) * 2  # Proto doubles level 0's map
        masks = self.check_masks(labels, batch_size, mh, mw)
        # every refusal comes before anything is uploaded: the ids are packed (into as many rows as the image with the most labels has)
        # and checked first, then the gt rows go up, then the ids are laid out in the gt buffer's row count
        bi = labels["batch_idx"].view(-1).cpu().long()
        most = max([int((bi == j).sum()) for j in range(batch_size)] + [1])
        mid0 = pack_mask_ids(labels, batch_size, imgsz_h, imgsz_w, most)
        if int(mid0.max()) > MASK_ID_MAX:
            raise L.UpaError(f"an image has a label at position {int(mid0.max())}: instance ids above {MASK_ID_MAX} do not fit the uint8 "
                             "overlap mask")
        super()._upload_labels(labels, batch_size)
        rows = int(self.gt_d.shape[1])
        mid = torch.zeros(batch_size, rows, dtype=torch.int32)
        mid[:, :min(rows, most)] = mid0[:, :rows]
        if self.masks_d is None or tuple(self.masks_d.shape) != tuple(masks.shape) or tuple(self.mid_d.shape) != tuple(mid.shape):
            if self._graphs is not None or self._capturing:
                raise L.UpaError(f"masks {tuple(masks.shape)} / {rows} gt rows do not match the compiled step's buffers")
            self.masks_d = torch.zeros(tuple(masks.shape), dtype=torch.uint8, device=self.device)
            self.mid_d = torch.zeros(tuple(mid.shape), dtype=torch.int32, device=self.device)
        # through a ring of pinned staging buffers, each guarded by the event of its last copy, as the gt rows go
        ring = self.__dict__.setdefault("_mask_ring", [None] * 4)
        self._mask_slot = (self.__dict__.get("_mask_slot", -1) + 1) % len(ring)
        ent = ring[self._mask_slot]
        if ent is None or ent[0].shape != masks.shape or ent[1].shape != mid.shape:
            ent = [torch.zeros(tuple(masks.shape), dtype=torch.uint8).pin_memory(), torch.zeros(tuple(mid.shape), dtype=torch.int32).pin_memory(),
                   None]
            ring[self._mask_slot] = ent
        if ent[2] is not None:
            ent[2].synchronize()
        ent[0].copy_(masks)
        ent[1].copy_(mid)
        self.masks_d.copy_(ent[0], non_blocking=True)
        self.mid_d.copy_(ent[1], non_blocking=True)
        ent[2] = torch.cuda.Event()
        ent[2].record(torch.cuda.current_stream(self.device))
