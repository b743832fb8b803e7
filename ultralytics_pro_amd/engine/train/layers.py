"""Train-mode forward / backward of the backbone and neck modules, all of it upa_* kernels (include/upa.h, "training step").

  Conv (conv -> BN(batch statistics) -> SiLU):  z = conv(x, W);  (mean, var) = stats(z);  y = act(bn(z)) (+ residual)
      backward: dz, dgamma, dbeta = bn_act_bwd(z, dy);  dW += wgrad(x, dz);  dx (+)= conv(dz, W^T flipped)
  C2f / Bottleneck / SPPF / C3 / BoT3 / C3k2 / C2PSA / Proto / Upsample: compositions of the above + pool / upsample / attention kernels.

The op protocol of the training graph (`trainer.DetectionTrainer._build_graph`): `convs()` the packable convs, `cout` the output
channels, `out_hw(h, w)` the output size, `forward(x, out=None)`, `backward(dy, dx, accumulate)`."""

from __future__ import annotations

import torch
import torch.nn as nn

from ... import _lib as L
from ...nn.modules import block as B
from ...nn.modules import conv as CV
from .. import runtime as R
from .ctx import _Ctx, _new, _residual, _s, add_into


class _Block:
    """The protocol's default for every op that keeps the map size."""

    def out_hw(self, h, w):
        return h, w


class ConvT(_Block):
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

    @classmethod
    def from_module(cls, ctx: _Ctx, m: CV.Conv, name: str, **kw):
        """The op of a `Conv` module (conv + BatchNorm2d + its activation)."""
        return cls(ctx, m.conv, m.bn, m._act_code(), name, **kw)

    def convs(self):
        return [self]

    def out_hw(self, h, w):
        return (h + 2 * self.p - self.k) // self.s + 1, (w + 2 * self.p - self.k) // self.s + 1

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
        rp, rld = _residual(residual)
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
        oh, ow = self.out_hw(h, w)
        self.x = x
        if self.bn is None:  # plain nn.Conv2d with bias: y = conv(x) + b
            y = out if out is not None else _new(n, self.cout, oh, ow, c.dtype, c.device, (id(self), "y"))
            self._conv(x, self.wp, self.cout, self.k, self.s, self.p, y, bias=self.conv.bias)
            return y
        z = _new(n, self.cout, oh, ow, c.dtype, c.device, (id(self), "z"))
        vx, vz = R.view_of(x), R.view_of(z)
        bn = self.bn
        # conv + batch statistics + normalisation / activation in ONE call: on the kernels with a statistics epilogue the sums come from
        # the convolution's own workgroups (no pass over z), elsewhere the library runs conv -> reduce -> combine itself
        y = out if out is not None else _new(n, self.cout, oh, ow, c.dtype, c.device, (id(self), "y"))
        vy = R.view_of(y)
        rp, rld = _residual(residual)
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
                side, ws = c._next_wgrad_stream()
                side_p = side.cuda_stream
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
        if c.wgrad_streams:
            side, ws = c._next_wgrad_stream()
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(c.device))  # dz is ready
            side.wait_event(ev)
            wst = side.cuda_stream
        else:
            ws, wst = c.wgrad_ws_here, st
        L.check(lib.upa_conv2d_wgrad(vx.ptr, vx.n, vx.h, vx.w, self.cin, vx.ld, vdz.ptr, self.cout, vdz.ld,
                                     self.conv.weight.grad.data_ptr(), self.k, self.s, self.p, 1, vx.dtype,
                                     ws.data_ptr(), ws.numel(), wst), f"wgrad[{self.name}]")
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


class PadConvT(ConvT):
    """`ConvT` of a conv whose input and / or output channels are no multiple of the kernels' 16-byte channel group (the Pose head's
    51-channel cv4 chain): the kernels run at the channel counts rounded up to `pad` and the op owns zero-padded f32 STAGING of every
    tensor they read or write at that width - the weight, gamma, beta, the running statistics (the plain last conv: the bias) and
    their gradients.  The module's parameters and buffers keep their shapes, so the state_dict and the trainer's flat layout do not
    change.  Once per step, for every padded op of the model together (`pad_descs`, upa_pad_copy_batched):
      gather   before the repack: staging = masters, zeros in the pad; gradient staging = zeros;
      scatter  after the backward: master gradients += the staging's real rows; running statistics copied back.
    Pad filters, biases and gamma / beta are zero, so pad activations are act(0) = 0 and pad gradients are exact zeros as long as the
    gradient that enters the chain has zero pad columns (upa_kpt_loss writes them)."""

    def __init__(self, ctx: _Ctx, conv: nn.Conv2d, bn, act_code: int, name: str, pad_cin: bool = True, pad_cout: bool = True, pad: int = 8):
        from types import SimpleNamespace as NS
        up = (lambda v, on: (v + pad - 1) // pad * pad if on else v)
        self.real = (conv.out_channels, conv.in_channels)
        co, ci = up(conv.out_channels, pad_cout), up(conv.in_channels, pad_cin)
        kk = conv.kernel_size[0] * conv.kernel_size[1]
        dev = ctx.device
        self._descs = []

        def staged(master, shape, real, flags, grad=True):
            """A zero staging tensor of `shape` for `master` (viewed as `real` = (rows, cols, inner)) with its gradient staging."""
            t = torch.zeros(shape, dtype=torch.float32, device=dev)
            prows, pcols = (shape[0], shape[1]) if len(shape) > 1 else (shape[0], 1)
            self._descs.append((master.data_ptr(), t.data_ptr()) + real + (prows, pcols, flags))
            if grad:
                t.grad = torch.zeros(shape, dtype=torch.float32, device=dev)
                self._descs.append((master.grad.data_ptr(), t.grad.data_ptr()) + real + (prows, pcols, L.UPA_PAD_SCATTER_ADD))
            return t

        w = staged(conv.weight, (co, ci) + tuple(conv.kernel_size), self.real + (kk,), L.UPA_PAD_GATHER)
        vec = (lambda p, flags=L.UPA_PAD_GATHER, grad=True: staged(p, (co,), (conv.out_channels, 1, 1), flags, grad))
        sconv = NS(weight=w, bias=None if conv.bias is None else vec(conv.bias), groups=conv.groups, dilation=conv.dilation,
                   kernel_size=conv.kernel_size, stride=conv.stride, padding=conv.padding, out_channels=co, in_channels=ci)
        sbn = None
        if bn is not None:
            back = L.UPA_PAD_GATHER | L.UPA_PAD_SCATTER_COPY
            sbn = NS(weight=vec(bn.weight), bias=vec(bn.bias), running_mean=vec(bn.running_mean, back, False),
                     running_var=vec(bn.running_var, back, False), eps=bn.eps, momentum=bn.momentum)
        self.module_conv, self.module_bn = conv, bn
        super().__init__(ctx, sconv, sbn, act_code, name)

    def pad_descs(self):
        """(master, padded, rows, cols, inner, padded rows, padded cols, flags) of every staged tensor: the rows of `UpaPadDesc`."""
        return list(self._descs)

    def staging(self):
        """{name: (padded tensor, real rows, real columns)} of everything staged, gradients included (tests, debugging)."""
        co, ci = self.real
        out = {"weight": (self.conv.weight, co, ci), "weight.grad": (self.conv.weight.grad, co, ci)}
        vecs = {"bias": self.conv.bias} if self.bn is None else {"bn.weight": self.bn.weight, "bn.bias": self.bn.bias,
                                                                  "bn.running_mean": self.bn.running_mean,
                                                                  "bn.running_var": self.bn.running_var}
        for k, t in vecs.items():
            out[k] = (t, co, 1)
            if getattr(t, "grad", None) is not None:
                out[k + ".grad"] = (t.grad, co, 1)
        return out


def pad_table(ops, device):
    """The device descriptor table (`UpaPadDesc` rows) of the padded ops among `ops`, and its length; (None, 0) without one."""
    import numpy as np
    rows = [d for op in ops if isinstance(op, PadConvT) for d in op.pad_descs()]
    if not rows:
        return None, 0
    t = np.zeros(len(rows), dtype=np.dtype([("master", "<u8"), ("padded", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("inner", "<i4"),
                                            ("prows", "<i4"), ("pcols", "<i4"), ("flags", "<i4")]))
    for i, r in enumerate(rows):
        t[i] = r
    return torch.from_numpy(t.view(np.uint8).copy()).to(device), len(rows)


def pad_copy(table, n, scatter: bool, device):
    """One launch over the table: gather (masters -> staging, zeros in the pad and in the gradient staging) or scatter (staged
    gradients added to the masters', running statistics copied back)."""
    if n:
        L.check(L.lib().upa_pad_copy_batched(table.data_ptr(), n, int(scatter), _s(device)), "pad_copy_batched")


class DWConvT(_Block):
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


class ConvTransposeT(_Block):
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

    def out_hw(self, h, w):
        return 2 * h, 2 * w

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


class UpsampleT(_Block):
    """Train-mode nn.Upsample(scale_factor=2, mode="nearest"): upa_upsample2x / upa_upsample2x_bwd.  No parameters; `cout` is its
    input's.  `y_key`: the buffer-pool key of an output it allocates itself (the graph gives it the node's)."""

    def __init__(self, ctx: _Ctx, cout: int):
        self.ctx, self.cout = ctx, cout
        self.y_key = (id(self), "y")

    def convs(self):
        return []

    def out_hw(self, h, w):
        return 2 * h, 2 * w

    def forward(self, x, out=None):
        c = self.ctx
        n, ch, h, w = x.shape
        y = out if out is not None else _new(n, ch, 2 * h, 2 * w, c.dtype, c.device, self.y_key)
        vs, vd = R.view_of(x), R.view_of(y)
        L.check(L.lib().upa_upsample2x(vs.ptr, vs.n, vs.h, vs.w, vs.c, vs.ld, vd.ptr, vd.ld, vs.dtype, _s(c.device)), "upsample2x")
        return y

    def backward(self, dy, dx, accumulate):
        vdy, vdx = R.view_of(dy), R.view_of(dx)
        L.check(L.lib().upa_upsample2x_bwd(vdy.ptr, vdx.n, vdx.h, vdx.w, vdx.c, vdy.ld, vdx.ptr, vdx.ld, int(accumulate), vdx.dtype,
                                           _s(self.ctx.device)), "upsample2x_bwd")


class BottleneckT(_Block):
    def __init__(self, ctx, m: B.Bottleneck, name):
        self.ctx = ctx
        self.cv1 = ConvT.from_module(ctx, m.cv1, name + ".cv1")
        self.cv2 = ConvT.from_module(ctx, m.cv2, name + ".cv2")
        self.cout = self.cv2.cout
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


class C2fT(_Block):
    def __init__(self, ctx, m: B.C2f, name):
        self.ctx = ctx
        self.c = m.c
        self.cv1 = ConvT.from_module(ctx, m.cv1, name + ".cv1")
        self.cv2 = ConvT.from_module(ctx, m.cv2, name + ".cv2")
        self.cout = self.cv2.cout
        self.m = [self._inner(ctx, b, f"{name}.m.{i}") for i, b in enumerate(m.m)]

    def _inner(self, ctx, b, name):
        return BottleneckT(ctx, b, name)

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


class SPPFT(_Block):
    def __init__(self, ctx, m: B.SPPF, name):
        self.ctx = ctx
        self.cv1 = ConvT.from_module(ctx, m.cv1, name + ".cv1")
        self.cv2 = ConvT.from_module(ctx, m.cv2, name + ".cv2")
        self.cout = self.cv2.cout
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


class C3T(_Block):
    """Train-mode C3 / C3k (block.py:237-262, :1510-1530): cv3(cat(m(cv1(x)), cv2(x))).  cv2 and the last inner Bottleneck write their
    halves of one concat buffer; the gradient of the buffer is sliced the same way."""

    def __init__(self, ctx, m: B.C3, name):
        self.ctx = ctx
        self.cv1 = ConvT.from_module(ctx, m.cv1, name + ".cv1")
        self.cv2 = ConvT.from_module(ctx, m.cv2, name + ".cv2")
        self.cv3 = ConvT.from_module(ctx, m.cv3, name + ".cv3")
        self.cout = self.cv3.cout
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


class C3k2T(C2fT):
    """Train-mode C3k2 (block.py:1485-1507): C2f's graph with Bottleneck(c, c, e=0.5) (c3k=False) or C3k(c, c, 2) (c3k=True) inside."""

    def _inner(self, ctx, b, name):
        if isinstance(b, B.C3):
            return C3T(ctx, b, name)
        if isinstance(b, B.Bottleneck):
            return BottleneckT(ctx, b, name)
        raise L.UpaError(f"{name}: {type(b).__name__} inside a C3k2 has no training path on HIP")


class ProtoT(_Block):
    """Train-mode Proto (block.py:257-276): cv3(cv2(upsample(cv1(x))))."""

    def __init__(self, ctx, m: B.Proto, name):
        self.ctx = ctx
        self.cv1 = ConvT.from_module(ctx, m.cv1, name + ".cv1")
        self.up = ConvTransposeT(ctx, m.upsample, name + ".upsample")
        self.cv2 = ConvT.from_module(ctx, m.cv2, name + ".cv2")
        self.cv3 = ConvT.from_module(ctx, m.cv3, name + ".cv3")
        self.cout = self.cv3.cout

    def convs(self):
        return [self.cv1, self.up, self.cv2, self.cv3]

    def out_hw(self, h, w):
        return 2 * h, 2 * w

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
