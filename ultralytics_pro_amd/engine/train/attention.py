"""Train-mode forward / backward of the attention blocks: yolov5-BoT3's MHSA (upa_mhsa_train_fwd / upa_mhsa_bwd) and YOLO11's C2PSA
(upa_psa_attention_train_fwd / _bwd, upa_dwconv2d_train_fwd / _bwd).  The op protocol is `layers`'."""

from __future__ import annotations

import torch
import torch.nn as nn

from ... import _lib as L
from ...nn.modules import block as B
from ...nn.modules import conv as CV
from .. import runtime as R
from .ctx import _new, _residual, _s, add_into, copy_into
from .layers import C3T, ConvT, _Block


MHSA_HEAD_DIMS = (4, 8, 16, 32, 64)  # the head widths upa_mhsa / upa_mhsa_train_fwd / upa_mhsa_bwd build


class MHSAT(_Block):
    """Train-mode MHSA (block.py:6020-6062): softmax(q^T k) applied to v, unscaled, (+ BottleneckTransformer's residual in the epilogue).
    forward:  query / key / value = three plain ConvT (bias, no BN) writing the channel slices [q | k | v] of one buffer ->
              upa_mhsa_train_fwd (y, lse).
    backward: upa_mhsa_bwd writes [dq | dk | dv] -> the three convs' backward, their data gradients accumulated into one dx.
    Saved: qkv and lse (D is recomputed by the kernel, so the output is not kept)."""

    def __init__(self, ctx, m: B.MHSA, name):
        self.ctx = ctx
        if getattr(m, "pos", False):
            raise L.UpaError(f"{name}: MHSA(pos_emb=True) has no training path on HIP")
        self.c, self.heads = m.query.out_channels, int(m.heads)
        self.cout = self.c
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
        rp, rld = _residual(residual)
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


class BottleneckTransformerT(_Block):
    """Train-mode BottleneckTransformer (block.py:6065-6092): x + MHSA(cv1(x)); the add is the attention kernel's epilogue, its gradient
    goes through `add_into` as in BottleneckT.  `fc1` is not part of the function (`DetectionTrainer._dead_parameters`)."""

    def __init__(self, ctx, m: B.BottleneckTransformer, name):
        self.ctx = ctx
        cv1 = getattr(m, "cv1", None)
        if not (isinstance(m, B.BottleneckTransformer) and isinstance(cv1, CV.Conv) and len(m.cv2) == 1 and isinstance(m.cv2[0], B.MHSA)
                and cv1.conv.kernel_size == (1, 1) and cv1.conv.stride == (1, 1)):
            raise L.UpaError(f"{name}: {type(m).__name__} outside the BoT3 configuration (1x1 cv1, one MHSA, stride 1) has no training path "
                             "on HIP")
        self.cv1 = ConvT.from_module(ctx, cv1, name + ".cv1")
        self.attn = MHSAT(ctx, m.cv2[0], name + ".cv2.0")
        self.cout = self.attn.cout
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


class AttentionT(_Block):
    """Train-mode v10_Attention (block.py:1668-1722): proj(softmax(scale q^T k) v + pe(v)) (+ the block's residual).
    forward:  qkv ConvT (no act) -> upa_psa_attention_train_fwd (o, lse) -> pe: upa_dwconv2d_train_fwd on each head's v slice of qkv
              (no gather copy) -> batch statistics -> upa_bn_act_fwd with o as its residual (t = o + bn(pe)) -> proj ConvT.
    backward: proj -> dt; dt is the gradient of BOTH o and pe's BatchNorm output (the sum node, no copy): upa_bn_act_bwd (pe's BN) ->
              upa_psa_attention_bwd writes dqkv -> upa_dwconv2d_bwd accumulates pe's data gradient into the dv slices and pe's weight
              gradient -> qkv ConvT.backward."""

    def __init__(self, ctx, m: B.v10_Attention, name):
        self.ctx = ctx
        self.heads, self.kd, self.hd, self.scale = m.num_heads, m.key_dim, m.head_dim, float(m.scale)
        if self.kd != 32 or self.hd != 64:
            raise L.UpaError(f"{name}: training supports key_dim 32 / head_dim 64 (every YOLO11 scale), got {self.kd} / {self.hd}")
        pe = m.pe
        if not (pe.conv.groups == pe.conv.in_channels == pe.conv.out_channels and pe.conv.kernel_size == (3, 3) and pe.conv.stride == (1, 1)
                and pe.conv.padding == (1, 1) and pe.conv.dilation == (1, 1) and pe.conv.bias is None and isinstance(pe.act, nn.Identity)):
            raise L.UpaError(f"{name}.pe: training supports a depthwise 3x3, stride 1, pad 1 conv + BatchNorm without activation, got {pe}")
        self.qkv = ConvT.from_module(ctx, m.qkv, name + ".qkv")
        self.proj = ConvT.from_module(ctx, m.proj, name + ".proj")
        self.cout = self.proj.cout
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


class PSABlockT(_Block):
    """Train-mode PSABlock (block.py:1724-1766): u = x + attn(x), y = u + ffn(u); both adds in the last conv's epilogue, their
    gradients through `add_into` as in BottleneckT."""

    def __init__(self, ctx, m: B.PSABlock, name):
        self.ctx = ctx
        self.attn = AttentionT(ctx, m.attn, name + ".attn")
        self.ffn = [ConvT.from_module(ctx, f, f"{name}.ffn.{i}") for i, f in enumerate(m.ffn)]
        self.cout = self.ffn[-1].cout
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


class C2PSAT(_Block):
    """Train-mode C2PSA (block.py:1829-1881): cv1 -> [a | b], b through the PSABlocks, cv2(cat(a, b')).  In train mode b must survive
    (the first block's qkv conv needs it for its weight gradient), so cv2 reads a second 2c buffer: the last block writes its b half,
    a is copied.  The gradient of that buffer is cv1's output gradient: its a half as it is, its b half rewritten by the blocks."""

    def __init__(self, ctx, m: B.C2PSA, name):
        self.ctx = ctx
        self.c = m.c
        self.cv1 = ConvT.from_module(ctx, m.cv1, name + ".cv1")
        self.cv2 = ConvT.from_module(ctx, m.cv2, name + ".cv2")
        self.cout = self.cv2.cout
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
