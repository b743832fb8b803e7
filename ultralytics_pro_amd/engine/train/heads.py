"""The tails of the training graph: the train-mode head, its loss and the gradient of both (`forward(xs)`, `loss_backward(labels,
batch_size)`).  A head reaches into its trainer for the nodes it routes gradients into, the buffer pool, the scaler and the labels."""

from __future__ import annotations

import ctypes as C

import torch

from ... import _lib as L
from ...nn.modules import head as H
from .. import runtime as R
from .ctx import _new, _s
from .layers import ConvT, DWConvT, PadConvT, ProtoT


def _branch(ctx, seq, name, op=ConvT, first=None):
    """Conv, Conv, nn.Conv2d: one yolov8 head branch (cv2 / legacy cv3 / cv4 of a level).  `op`: the conv op's type (`PadConvT` for a
    chain whose channels are no 16-byte multiple); `first`: keyword arguments of the first op alone (its input is the neck's map)."""
    return [op.from_module(ctx, seq[0], name + ".0", **(first or {})), op.from_module(ctx, seq[1], name + ".1"),
            op(ctx, seq[2], None, L.ACT_NONE, name + ".2")]


def _chain_backward(ctx, seq, dy, dx, acc, key):
    """Backward of a chain of ops from its output gradient dy: the inner gradients get one buffer per op input (`key + (j,)`), the first
    op writes (`acc`: accumulates) into dx."""
    g = dy
    for j in range(len(seq) - 1, 0, -1):
        vt = R.view_of(seq[j].x)
        d = _new(vt.n, vt.c, vt.h, vt.w, ctx.dtype, ctx.device, key + (j,))
        seq[j].backward(g, d, False)
        g = d
    seq[0].backward(g, dx, acc)


class DetectT:
    """Train-mode Detect (head.py:116-126 returns the raw per-level maps) + v8DetectionLoss + its gradient."""

    fork_levels = True  # (False: every level on the main stream, as before round 5 - the A/B switch)

    def __init__(self, ctx, m: H.Detect, name, trainer):
        self.ctx = ctx
        self.m, self.tr = m, trainer
        self.nl, self.nc, self.reg_max, self.no = m.nl, m.nc, m.reg_max, m.no
        # nc classes that are no 16-byte channel group of the trainer's dtype (a pose model's nc = 1), which the last conv's row stores
        # refuse: the class branch's last conv runs on `PadConvT` and the raw maps are `nop` channels wide - the loss reads and writes
        # the first `no` of each row, the rest stays zero.  Every nc the plain `ConvT` takes keeps it (nop = no).
        self.nop = 4 * m.reg_max + (m.nc + 7) // 8 * 8 if (m.legacy_cls and m.nc % ctx.E) else m.no
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
                        ops.append(ConvT.from_module(ctx, pw, f"{name}.{tag}.{i}.{j}.1"))
                    row.append(ops + [ConvT(ctx, seq[2], None, L.ACT_NONE, f"{name}.{tag}.{i}.2")])
                    continue
                ops = _branch(ctx, seq, f"{name}.{tag}.{i}")
                if tag == "cv3" and self.nop != self.no:
                    ops[-1] = PadConvT(ctx, seq[2], None, L.ACT_NONE, f"{name}.{tag}.{i}.2", pad_cin=False)
                row.append(ops)
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
            raw = _new(n, self.nop, h, w, c.dtype, dev, (id(self), "raw", i))
            for k, (seq, out) in enumerate(zip(self.br[i], (raw[:, :nb], raw[:, nb:]))):
                t = x
                for op in seq[:-1]:
                    t = op.forward(t)
                seq[-1].forward(t, out=out)
            self.raw[i] = raw
            if c.dtype == torch.float32:
                self.raw32[i] = raw
            else:  # the loss reads f32 maps
                r32 = _new(n, self.nop, h, w, torch.float32, dev, (id(self), "raw32", i))
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

    # the hooks of a head with more branches on the same level inputs (`ExtraDetectT`)
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
            if self.nop != self.no:
                grads32[-1].zero_()  # the loss writes `no` columns of each row: the pad columns feed the padded conv's backward as zeros
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
                _chain_backward(c, seq, dy, dx, acc or k > 0, (id(self), "d", i, k))
            self._level_more_bwd(i, dx)

        # as in the forward pass: the small levels' chains beside the 80 x 80 level's (they write the gradients of different neck outputs)
        self._fork_levels(lambda: level_bwd(0), lambda: [level_bwd(i) for i in range(1, nl)], nl > 1)
        if tr._pad_table()[1]:
            # the staged gradients and running statistics of the padded convs go back to the module's tensors once every weight
            # gradient of the head has been enqueued: behind the side streams, in front of the gradient buckets of the head's layer
            tr._join_wgrad()
            tr._pad_scatter()
        return items


class ExtraDetectT(DetectT):
    """Train-mode head with one more per-level branch: `DetectT` with, per level, the cv4 chain (Conv 3x3, Conv 3x3, Conv2d 1x1) on
    ops of `conv_op`, whose maps (`self.extra`) feed a second loss term.  That term (a subclass's `_more_losses`) runs on the detection
    loss's workspace - the per-anchor assignment is read in place -, writes the maps' gradients (`self.dextra`, buffers under
    `grad_key`) and its loss items between box and [cls, dfl]; cv4 backpropagates into the same neck gradients as cv2 / cv3."""

    conv_op, first = ConvT, None  # `_branch`'s op type and the first op's keyword arguments
    grad_key = None

    def __init__(self, ctx, m, name, trainer):
        super().__init__(ctx, m, name, trainer)
        self.cv4 = [_branch(ctx, seq, f"{name}.cv4.{i}", op=self.conv_op, first=self.first) for i, seq in enumerate(m.cv4)]
        self.extra = [None] * m.nl

    def convs(self):
        return super().convs() + [cv for seq in self.cv4 for cv in seq]

    def _level_more(self, i, x):
        t = x
        for op in self.cv4[i]:
            t = op.forward(t)
        self.extra[i] = t

    def _level_more_bwd(self, i, dx):
        _chain_backward(self.ctx, self.cv4[i], self.dextra[i], dx, True, (id(self), "d4", i))

    def _level_tables(self):
        """Fresh gradient buffers of the cv4 maps and the per-level tables an extra loss takes: (views of the maps, [maps, gradients,
        hs, ws, lds, ldds] as void pointers)."""
        c = self.ctx
        self.dextra = [_new(*[int(v) for v in t.shape], c.dtype, c.device, (id(self), self.grad_key, i)) for i, t in enumerate(self.extra)]
        vm, vd = [R.view_of(t) for t in self.extra], [R.view_of(t) for t in self.dextra]
        FP, IA = C.c_void_p * self.nl, C.c_int * self.nl
        tabs = [FP(*[v.ptr for v in vm]), FP(*[v.ptr for v in vd]), IA(*[v.h for v in vm]), IA(*[v.w for v in vm]),
                IA(*[v.ld for v in vm]), IA(*[v.ld for v in vd])]
        return vm, [C.cast(t, C.c_void_p) for t in tabs]  # (a cast keeps its array alive)

    def _loss_workspaces(self, loss: str, wsb, batch_size, n_anchors, max_gt):
        """(the per-anchor assignment inside the detection loss's workspace `wsb`, the workspace of upa_<loss>, its bytes)."""
        lib = L.lib()
        asg = lib.upa_detection_loss_assignment(wsb.data_ptr(), batch_size, n_anchors, max_gt)
        nws = getattr(lib, f"upa_{loss}_workspace_bytes")(batch_size, n_anchors)
        return asg, self.tr.pool.get((loss + "_ws", batch_size, n_anchors), (nws,), torch.uint8, self.ctx.device), nws

    def _items_out(self, k: int):
        """The (3 + k,) buffer of the step's loss items: the extra loss writes its k items at [1, 1 + k)."""
        return self.tr.pool.get((f"loss_items{3 + k}",), (3 + k,), torch.float32, self.ctx.device)

    def _splice_items(self, items, out):
        """box and [cls, dfl] of the detection `items` around the extra items of `out`."""
        lib, st, n = L.lib(), _s(self.ctx.device), int(out.numel())
        L.check(lib.upa_copy_rows(items.data_ptr(), 1, 1, 3, out.data_ptr(), n, st), "copy_rows")
        L.check(lib.upa_copy_rows(items.data_ptr() + 4, 1, 2, 3, out.data_ptr() + 4 * (n - 2), n, st), "copy_rows")
        return out


class SegmentT(ExtraDetectT):
    """Train-mode Segment (head.py:790-837 returns the raw maps, the mask coefficients and the prototypes) + v8SegmentationLoss
    (utils/loss.py:531-709) + its gradient: the cv4 chains end in nm coefficients and level 0's input also feeds `ProtoT`.  The mask
    term is upa_mask_loss; Proto backpropagates into level 0's neck gradient.  Loss items: (box, seg, cls, dfl)."""

    grad_key = "dmc"

    def __init__(self, ctx, m: H.Segment, name, trainer):
        super().__init__(ctx, m, name, trainer)
        self.nm = m.nm
        self.proto = ProtoT(ctx, m.proto, name + ".proto")
        self.p = None

    def convs(self):
        return super().convs() + self.proto.convs()

    def _level_more(self, i, x):
        super()._level_more(i, x)
        if i == 0:
            self.p = self.proto.forward(x)

    def _more_losses(self, items, wsb, batch_size, n_anchors, max_gt):
        c, tr, lib = self.ctx, self.tr, L.lib()
        dev = c.device
        vp = R.view_of(self.p)
        _, (coefs, dcoefs, hs, ws, lds, ldds) = self._level_tables()
        self.dp = _new(vp.n, vp.c, vp.h, vp.w, c.dtype, dev, (id(self), "dproto"))
        vdp = R.view_of(self.dp)
        masks_d, mid_d = tr.masks_d, tr.mid_d
        if tuple(masks_d.shape) != (batch_size, vp.h, vp.w) or tuple(mid_d.shape) != (batch_size, max_gt):
            raise L.UpaError(f"mask buffers {tuple(masks_d.shape)} / {tuple(mid_d.shape)} do not match the step: prototypes "
                             f"{(batch_size, vp.h, vp.w)}, gt rows {(batch_size, max_gt)}")
        asg, mws, nws = self._loss_workspaces("mask_loss", wsb, batch_size, n_anchors, max_gt)
        items4 = self._items_out(1)
        imgsz_h, imgsz_w = tr._imgsz
        L.check(lib.upa_mask_loss(vp.ptr, batch_size, vp.h, vp.w, self.nm, vp.ld, coefs, dcoefs, hs, ws, lds, ldds, self.nl,
                                  asg, 2, tr.gt_d.data_ptr(), tr.ngt_d.data_ptr(), max_gt, mid_d.data_ptr(), masks_d.data_ptr(),
                                  imgsz_h, imgsz_w, tr.hyp["box"], 1.0, tr.scaler.ptr(), items4.data_ptr() + 4, vdp.ptr, vdp.ld,
                                  mws.data_ptr(), nws, c.code, _s(dev)), "mask_loss")
        return self._splice_items(items, items4)  # (box, seg, cls, dfl), loss.py:541

    def _level_more_bwd(self, i, dx):
        super()._level_more_bwd(i, dx)
        if i == 0:
            self.proto.backward(self.dp, dx, True)


class PoseT(ExtraDetectT):
    """Train-mode Pose (head.py:1208-1273 returns the raw maps and the raw keypoint maps) + v8PoseLoss (utils/loss.py:712-870) + its
    gradient: the cv4 chains end in nk keypoint values and run on `PadConvT` - c4 and nk (51 for the 17 x 3 skeleton) are no 16-byte
    multiples, the chain runs at the channel counts rounded up to `Pose.PAD` with zero pad channels.  The keypoint terms are
    upa_kpt_loss; it reads the padded raw map in the trainer's dtype and writes zero pad columns, so every pad gradient of the chain is
    an exact zero.  Loss items: (box, pose, kobj, cls, dfl)."""

    conv_op, first = PadConvT, dict(pad_cin=False)
    grad_key = "dkp"

    def __init__(self, ctx, m: H.Pose, name, trainer):
        super().__init__(ctx, m, name, trainer)
        self.nkpt, self.ndim = (int(v) for v in m.kpt_shape)
        self.nk = self.nkpt * self.ndim
        from ...utils.metrics import OKS_SIGMA
        sig = OKS_SIGMA if tuple(m.kpt_shape) == (17, 3) else [1.0 / self.nkpt] * self.nkpt  # loss.py:720-722
        self.sigma = (C.c_float * self.nkpt)(*[float(v) for v in sig])

    def _more_losses(self, items, wsb, batch_size, n_anchors, max_gt):
        c, tr, lib = self.ctx, self.tr, L.lib()
        dev = c.device
        vk, (kpts, dkpts, hs, ws, lds, ldds) = self._level_tables()
        strides = (C.c_float * self.nl)(*[float(s) for s in self.m.stride])
        kpt_d = tr.kpt_d
        if kpt_d is None or tuple(kpt_d.shape) != (batch_size, max_gt, self.nkpt, 3):
            raise L.UpaError(f"keypoint buffer {None if kpt_d is None else tuple(kpt_d.shape)} does not match the step: "
                             f"{(batch_size, max_gt, self.nkpt, 3)}")
        asg, kws, nws = self._loss_workspaces("kpt_loss", wsb, batch_size, n_anchors, max_gt)
        items5 = self._items_out(2)
        L.check(lib.upa_kpt_loss(kpts, dkpts, hs, ws, lds, ldds, self.nl, batch_size, vk[0].c, self.nkpt, self.ndim, asg, 2,
                                 tr.gt_d.data_ptr(), tr.ngt_d.data_ptr(), max_gt, kpt_d.data_ptr(), C.cast(strides, C.c_void_p),
                                 C.cast(self.sigma, C.c_void_p), tr.hyp["pose"], tr.hyp["kobj"], 1.0, tr.scaler.ptr(),
                                 items5.data_ptr() + 4, kws.data_ptr(), nws, c.code, _s(dev)), "kpt_loss")
        return self._splice_items(items, items5)  # (box, pose, kobj, cls, dfl), loss.py:727


class ClassifyT:
    """Train-mode Classify (head.py:1523-1529 returns the raw logits) + v8ClassificationLoss (utils/loss.py:873-880) + its gradient:
    ConvT (in output-channel slices, `_conv_parts`) -> upa_global_avgpool_fwd -> upa_linear, then upa_cross_entropy_fwd_bwd -> upa_linear_bwd -> upa_global_avgpool_bwd ->
    ConvT.backward.  The pooled rows, the logits and their gradients are float32 in both trainer modes and the linear layer is exact
    float32 (as the inference head keeps it, `Classify` docstring); only the (B, 1280, h, w) activation and its gradient carry the
    trainer's dtype.  `Dropout(p = 0)` is the identity and never runs."""

    def __init__(self, ctx, m: H.Classify, name, trainer):
        self.ctx = ctx
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
            return [(0, cout, ConvT.from_module(ctx, cv, name))]

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
