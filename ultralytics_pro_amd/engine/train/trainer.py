"""The trainers: flat parameter buffers, the graph walk (forward, loss, backward), the gradient exchange, the fused optimizer step and
the hipGraph capture / replay of the whole step."""

from __future__ import annotations

import math

import numpy as np

import torch
import torch.nn as nn

from ... import _lib as L
from ...nn.modules import block as B
from ...nn.modules import conv as CV
from ...nn.modules import head as H
from ...nn.modules import resample as RS
from .. import runtime as R
from .attention import BoT3T, C2PSAT
from .ctx import PinnedRing, _Ctx, _new, _s, add_into, copy_into
from .graph import _Node, plan_concats
from .heads import ClassifyT, DetectT, PoseT, SegmentT
from .layers import C2fT, C3k2T, C3T, ConvT, ConvTransposeT, DWConvT, SPPFT, UpsampleT, pad_copy, pad_table
from .optim import HYP, SCHED, GradScaler, _head_nc, resolve_optimizer
from .targets import MASK_ID_MAX, MAX_GT, MAX_GT_CAP, pack_cls_targets, pack_keypoints, pack_mask_ids, pack_targets

# (module type, op type) of the composite layers, first match wins: a subclass stands in front of its base (C3k2 is a C2f, BoT3 a C3)
_BLOCK_OPS = ((B.C3k2, C3k2T), (B.C2PSA, C2PSAT), (B.C2f, C2fT), (B.BoT3, BoT3T), (B.C3, C3T), (B.SPPF, SPPFT))


class DetectionTrainer:
    """One-process-per-GPU trainer for a DetectionModel (reference: engine/trainer.py BaseTrainer._do_train inner loop).
    `optimizer`: "SGD" (default: SGD-Nesterov), "Adam", "AdamW" (lr and beta1 = `momentum` from `hyp`, plus `beta2`, `adam_eps`) or
    "auto" with `iterations` (`resolve_optimizer`); `optimizer_name` is the resolved one."""

    tail_type, tail_op = H.Detect, DetectT  # the head that ends the model and its op: H.Detect itself here, a trainer of another task names its own
    _OTHER_TAILS = ((H.Segment, "segmentation models (Segment head) have no training path on HIP in DetectionTrainer (v8DetectionLoss only): "
                                "train them with SegmentationTrainer"),
                    (H.Pose, "pose models (Pose head) have no training path on HIP in DetectionTrainer (v8DetectionLoss only): pose "
                             "training (v8PoseLoss) is PoseTrainer's"))

    def __init__(self, model, dtype=torch.bfloat16, hyp=None, device=None, world_size=1, ema=True, wgrad_streams: int = 1,
                 amp_scaler: bool = False, optimizer: str = "SGD", iterations=None, yolo11: bool = False):
        self.optimizer_name, opt_hyp, self._auto_optimizer = resolve_optimizer(
            optimizer, iterations, _head_nc(model) if str(optimizer).lower() == "auto" and iterations is not None else 0)
        for head, refusal in self._OTHER_TAILS:  # a head with an extra branch trains under the trainer that names it
            if not issubclass(self.tail_type, head) and any(isinstance(m, head) for m in model.modules()):
                raise L.UpaError(refusal)
        # the non-legacy Detect head (YOLO11: depthwise class branch, `DWConvT`) trains on request only: `yolo11=True`
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
        self._buckets = None      # enable_overlapped_allreduce(): the bucketed exchange and the waits it exposed
        self._exposed = []
        self._imgsz = None
        self._img_zeroed = set()  # input buffers whose pad channels are zero (`_input_nhwc`)
        self._label_ring = PinnedRing()
        self.gt_d = self.ngt_d = None
        self.schedule = None      # set_schedule(): warm-up interpolation + gradient accumulation of the reference's loop
        self.ni = 0               # iteration counter (the reference's `ni = i + nb * epoch`)
        self.last_opt_step = -1   # trainer.py:386
        self._pad_tab, self._pad_n = None, None  # the descriptor table of the padded convs (`PadConvT`), built at the first step
        self.max_gt = MAX_GT  # rows per image of the padded gt tensor (the reference pads to counts.max(), loss.py:445-461)
        model.to(self.device)
        self._flatten_parameters(ema)
        self._build_graph()

    # ---- parameters ---------------------------------------------------------------------------------------------------
    def _flatten_parameters(self, ema):
        """Flat f32 buffers [biases | decayed weights | norm weights] with model.parameters() viewing into them (grouped as the
        reference's build_optimizer groups them, trainer.py:917-926, so the optimizer is three fused launches; the state_dict stays the
        reference's)."""
        from ...parallel import flat_parameter_layout
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
        """One `_Node` per model layer: its op (`layers`' protocol; the last node's is the tail, `_tail_op`; a Concat has none) and its
        output channels."""
        ctx = self.ctx
        self.nodes = []
        self.convs = []
        self._pack_table, self._pack_n = None, 0
        cout = {}
        for m in self.model.model:
            name = f"model.{m.i}"
            src = (lambda j: j if j != -1 else m.i - 1)
            op, co = self._tail_op(m, name), None  # (the tail has no `cout`: nothing reads its output but its own loss)
            if op is not None:
                pass
            elif isinstance(m, CV.Concat):
                co = sum(cout[src(j)] for j in m.f)
            else:
                op = self._layer_op(m, name, cout.get(src(m.f)) if isinstance(m.f, int) else None)
                co = op.cout
            if op is not None:
                self.convs += op.convs()
            cout[m.i] = co
            nd = _Node(m.i, m.f, op, co)
            if isinstance(op, UpsampleT):
                op.y_key = (id(nd), "y")  # its own output lives under the node's buffer key, as the Concat's does
            self.nodes.append(nd)
        self.detect = self.nodes[-1].op
        self._cat_slot = plan_concats([(nd.i, nd.f, nd.cout, nd.op is not None) for nd in self.nodes])

    def _layer_op(self, m, name, cin):
        """The op of a layer that is neither the tail nor a Concat; `cin`: the channels of its (single) input."""
        if not isinstance(m, B.C3k):  # (C3k: a C3 subclass that only lives inside a C3k2)
            for module_type, op_type in _BLOCK_OPS:
                if isinstance(m, module_type):
                    return op_type(self.ctx, m, name)
            if isinstance(m, CV.Conv):
                return ConvT.from_module(self.ctx, m, name, no_dgrad=(m.i == 0 and m.f == -1))
            if isinstance(m, RS.Upsample):
                return UpsampleT(self.ctx, cin)
        raise L.UpaError(f"{type(m).__name__} (layer {m.i}) has no training path on HIP yet")

    def _tail_op(self, m, name):
        """The op of the module that ends the graph and owns the loss (`forward(x)`, `loss_backward(labels, batch_size)`), None for
        every other module: `tail_op` for a `tail_type`.  (`ClassificationTrainer` overrides the hook.)"""
        if isinstance(m, self.tail_type):
            return self.tail_op(self.ctx, m, name, self)
        return None

    # ---- one step -----------------------------------------------------------------------------------------------------
    def _input_nhwc(self, img):
        """(N,3,H,W) f32 NCHW image batch -> NHWC view padded to one 16-byte channel group (pad channels stay zero)."""
        n, c, h, w = img.shape
        E = self.ctx.E
        buf = self.pool.get(("img", n, h, w), (n, h, w, E), self.dtype, self.device)
        if (n, h, w) not in self._img_zeroed:
            buf.zero_()  # one-time: the pad channels are never written again
            self._img_zeroed.add((n, h, w))
        L.check(L.lib().upa_nchw_to_nhwc(img.data_ptr(), n, c, h, w, buf.data_ptr(), E, self.ctx.code, _s(self.device)),
                "nchw_to_nhwc")
        return buf.permute(0, 3, 1, 2)

    # the padded convs' staging (`PadConvT`: a Pose head's cv4 chains, the class branch of a head whose nc is no 16-byte group): one
    # launch per direction and step; a model without one launches nothing
    def _pad_table(self):
        if self._pad_n is None:
            self._pad_tab, self._pad_n = pad_table(self.convs, self.device)
        return self._pad_tab, self._pad_n

    def _pad_scatter(self):
        tab, n = self._pad_table()
        pad_copy(tab, n, True, self.device)

    def _pack_weights(self):
        """Repack every conv's master weights into the MFMA fragment layouts (forward, data gradient) - one launch for the
        whole model plus one per stride-2 conv (its four phase kernels).  The descriptor table is built once: the master
        weights are views of the flat parameter buffer and the packed buffers are owned by the layers."""
        tab, n = self._pad_table()
        pad_copy(tab, n, False, self.device)  # the staging the repack reads; the gradient staging starts the step at zero
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

    def _src(self, nd, j):
        """The node that input `j` of node `nd` names (-1: the node in front)."""
        return self.nodes[j] if j != -1 else self.nodes[nd.i - 1]

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
        tail = self.nodes[-1]
        with R.static_buffers(self.pool):
            self._pack_weights()
            x = self._input_nhwc(img.float().contiguous() if img.dtype != torch.float32 else img.contiguous())
            # the stem sees E input channels: 3 real + zero padding (the packed weights are zero there as well)
            ys = []
            for nd in self.nodes:
                xin = x if nd.f == -1 else (ys[nd.f] if isinstance(nd.f, int) else [x if j == -1 else ys[j] for j in nd.f])
                if nd is tail:  # Detect; Classify in ClassificationTrainer
                    y = nd.op.forward(xin)
                elif nd.op is None:  # Concat
                    n, _, h, w = xin[0].shape
                    y = _new(n, sum(int(t.shape[1]) for t in xin), h, w, ctx.dtype, dev, (id(nd), "y"))
                    c0 = 0
                    for j, t in zip(nd.f, xin):
                        j = j if j != -1 else nd.i - 1
                        if self._cat_slot.get(j, (None,))[0] != nd.i:  # not written in place by its producer
                            copy_into(ctx, t, y[:, c0:c0 + t.shape[1]])
                        c0 += t.shape[1]
                else:
                    out = None
                    slot = self._cat_slot.get(nd.i)
                    if slot is not None:  # this layer's output lives in its slice of the Concat's buffer
                        cat_i, c0, cj, ctot = slot
                        n, _, h, w = xin.shape
                        h, w = nd.op.out_hw(h, w)
                        out = _new(n, ctot, h, w, ctx.dtype, dev, (id(self.nodes[cat_i]), "y"))[:, c0:c0 + cj]
                    y = nd.op.forward(xin, out=out)
                nd.y = y
                nd.g = None
                x = y
                ys.append(y)
            items = self.detect.loss_backward(labels, img.shape[0])
            self._bucket_hook(tail.i)
            # ---- backward over the layer list in reverse
            for nd in reversed(self.nodes[:-1]):
                if nd.g is None:
                    self._bucket_hook(nd.i)
                    continue  # output unused by the loss
                dy = nd.g
                if nd.op is None:  # Concat: route the slices of its gradient to its inputs
                    c0 = 0
                    for j in nd.f:
                        src = self._src(nd, j)
                        cj = int(src.y.shape[1])
                        if src.g is None:   # the Concat is the first consumer met: its slice IS the gradient buffer, later ones accumulate
                            src.g = dy[:, c0:c0 + cj]
                        else:
                            add_into(ctx, dy[:, c0:c0 + cj], src.g)
                        c0 += cj
                elif nd.i == 0:
                    nd.op.backward(dy, None, False)
                else:
                    dx, acc = self._grad_of(self._src(nd, nd.f))
                    nd.op.backward(dy, dx, acc)
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
        from ...parallel import gradient_bucket_table
        return gradient_bucket_table(self._param_meta, self.groups, target_bytes)

    def enable_overlapped_allreduce(self, target_bytes: int = 16 << 20):
        """Issue the gradient all-reduce per bucket DURING backward on a communication stream (eager steps only: a collective
        cannot sit inside the captured backward graph, so `compile()`d multi-GPU steps keep the single all-reduce between their
        two graphs).  Returns the bucket table [(first layer, [ranges])]."""
        from ...parallel import BucketedAllReduce
        table = self.gradient_buckets(target_bytes)
        self._bucket_first = {first: k for k, (first, _) in enumerate(table)}
        self._buckets = BucketedAllReduce(self.G, [r for _, r in table])
        ntot = self.groups[-1][0] + self.groups[-1][1]
        assert self._buckets.covered() == ntot, "gradient buckets must cover the flat buffer exactly once"
        self._exposed = []
        return table

    def _stream_events(self):
        """An event on the main stream and on every weight-gradient stream: what a bucket's all-reduce has to wait for."""
        evs = []
        for st in [torch.cuda.current_stream(self.device)] + list(self.ctx.wgrad_streams):
            ev = torch.cuda.Event()
            ev.record(st)
            evs.append(ev)
        return evs

    def _bucket_hook(self, layer_i: int):
        """Called by the backward walk after layer `layer_i` has enqueued its gradient kernels."""
        b = self._buckets
        if b is None or not self._issue_buckets or layer_i not in self._bucket_first:
            return
        b.issue(self._bucket_first[layer_i], self._stream_events())

    def all_reduce_gradients(self):
        """Batch-DP exchange step: SUM all-reduce of the flat f32 gradient buffer over RCCL - one collective, or
        the buckets `enable_overlapped_allreduce` issued during backward (then only the wait is left here, and the time the
        optimizer had to wait for them is recorded: `allreduce_exposed_ms`).
        The reference multiplies the loss by world_size and lets DDP average the gradients (trainer.py:424-425), i.e.
        every rank ends up with sum_over_ranks d(loss_rank) - exactly the SUM of the unscaled per-rank gradients."""
        if self.world_size > 1:
            b = self._buckets
            if b is not None and b.issued:
                main = torch.cuda.current_stream(self.device)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(main)
                # a span the walk never hooked (parameters outside `model.<N>.*`: layer -1, or a layer without gradient) goes now:
                # backward has finished on the HOST side only, so the communication stream is ordered behind the main stream and
                # every weight-gradient stream first, exactly as `_bucket_hook` does
                late = [k for k in range(len(b.buckets)) if k not in b.issued]
                if late:
                    evs = self._stream_events()
                    for k in late:
                        b.issue(k, evs)
                b.wait()
                e1.record(main)
                self._exposed.append((e0, e1))
                return
            from ...parallel import allreduce_gradients_
            n = self.groups[-1][0] + self.groups[-1][1]
            allreduce_gradients_(self.G[:n])

    def allreduce_exposed_ms(self):
        """Mean time (ms) the main stream spent waiting for the overlapped all-reduce after backward had finished, over the
        steps since the last call (None if nothing was recorded).  Synchronises."""
        ex = self._exposed
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
        """clip_grad_norm_(10) + the optimizer + EMA (engine/trainer.py:674-682, :891-950; utils/torch_utils.py:606-650) as one fused
        launch per parameter group: upa_sgd_nesterov_ema, or upa_adam_ema behind one upa_adam_step_advance (second-moment buffer `V`,
        step count on the device)."""
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
        # the staging buffer has gt_d's row count and only [:, :need] is overwritten (rows past an image's count are never read: n_gt
        # bounds them)
        h_gt, h_ngt = self._label_ring.stage([(self.gt_d.shape, torch.float32), ((batch_size,), torch.int32)])
        h_gt[:, :need].copy_(gt)
        h_ngt.copy_(ngt)
        self.gt_d.copy_(h_gt, non_blocking=True)
        self.ngt_d.copy_(h_ngt, non_blocking=True)
        self._label_ring.commit(torch.cuda.current_stream(self.device))

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
        from ...parallel import broadcast_
        if self.nbuf:
            if self.ERB is not None:
                broadcast_(self.ERB[:self.nbuf], src)
            broadcast_(self.RB[:self.nbuf], src)

    def broadcast_stop(self, stop: bool, src: int = 0) -> bool:
        """The early-stopping decision of rank `src` on every rank (engine/trainer.py:505-508): all ranks must leave the epoch loop
        together or the next collective hangs."""
        from ...parallel import broadcast_flag
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
            return ClassifyT(self.ctx, m, name, self)
        if isinstance(m, H.Detect):
            raise L.UpaError(f"{type(m).__name__} (layer {m.i}) is not a classification tail: use DetectionTrainer")
        return None

    def _upload_labels(self, labels, batch_size):
        cls = pack_cls_targets(labels, batch_size, self.detect.nc)
        if self.cls_d is None or self.cls_d.shape[0] != batch_size:
            if self._graphs is not None or self._capturing:
                raise L.UpaError(f"a batch of {batch_size} images but the compiled step holds {int(self.cls_d.shape[0])}")
            self.cls_d = torch.zeros(batch_size, dtype=torch.int32, device=self.device)
        (h_cls,) = self._label_ring.stage([((batch_size,), torch.int32)])
        h_cls.copy_(cls)
        self.cls_d.copy_(h_cls, non_blocking=True)
        self._label_ring.commit(torch.cuda.current_stream(self.device))


class ExtraLabelsTrainer(DetectionTrainer):
    """DetectionTrainer for a model whose head (`tail_type`) has an extra branch with a loss term of its own (`tail_op`) that reads more
    labels than the gt rows.  Everything but the tail and the labels is DetectionTrainer's: the graph walk, `step`, `compile` / replay,
    `set_schedule`, every optimizer, GradScaler, EMA and the multi-rank path.  The extra labels go up with the gt rows, through a pinned
    ring of their own, into the device buffers the tail op reads as attributes of the trainer.  Every refusal - the constructor's (a
    model that does not end in `tail_type`; a YOLO11 head, depthwise class branch, with or without yolo11=True: no golden pins it) and
    the label upload's (`_check_extra`, `_pack_extra`) - comes before any launch or upload.

    A subclass names `tail_type`, `tail_op` and `_yolo11_refusals` and states `_check_extra` and `_pack_extra`."""

    _yolo11_refusals = None  # (without yolo11=True, with it)

    def __init__(self, model, **kw):
        self._extra_ring = PinnedRing()  # the extra labels' staging, beside the gt rows' `_label_ring`
        super().__init__(model, **kw)

    def _checked_tail(self, model, yolo11: bool):
        """The model's tail, refused unless it is a yolov8 (legacy class branch) head of `tail_type`."""
        tail = model.model[-1] if hasattr(model, "model") and len(model.model) else None
        if not isinstance(tail, self.tail_type):
            raise L.UpaError(f"{type(self).__name__} needs a model that ends in a {self.tail_type.__name__} head, got {type(tail).__name__}")
        if not tail.legacy_cls:
            raise L.UpaError(self._yolo11_refusals[bool(yolo11)])
        return tail

    def _check_extra(self, labels, batch_size):
        """The host-side refusals of the extra labels; what it returns is handed to `_pack_extra`."""
        raise NotImplementedError

    def _pack_extra(self, labels, batch_size, most, checked):
        """[(name of the trainer's device buffer, host tensor, per_label)]: a per_label tensor is (B, most, ...), one row per label of
        the image with the most labels, and is laid out in the gt buffer's row count."""
        raise NotImplementedError

    def _upload_labels(self, labels, batch_size):
        # every refusal comes before anything is uploaded: the extra labels are checked and packed (into as many rows as the image with
        # the most labels has) first, then the gt rows go up, then the per-label tensors are laid out in the gt buffer's row count
        checked = self._check_extra(labels, batch_size)
        bi = labels["batch_idx"].view(-1).cpu().long()
        most = max([int((bi == j).sum()) for j in range(batch_size)] + [1])
        packed = self._pack_extra(labels, batch_size, most, checked)
        super()._upload_labels(labels, batch_size)
        rows = int(self.gt_d.shape[1])
        shapes = [(batch_size, rows) + tuple(t.shape[2:]) if per_label else tuple(t.shape) for _, t, per_label in packed]
        held = [getattr(self, name) for name, _, _ in packed]
        if any(d is None or tuple(d.shape) != s for d, s in zip(held, shapes)):
            if self._graphs is not None or self._capturing:
                raise L.UpaError(f"{' / '.join(name for name, _, _ in packed)} of shapes {shapes} ({rows} gt rows, {batch_size} images) do "
                                 f"not match the compiled step's buffers {[None if d is None else tuple(d.shape) for d in held]}")
            for (name, t, _), s in zip(packed, shapes):
                setattr(self, name, torch.zeros(s, dtype=t.dtype, device=self.device))
        hosts = self._extra_ring.stage([(s, t.dtype) for (_, t, _), s in zip(packed, shapes)])
        for h, (name, t, per_label) in zip(hosts, packed):
            if per_label:
                h[:, :min(rows, most)].copy_(t[:, :rows])
                h[:, min(rows, most):].zero_()  # (never read - n_gt bounds the rows - but a reused slot must not carry an earlier batch)
            else:
                h.copy_(t)
            getattr(self, name).copy_(h, non_blocking=True)
        self._extra_ring.commit(torch.cuda.current_stream(self.device))


class PoseTrainer(ExtraLabelsTrainer):
    """One-process-per-GPU trainer for a PoseModel (reference: models/yolo/pose/train.py on engine/trainer.py's loop; the loss is
    v8PoseLoss, utils/loss.py:712-870).  The tail is `PoseT`; the labels additionally carry `"keypoints"`, (n_labels, nkpt, ndim)
    normalised [x, y(, visibility)] in the rows of `"bboxes"` (device buffer `kpt_d`).  The gains `pose` (12.0) and `kobj` (1.0) join the
    hyper-parameters here.  `step()` returns the (5,) loss items (box, pose, kobj, cls, dfl).
    The cv4 chains' 51 channels train on `PadConvT`'s zero-padded staging: one gather launch in front of the weight repack and one
    scatter launch behind the head's backward, both inside the captured step.
    Refused by the label upload: labels without "keypoints"; a keypoint tensor that is not (n_labels, *kpt_shape); non-finite
    keypoints."""

    tail_type, tail_op = H.Pose, PoseT
    _yolo11_refusals = ("Pose (YOLO11, non-legacy head with a depthwise class branch): PoseTrainer builds the yolov8 Pose head only, "
                        "with or without yolo11=True - no golden record pins a YOLO11 pose step",) * 2
    POSE_HYP = dict(pose=12.0, kobj=1.0)  # cfg/default.yaml of the reference

    def __init__(self, model, dtype=torch.bfloat16, hyp=None, device=None, world_size=1, ema=True, wgrad_streams: int = 1,
                 amp_scaler: bool = False, optimizer: str = "SGD", iterations=None, yolo11: bool = False):
        self.kpt_shape = tuple(int(v) for v in self._checked_tail(model, yolo11).kpt_shape)
        self.kpt_d = None
        super().__init__(model, dtype=dtype, hyp=dict(self.POSE_HYP, **(hyp or {})), device=device, world_size=world_size, ema=ema,
                         wgrad_streams=wgrad_streams, amp_scaler=amp_scaler, optimizer=optimizer, iterations=iterations, yolo11=yolo11)

    @staticmethod
    def check_keypoints(labels, kpt_shape):
        """The refusals of the label upload, on the host: returns the (n_labels, nkpt, ndim) float32 keypoints."""
        if not isinstance(labels, dict) or "keypoints" not in labels:
            raise L.UpaError('pose labels need "keypoints": (n_labels, nkpt, ndim) normalised [x, y(, visibility)]')
        kp = torch.as_tensor(labels["keypoints"]).detach().cpu().float()
        n = int(labels["bboxes"].view(-1, 4).shape[0])
        if tuple(kp.shape) != (n,) + tuple(kpt_shape):
            raise L.UpaError(f"keypoints of shape {tuple(kp.shape)} for {n} labels of a model with kpt_shape {tuple(kpt_shape)}: "
                             f"expected {(n,) + tuple(kpt_shape)}")
        if not bool(torch.isfinite(kp).all()):
            raise L.UpaError("keypoints hold non-finite values")
        return kp

    def _check_extra(self, labels, batch_size):
        return self.check_keypoints(labels, self.kpt_shape)

    def _pack_extra(self, labels, batch_size, most, checked):
        return [("kpt_d", pack_keypoints(labels, batch_size, *self._imgsz, most, self.kpt_shape), True)]


class SegmentationTrainer(ExtraLabelsTrainer):
    """One-process-per-GPU trainer for a SegmentationModel (reference: models/yolo/segment/train.py on engine/trainer.py's loop; the loss
    is v8SegmentationLoss, utils/loss.py:531-709).  The tail is `SegmentT`; the labels additionally carry `"masks"`, the (B, mh, mw)
    overlap mask at prototype resolution (instance p of an image painted as p + 1, later instances over earlier ones - what the
    reference's dataset delivers with overlap_mask=True, mask_ratio=4): device buffers `masks_d` and, per gt row, the instance id
    `mid_d`.  `step()` returns the (4,) loss items (box, seg, cls, dfl).
    Refused as well: overlap_mask=False (per-instance mask stacks); masks that are not at prototype resolution (the reference's
    F.interpolate fallback, loss.py:604-605, is not built); instance ids above 255 (the mask is read as uint8)."""

    tail_type, tail_op = H.Segment, SegmentT
    _yolo11_refusals = ("Segment (YOLO11, non-legacy head with a depthwise class branch) has no training path on HIP unless it is "
                        "asked for with yolo11=True - and SegmentationTrainer does not build it yet",
                        "Segment (YOLO11, non-legacy head with a depthwise class branch): SegmentationTrainer builds the yolov8 "
                        "Segment head only")

    def __init__(self, model, dtype=torch.bfloat16, hyp=None, device=None, world_size=1, ema=True, wgrad_streams: int = 1,
                 amp_scaler: bool = False, optimizer: str = "SGD", iterations=None, yolo11: bool = False, overlap_mask: bool = True):
        tail = self._checked_tail(model, yolo11)
        if not overlap_mask:
            raise L.UpaError("overlap_mask=False (one mask plane per instance) has no training path on HIP: the mask loss reads the "
                             "overlap mask (overlap_mask=True, the reference's default)")
        ConvTransposeT.check(tail.proto.upsample, f"model.{getattr(tail, 'i', '?')}.proto.upsample")
        self.masks_d = self.mid_d = None
        super().__init__(model, dtype=dtype, hyp=hyp, device=device, world_size=world_size, ema=ema, wgrad_streams=wgrad_streams,
                         amp_scaler=amp_scaler, optimizer=optimizer, iterations=iterations, yolo11=yolo11)

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

    def _check_extra(self, labels, batch_size):
        imgsz_h, imgsz_w = self._imgsz
        s0 = float(self.detect.m.stride[0])
        return self.check_masks(labels, batch_size, int(imgsz_h / s0) * 2, int(imgsz_w / s0) * 2)  # Proto doubles level 0's map

    def _pack_extra(self, labels, batch_size, most, masks):
        mid = pack_mask_ids(labels, batch_size, *self._imgsz, most)
        if int(mid.max()) > MASK_ID_MAX:
            raise L.UpaError(f"an image has a label at position {int(mid.max())}: instance ids above {MASK_ID_MAX} do not fit the uint8 "
                             "overlap mask")
        return [("masks_d", masks, False), ("mid_d", mid, True)]
