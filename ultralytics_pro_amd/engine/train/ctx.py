"""Per-trainer scratch shared by all layers, the buffer / view helpers of the ops and the pinned staging ring of the label uploads."""

from __future__ import annotations

import torch

from ... import _lib as L
from .. import runtime as R


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
        self._wgrad_ws_level = None  # (`wgrad_ws_here`)
        # weight gradients run on a side stream (a parallel branch of the captured graph): a layer's dW only needs its
        # input and dz, so it overlaps the data-gradient / BN-backward chain of the layers in front of it
        # (wgrad_streams = 0: weight gradients on the main stream, no overlap - the A/B switch of that measurement)
        self.wgrad_streams = [torch.cuda.Stream(device=device) for _ in range(max(0, int(wgrad_streams)))]
        self.wgrad_wss = [self.wgrad_ws for _ in self.wgrad_streams]  # one partial-sum workspace per stream
        self.wgrad_rr = 0
        self.wgrad_pending = False

    @property
    def ws(self):
        return self._ws[self._ws_sel]

    @property
    def wgrad_ws_here(self):
        """The weight-gradient partial-sum workspace for a weight gradient launched on the CURRENT stream (`wgrad_streams = 0`): the main
        stream's, or - while `DetectT._fork_levels` runs the small Detect levels on the level stream - a second buffer of the same size:
        two streams must never write and reduce split-K partials in one buffer at the same time."""
        if self._ws_sel == 0:
            return self.wgrad_ws
        lv = self._wgrad_ws_level
        if lv is None or lv.numel() < self.wgrad_ws.numel():
            lv = self._wgrad_ws_level = torch.empty(self.wgrad_ws.numel(), dtype=torch.uint8, device=self.device)
        return lv

    def _next_wgrad_stream(self):
        """(side stream, its partial-sum workspace) of the next weight gradient, round robin; `_join_wgrad` has work from here on."""
        j = self.wgrad_rr % len(self.wgrad_streams)
        self.wgrad_rr += 1
        self.wgrad_pending = True
        return self.wgrad_streams[j], self.wgrad_wss[j]


def _new(n, c, h, w, dtype, dev, key):
    return R.alloc_nhwc(n, c, h, w, dtype, dev, key)


def _residual(t):
    """(pointer, pixel pitch) of an optional residual view: (None, 0) without one."""
    if t is None:
        return None, 0
    v = R.view_of(t)
    return v.ptr, v.ld


def add_into(ctx, src, dst):
    """dst += src (NHWC views)."""
    vs, vd = R.view_of(src), R.view_of(dst)
    L.check(L.lib().upa_add_view(vd.ptr, vd.ld, vs.ptr, vs.ld, vd.ptr, vd.ld, vd.n, vd.h, vd.w, vd.c, vd.dtype, _s(ctx.device)),
            "add_view")


def copy_into(ctx, src, dst):
    vs, vd = R.view_of(src), R.view_of(dst)
    L.check(L.lib().upa_copy_view(vs.ptr, vs.n, vs.h, vs.w, vs.c, vs.ld, vd.ptr, vd.ld, vs.dtype, _s(ctx.device)), "copy_view")


def _pinned_zeros(shape, dtype):
    return torch.zeros(shape, dtype=dtype).pin_memory()


class PinnedRing:
    """A ring of PINNED host staging slots for a per-step upload, each guarded by the event of its last copy: a copy from pageable
    memory makes the host wait for the stream, and the step's launches then trail the GPU by the time the packing + the copy took
    (0.45 ms of idle GPU per yolov8s step in the kernel trace, tools/experiments/r05_train_gaps.py).
      bufs = ring.stage([(shape, dtype), ...])   the next slot's zero-initialised host tensors, (re)allocated when the shapes differ
                                                 from the slot's, after its last copy has finished
      ... fill bufs, device.copy_(buf, non_blocking=True) ...
      ring.commit(stream)                        the slot is busy until what `stream` holds now has run
    `alloc(shape, dtype)` and `event()` are injectable, so the ring's bookkeeping runs without a device."""

    def __init__(self, slots: int = 4, alloc=_pinned_zeros, event=torch.cuda.Event):
        self._slots = [None] * slots  # [specs, host tensors, event of the last copy | None]
        self._at = -1
        self._alloc, self._event = alloc, event

    def stage(self, specs):
        specs = [(tuple(int(v) for v in shape), dtype) for shape, dtype in specs]
        self._at = (self._at + 1) % len(self._slots)
        ent = self._slots[self._at]
        if ent is None or ent[0] != specs:
            ent = self._slots[self._at] = [specs, [self._alloc(shape, dtype) for shape, dtype in specs], None]
        if ent[2] is not None:
            ent[2].synchronize()
        return ent[1]

    def commit(self, stream):
        ev = self._event()
        ev.record(stream)
        self._slots[self._at][2] = ev
