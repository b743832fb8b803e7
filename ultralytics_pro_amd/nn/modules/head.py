"""Detection heads with the reference's operator API (ultralytics/nn/modules/head.py), on HIP kernels."""

from __future__ import annotations

import itertools
import math

import torch
import torch.nn as nn

from ... import _lib as L
from ...engine import runtime as R
from .block import DFL, Proto
from .conv import Conv, DWConv, PackedConv, _HipConvMixin, fold_bn, hip_conv2d, version_key

__all__ = ("Detect", "Segment", "Pose", "Classify")


def _magic_exact(xmax: int, d: int) -> bool:
    """csrc/detect_epi.h upa_magic_exact: umulhi(x, floor(2^32 / d) + 1) == x // d for every 0 <= x <= xmax."""
    if xmax < 0 or d <= 0 or xmax > 0xFFFFFFFF:
        return False
    e = ((1 << 32) // d + 1) * d - (1 << 32)
    return xmax * e < (1 << 32)


class Detect(nn.Module, _HipConvMixin):
    """YOLO Detect head (head.py:28-191), legacy v3/v5/v8 class branch (:98-100).

    eval forward returns `(y, x)` like the reference: y = (B, 4+nc, A) float32 decoded boxes (xywh, pixels) and class
    probabilities, x = the per-level raw maps (NHWC views, logical (B, 4*reg_max+nc, H, W)).
    Per level the box and class branches write the two channel slices of one (B,H,W,144) buffer (the reference's
    `torch.cat((cv2(x), cv3(x)), 1)`, head.py:122) and one `upa_detect_decode` launch performs
    DFL + dist2bbox + stride scaling + sigmoid (head.py:151-169).
    """

    dynamic = False
    export = False
    format = None
    end2end = False
    max_det = 300
    shape = None
    anchors = torch.empty(0)
    strides = torch.empty(0)
    legacy = False
    xyxy = False

    def __init__(self, nc: int = 80, ch: tuple = ()):
        super().__init__()
        self.nc = nc
        self.nl = len(ch)
        self.reg_max = 16
        self.no = nc + self.reg_max * 4
        self.stride = torch.zeros(self.nl)
        c2, c3 = max((16, ch[0] // 4, self.reg_max * 4)), max(ch[0], min(self.nc, 100))
        self.cv2 = nn.ModuleList(
            nn.Sequential(Conv(x, c2, 3), Conv(c2, c2, 3), nn.Conv2d(c2, 4 * self.reg_max, 1)) for x in ch)
        # legacy v3/v5/v8 class branch: Conv3x3 -> Conv3x3 -> 1x1; v11+ (legacy = False, head.py:101-110): DW3x3 -> 1x1 -> DW3x3 -> 1x1 -> 1x1.
        # Recorded per instance (parse_model sets the CLASS attribute for the model being built).  The fused class-branch forms below
        # (branch tail, level stream, grouped levels) assume the legacy branch: the DWConv branch runs its convs and `upa_detect_tail`.
        self.legacy_cls = bool(self.legacy)
        if self.legacy_cls:
            self.cv3 = nn.ModuleList(nn.Sequential(Conv(x, c3, 3), Conv(c3, c3, 3), nn.Conv2d(c3, self.nc, 1)) for x in ch)
        else:
            self.cv3 = nn.ModuleList(
                nn.Sequential(nn.Sequential(DWConv(x, x, 3), Conv(x, c3, 1)), nn.Sequential(DWConv(c3, c3, 3), Conv(c3, c3, 1)),
                              nn.Conv2d(c3, self.nc, 1))
                for x in ch)
        self.dfl = DFL(self.reg_max) if self.reg_max > 1 else nn.Identity()

    # ---- decode fused into the last 1x1 conv of each branch (bf16 perf mode) ----------------------------------------------
    # `upa_detect_tail`: the branch's final nn.Conv2d and its half of Detect._inference (DFL + dist2bbox + stride, or the
    # class sigmoid; head.py:151-169) are ONE kernel - the (B, H, W, 4*reg_max + nc) logits stay in MFMA accumulators.
    # `keep_raw` decides whether they are ALSO written out as the second return value (the reference's `(y, x)`,
    # head.py:126; the predict / validate hot path only reads y).  f32 parity mode keeps conv + upa_detect_decode.
    fuse_decode = True
    keep_raw = True

    def _plan(self):
        return self.__dict__.setdefault("_plans", {})

    def begin(self, n: int, level_hw, dtype, device) -> None:
        """Allocate the decoded output for a forward whose Detect inputs will have the spatial sizes `level_hw` (known
        statically from the input size) so that every level's branches can decode straight into their anchor range."""
        a0, tot = [], 0
        for (h, w) in level_hw:
            a0.append(tot)
            tot += int(h) * int(w)
        fused = bool(self.fuse_decode and dtype == torch.bfloat16 and self.reg_max == 16 and self.nc <= 128
                     and all(h * w >= 2 and w >= 2 for h, w in level_hw)
                     # the fused tails split a flat pixel index into (image, anchor) with a multiply-high: only exact up to a
                     # bound (1280x1280 bs 8 is past it) - larger shapes take conv + upa_detect_decode
                     and all(_magic_exact(n * h * w - 1, h * w) and _magic_exact(h * w - 1, w) for h, w in level_hw))
        y = R.alloc_plain((n, 4 + self.nc, tot), torch.float32, device, key=(id(self), "y"))
        plan = dict(y=y, a0=a0, a_total=tot, fused=fused, hw=[(int(h), int(w)) for h, w in level_hw], n=int(n), decoded=set(),
                    hot=None, hot_levels=set())
        if fused and self.nms_keys:
            # NMS prefilter: the class launches also write every anchor's best-class NMS key (upa_detect_branch_tail, or
            # upa_detect_tail for class branches outside that form / with raw maps kept)
            plan["hot"] = R.alloc_plain((n, tot), torch.int64, device, key=(id(self), "best_keys"))  # u64 bit patterns
        self._plan()[R.current_tag()] = plan

    # `upa_detect_branch_tail`: with no raw output wanted, the branch's SECOND 3x3 conv joins that launch too (its SiLU'd
    # accumulators are the MFMA operand of the 1x1 conv), so a branch is two launches: conv3x3, [conv3x3 + 1x1 + decode].
    fuse_branch = True
    # NMS prefilter (off by default): the fused class tails also write the NMS sort key of every anchor's best class, a dense
    # (B, A) array that `utils.nms` compacts instead of re-reading the (B, nc, A) scores (upa_nms_batched_hot; single-label NMS)
    nms_keys = False
    # `scores_out = False` (only with `nms_keys` and without `keep_raw`): the class rows of the decoded output are NOT written
    # (`upa_opts.keys_only`) - single-label `non_max_suppression` takes every anchor's best class and score from the keys and the
    # boxes from rows 0-3, so for predict the (B, nc, A) scores (86 MB per batch-32 step of yolov8n) and all but one sigmoid per
    # anchor are dead work.  The detections are bit-identical; rows 4.. of the returned tensor are then UNDEFINED (a consumer
    # that reads them - multi_label NMS, validation - must leave this at True).
    scores_out = True

    def _keys_only(self) -> bool:
        return bool(self.nms_keys and not self.scores_out and not self.keep_raw)

    def _tail(self, seq: nn.Sequential, x: torch.Tensor, raw: torch.Tensor | None, kind: int, i: int, plan) -> None:
        """conv3x3 -> conv3x3 -> [1x1 + decode] of one branch (kind 1 = box, 2 = class) of level i."""
        t = seq[0](x)
        if raw is None and self.fuse_branch and self._branch_tail(t, seq[1], seq[2], kind, i, plan):
            return
        self._tail_call(seq[1](t), seq[2], raw, kind, i, plan)

    def _branch_tail_args(self, t: torch.Tensor, mid, conv: nn.Conv2d, kind: int):
        """(view of t, packed 3x3, packed 1x1 tail, its bias) for `upa_detect_branch_tail`, or None outside the fused form."""
        if kind == 2 and not self.legacy_cls:
            return None
        c = mid.conv.in_channels
        cp = 64 if kind == 1 else (80 if c == 80 else 96)  # padded channel count of the fused form (upa_detect_branch_tail)
        if not (isinstance(mid, Conv) and isinstance(mid.act, nn.SiLU) and mid.conv.kernel_size == (3, 3) and mid.conv.stride == (1, 1)
                and mid.conv.padding == (1, 1) and mid.conv.groups == 1 and mid.conv.out_channels == c == conv.in_channels
                and t.dtype == torch.bfloat16 and conv.kernel_size == (1, 1)
                and (c == 64 if kind == 1 else (c <= 96 and c % 8 == 0 and self.nc <= 96))):
            return None
        pk3 = self._packed(mid.conv, mid.bn, t.device, t.dtype, False, pad_cout=cp)
        cache = self.__dict__.setdefault("_pk_cache", {})
        key = (id(conv), str(t.device), "tail", cp)
        ver = version_key(conv.weight, conv.bias)
        hit = cache.get(key)
        if hit is None or hit[0] != ver:
            w = torch.zeros(cp, cp)
            b = torch.zeros(cp)
            w[:conv.out_channels, :c] = conv.weight.detach().float().reshape(conv.out_channels, c).cpu()
            if conv.bias is not None:
                b[:conv.out_channels] = conv.bias.detach().float().cpu()
            host = torch.empty(L.lib().upa_tail_packed_weight_bytes(cp, cp), dtype=torch.uint8)
            L.check(L.lib().upa_pack_tail_weight(w.data_ptr(), cp, cp, host.data_ptr()), "pack_tail_weight")
            hit = (ver, (host.to(t.device), b.to(t.device)))
            cache[key] = hit
        wt, bt = hit[1]
        return R.view_of(t), pk3, wt, bt

    def _branch_tail(self, t: torch.Tensor, mid, conv: nn.Conv2d, kind: int, i: int, plan) -> bool:
        """[conv3x3 + SiLU + 1x1 + decode] in one launch; False when the branch is outside the fused form."""
        args = self._branch_tail_args(t, mid, conv, kind)
        if args is None:
            return False
        vt, pk3, wt, bt = args
        hot = plan.get("hot") if kind == 2 else None
        rc = L.lib().upa_detect_branch_tail(vt.ptr, vt.n, vt.h, vt.w, vt.c, vt.ld, pk3.w.data_ptr(), pk3.bias.data_ptr(),
                                            wt.data_ptr(), bt.data_ptr(), kind, self.nc, float(self.stride[i]),
                                            plan["y"].data_ptr(), plan["a_total"], plan["a0"][i],
                                            hot.data_ptr() if hot is not None else None, vt.dtype, R.opts_ptr(),
                                            L.current_stream(t.device))
        if rc == L.UPA_EUNSUPPORTED:
            return False
        L.check(rc, "detect_branch_tail")
        if hot is not None:
            plan["hot_levels"].add(i)
        return True

    # ---- one level, both branches, all six convolutions + the decode in ONE line-buffer launch (csrc/detect_stream.hip) ----------------
    # yolov8n's 80 x 80 level (64 input channels; 64-channel box branch, 80-channel class branch): the stacked first conv + the grouped
    # branch tails write and re-read a 144-channel intermediate and reload every weight slab per tile; the streaming form keeps t1 / t2 as
    # a few rows in LDS and the weights in registers.  Slower launch for launch (0.878 vs 0.799 ms one step at a time: two waves per SIMD, every
    # role bound by its own in-order issue, profiles/r06_detect_stream.txt) but 192 workgroups that hold a quarter less CU time: +2.4 % with four
    # steps in flight.  So it runs on request: `upa_opts.detect_stream = 2`, which `engine/pipeline.py` sets for copies in flight.
    level_stream = True

    def _level_stream(self, i: int, x: torch.Tensor, plan) -> bool:
        """Level i through `upa_detect_level_stream`; False (nothing launched) outside its form."""
        o_ = R.current_opts()
        if not self.level_stream or o_ is None or o_.detect_stream != 2 or x.dtype != torch.bfloat16 or self.reg_max != 16 \
                or not self.legacy_cls:
            return False
        b, c = self.cv2[i], self.cv3[i]
        ok3 = lambda m, ci, co: (isinstance(m, Conv) and not m.training and isinstance(m.act, nn.SiLU) and hasattr(m, "bn")  # noqa: E731
                                 and m.conv.kernel_size == (3, 3) and m.conv.stride == (1, 1) and m.conv.padding == (1, 1)
                                 and m.conv.groups == 1 and m.conv.in_channels == ci and m.conv.out_channels == co)
        ok1 = lambda m, ci, co: (isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) and m.stride == (1, 1) and m.padding == (0, 0)  # noqa: E731
                                 and m.groups == 1 and m.in_channels == ci and m.out_channels == co)
        cin = int(x.shape[1])
        if not (cin == 64 and self.nc <= 80 and ok3(b[0], 64, 64) and ok3(b[1], 64, 64) and ok1(b[2], 64, 64)
                and ok3(c[0], 64, 80) and ok3(c[1], 80, 80) and ok1(c[2], 80, self.nc)):
            return False
        dev, dt = x.device, x.dtype
        br = []
        for seq, cw, ct in ((b, 64, 64), (c, 80, 80)):
            pk1 = seq[0]._packed(seq[0].conv, seq[0].bn, dev, dt, False)
            pk2 = seq[1]._packed(seq[1].conv, seq[1].bn, dev, dt, False)
            pkt = self._packed(seq[2], None, dev, dt, False, pad_cout=ct)
            br.append(L.DetectBranch(cw, 0, pk1.w.data_ptr(), pk1.bias.data_ptr(), pk2.w.data_ptr(), pk2.bias.data_ptr(), pkt.w.data_ptr(),
                                     pkt.bias.data_ptr()))
        import ctypes as C
        vx = R.view_of(x)
        hot = plan.get("hot")
        rc = L.lib().upa_detect_level_stream(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, C.byref(br[0]), C.byref(br[1]), self.nc,
                                             float(self.stride[i]), plan["y"].data_ptr(), plan["a_total"], plan["a0"][i],
                                             hot.data_ptr() if hot is not None else None, L.dtype_code(dt), R.opts_ptr(),
                                             L.current_stream(dev))
        if rc == L.UPA_EUNSUPPORTED:
            return False
        L.check(rc, "detect_level_stream")
        if hot is not None:
            plan["hot_levels"].add(i)
        return True

    # ---- several levels per launch (linear graphs: the levels run one after the other on one stream anyway) ---------------------
    # The 40 x 40 and 20 x 20 levels' launches are 400 and 100 workgroups at batch 32 - a fraction of a round each, mostly launch
    # ramp and halo latency.  `upa_conv2d_bias_act_group` / `upa_detect_branch_tail_group` put problems that use the same kernel
    # instantiation into ONE grid, so the smaller level rides inside the larger one's partial round: 4 launches fewer per step.  (All
    # three levels in one grid - the 80 x 80 level on the 128-pixel variant - measured slower: upa_opts.no_group = 2.)
    group_levels = True
    stack_first = True  # the first level's two first convs as one 144-channel convolution (see _levels_grouped)

    def _levels_grouped(self, idx, xs, plan, allow_stack: bool = True) -> bool:
        """Both branches of the levels `idx` (inputs `xs`, NHWC) through the group entry points; False (nothing launched) when a
        level is outside the fused forms."""
        import ctypes as C
        if not self.legacy_cls:
            return False
        lib = L.lib()
        dev = xs[0].device
        stream = L.current_stream(dev)
        todo = []
        for kind, seqs in ((1, self.cv2), (2, self.cv3)):  # check everything before the first launch
            for i in idx:
                c0 = seqs[i][0]
                if not (isinstance(c0, Conv) and not c0.training and c0.conv.kernel_size == (3, 3) and c0.conv.stride == (1, 1)
                        and c0.conv.padding == (1, 1) and c0.conv.groups == 1 and isinstance(c0.act, nn.SiLU) and hasattr(c0, "bn")):
                    return False
            todo.append((kind, seqs))
        # stage 1: the first convs of all branches in ONE group call.  Order = which neighbours may share a grid: the two branches of
        # the first (largest) level read the same input and use the same workgroup size, then each kind's remaining levels
        # The two first convs of the first (largest) level read the same input: stacked along the output channels they are ONE 64 + 80 =
        # 144-channel convolution (conv_big's nine-tile variant) - the halo of a tile is fetched once instead of once per branch, the box
        # branch multiplies no padded fifth tile, half the workgroups - and each branch's second half reads its channel slice of the
        # 144-channel tensor.  Same products in the same order per output channel as conv_big's two-problem grid: bit-identical to it -
        # NOT to the level-by-level walks under library-default options, whose 64 -> 64 box conv takes conv_ws3 (another f32 summation order:
        # last-bit differences, tests/test_hip_e2e.py::test_e2e_grouped_detect_levels_equal_level_by_level runs under conv_ws3 = 1 for that
        # reason; a default-options tolerance test sits next to it).  Measured (yolov8n bs 32, round 5, same
        # box, upa_opts.no_stack_first = 1 | 0): the stacked launch takes what the two-problem grid took (65.9 vs 66.1 us with four steps
        # in flight, 58.46 k images/s either way; the serial step 0.810 -> 0.808 ms): the first convs are bound by their per-tap matrix /
        # LDS work, not by the second halo fetch.  Kept: one launch and one tensor fewer, never slower.
        o_ = R.current_opts()
        i0 = idx[0]
        b0, c0_ = self.cv2[i0][0], self.cv3[i0][0]
        stacked = (allow_stack and self.stack_first and (o_ is None or not o_.no_stack_first) and xs[0].dtype == torch.bfloat16
                   and b0.conv.out_channels == 64 and c0_.conv.out_channels == 80 and b0.conv.in_channels == c0_.conv.in_channels
                   and b0.conv.in_channels >= 64)
        order = ([("stack", None, i0)] if stacked else [(kind, seqs, i0) for kind, seqs in todo]) + \
                [(kind, seqs, i) for kind, seqs in todo for i in idx[1:]]
        probs = (L.ConvProblem * len(order))()
        mid_of = {}
        for j, (kind, seqs, i) in enumerate(order):
            x = xs[idx.index(i)]
            vx = R.view_of(x)
            if kind == "stack":
                pk = self._packed_stack([(b0.conv, b0.bn), (c0_.conv, c0_.bn)], dev, x.dtype)
                t = R.alloc_nhwc(vx.n, pk.cout, vx.h, vx.w, x.dtype, dev, key=(id(b0), "y144"))
                mid_of[(1, i)], mid_of[(2, i)] = t[:, :64], t[:, 64:]
            else:
                c0 = seqs[i][0]
                pk = c0._packed(c0.conv, c0.bn, dev, x.dtype, False)
                t = R.alloc_nhwc(vx.n, pk.cout, vx.h, vx.w, x.dtype, dev, key=(id(c0), "y"))
                mid_of[(kind, i)] = t
            vy = R.view_of(t)
            probs[j] = L.ConvProblem(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, pk.w.data_ptr(), pk.bias.data_ptr(), vy.ptr, pk.cout, vy.ld, None, 0)
        L.check(lib.upa_conv2d_bias_act_group(C.cast(probs, C.c_void_p), len(order), 3, 1, 1, L.ACT_SILU, L.dtype_code(xs[0].dtype),
                                              R.opts_ptr(), stream), "conv2d_group")
        # stage 2: the branch tails of both kinds in one call (box and class problems share grids where their workgroup sizes agree)
        args = {kind: [self._branch_tail_args(mid_of[(kind, i)], seqs[i][1], seqs[i][2], kind) for i in idx] for kind, seqs in todo}
        hot = plan.get("hot")
        rc = L.UPA_EUNSUPPORTED
        if all(a is not None for k in args for a in args[k]):
            lvs = {}
            for kind in (1, 2):
                lv = (L.BranchLevel * len(idx))()
                for j, (i, (vt, pk3, wt, bt)) in enumerate(zip(idx, args[kind])):
                    lv[j] = L.BranchLevel(vt.ptr, vt.n, vt.h, vt.w, vt.c, vt.ld, pk3.w.data_ptr(), pk3.bias.data_ptr(), wt.data_ptr(),
                                          bt.data_ptr(), float(self.stride[i]), plan["a0"][i])
                lvs[kind] = lv
            rc = lib.upa_detect_head_tails(C.cast(lvs[1], C.c_void_p), C.cast(lvs[2], C.c_void_p), len(idx), self.nc, plan["y"].data_ptr(),
                                           plan["a_total"], hot.data_ptr() if hot is not None else None, L.dtype_code(xs[0].dtype),
                                           R.opts_ptr(), stream)
        if rc == L.UPA_EUNSUPPORTED:  # a branch outside the branch-tail form: the second halves level by level
            for kind, seqs in todo:
                for i in idx:
                    t = mid_of[(kind, i)]
                    if not self._branch_tail(t, seqs[i][1], seqs[i][2], kind, i, plan):
                        self._tail_call(seqs[i][1](t), seqs[i][2], None, kind, i, plan)
        else:
            L.check(rc, "detect_head_tails")
            if hot is not None:
                plan["hot_levels"].update(idx)
        return True

    def _tail_call(self, t: torch.Tensor, conv: nn.Conv2d, raw, kind: int, i: int, plan) -> None:
        """The fused launch itself: t = the branch's second 3x3 output, conv = its final nn.Conv2d."""
        cout = 4 * self.reg_max if kind == 1 else self._ncp(t.dtype)
        pk = self._packed(conv, None, t.device, t.dtype, False, pad_cout=cout)
        vt = R.view_of(t)
        rp, rld = (None, 0)
        if raw is not None:
            vr = R.view_of(raw)
            rp, rld = vr.ptr, vr.ld
        hot = plan.get("hot") if kind == 2 else None
        L.check(L.lib().upa_detect_tail(vt.ptr, vt.n, vt.h, vt.w, vt.c, vt.ld, pk.w.data_ptr(), pk.bias.data_ptr(), cout, kind,
                                        self.nc, float(self.stride[i]), plan["y"].data_ptr(), plan["a_total"], plan["a0"][i],
                                        rp, rld, hot.data_ptr() if hot is not None else None, vt.dtype, R.opts_ptr(),
                                        L.current_stream(t.device)), "detect_tail")
        if hot is not None:
            plan["hot_levels"].add(i)

    def _branch(self, seq: nn.Sequential, x: torch.Tensor, out: torch.Tensor) -> None:
        t = seq[1](seq[0](x))
        # `out` may be wider than the conv (class rows are padded to the 16-byte store width when nc is not a multiple
        # of it): the extra filters are zero and the extra channels are never read
        pk = self._packed(seq[2], None, x.device, x.dtype, False, pad_cout=int(out.shape[1]))
        hip_conv2d(t, pk, 1, 0, L.ACT_NONE, out=out)

    def _ncp(self, dtype) -> int:
        """Class channels as stored: nc rounded up to 16 bytes of `dtype` (any nc is accepted, as in the reference)."""
        e = 16 // (2 if dtype == torch.bfloat16 else 4)
        return (self.nc + e - 1) // e * e

    # ---- branch-level concurrency -------------------------------------------------------------------------------------
    # The box and class branches of a level are independent 3-conv chains and a level only depends on its own input
    # (head.py:116-126), so the executor may start a level the moment its feature map exists (`start_level`, called by
    # BaseModel._predict_once) on two side HIP streams forked from the producing stream; `forward` joins them before
    # the decode.  Under hipGraph capture the event fork/join becomes parallel graph branches.  The small 20x20/40x40
    # launches of the neck and the head are latency-bound (a few hundred workgroups on 256 CUs), so they overlap well.
    concurrent = True

    def _side_streams(self, device):
        pools = self.__dict__.setdefault("_streams", {})
        key = (R.current_tag(), str(device))
        st = pools.get(key)
        if st is None:
            st = [torch.cuda.Stream(device=device) for _ in range(2 * self.nl)]
            pools[key] = st
        return st

    def _pend(self):
        return self.__dict__.setdefault("_pending", {}).setdefault(R.current_tag(), {})

    def start_level(self, i: int, x: torch.Tensor, defer_ok: bool = True) -> None:
        if self._keys_only() and (R.current_opts() is None or not R.current_opts().keys_only):
            with R.use_opts(keys_only=1):
                return self._start_level(i, x, defer_ok)
        return self._start_level(i, x, defer_ok)

    def _start_level(self, i: int, x: torch.Tensor, defer_ok: bool = True) -> None:
        """Launch level i's two branches (asynchronously when `concurrent`); results land in the level's raw buffer and /
        or, with the fused decode, directly in the decoded output.  On one stream (linear graphs) the levels are left to `forward`,
        which runs them several per launch (`_levels_grouped`)."""
        pend = self._pend()
        x = R.to_nhwc(x, x.dtype)
        nb = 4 * self.reg_max
        n, _, h, w = x.shape
        plan = self._plan().get(R.current_tag())
        if plan is not None and (plan["n"] != n or plan["hw"][i] != (h, w) or plan["y"].device != x.device):
            plan = None  # stale plan (other input size): this level goes through the separate decode
        fused = plan is not None and plan["fused"] and x.dtype == torch.bfloat16
        ncp = self._ncp(x.dtype)
        buf = None
        if not fused or self.keep_raw:
            buf = R.alloc_nhwc(n, nb + ncp, h, w, x.dtype, x.device, key=(id(self), "raw", i))
        outs = (None, None) if buf is None else (buf[:, :nb], buf[:, nb:])
        raw = None if buf is None else buf[:, :self.no]

        def run(k):
            seq = (self.cv2[i], self.cv3[i])[k]
            if fused:
                self._tail(seq, x, outs[k], k + 1, i, plan)
            else:
                self._branch(seq, x, outs[k])

        linear = not self.concurrent or R.current_tag() != 0
        if defer_ok and linear and fused and self.group_levels and self.fuse_branch and not self.keep_raw:
            return  # `forward` picks it up (grouped with the other small levels)
        if fused and buf is None and self.fuse_branch and self._level_stream(i, x, plan):
            # the same line-buffer launch on every walk (grouped, level by level, concurrent): the output does not depend on the walk
            plan["decoded"].add(i)
            pend[i] = (None, [])
            return
        if fused:
            plan["decoded"].add(i)
        if linear:
            # inside a concurrently scheduled sub-batch (BaseModel.compile(micro_batches>1)) the branches stay on the
            # sub-batch's stream: the sub-batches already overlap each other, and nesting a second level of event
            # forks inside a forked capture stream crashed hipStreamEndCapture on ROCm 7.2 (segfault, not an error code)
            run(0)
            run(1)
            pend[i] = (raw, [])
            return
        main = torch.cuda.current_stream(x.device)
        fork = torch.cuda.Event()
        fork.record(main)
        joins = []
        streams = self._side_streams(x.device)
        for k in range(2):
            side = streams[2 * i + k]
            side.wait_event(fork)
            with torch.cuda.stream(side):
                run(k)
                ev = torch.cuda.Event()
                ev.record(side)
            joins.append(ev)
        pend[i] = (raw, joins)

    def forward(self, x):
        if self._keys_only() and (R.current_opts() is None or not R.current_opts().keys_only):
            with R.use_opts(keys_only=1):
                return self._forward(x)
        return self._forward(x)

    def _forward(self, x):
        if self.training:
            raise L.UpaError("training-mode Detect is not on the HIP path yet (SURVEY §8f rank 2)")
        pend = self._pend()
        if not pend:  # called directly (not through BaseModel._predict_once): the level shapes come with the inputs
            self.begin(x[0].shape[0], [(t.shape[2], t.shape[3]) for t in x], x[0].dtype, x[0].device)
        rest = [i for i in range(self.nl) if i not in pend]
        plan = self._plan().get(R.current_tag())
        linear = not self.concurrent or R.current_tag() != 0
        grp = list(rest)
        if (len(grp) >= 2 and linear and self.group_levels and self.fuse_branch and not self.keep_raw and plan is not None and plan["fused"]
                and all(x[i].dtype == torch.bfloat16 and plan["n"] == x[i].shape[0] and plan["hw"][i] == tuple(x[i].shape[2:])
                        and plan["y"].device == x[i].device for i in grp)):
            xs_n = [R.to_nhwc(x[i], x[i].dtype) for i in grp]
            streamed = self._level_stream(grp[0], xs_n[0], plan)  # the first (largest) level as ONE line-buffer launch where it applies
            if streamed:
                plan["decoded"].add(grp[0])
                pend[grp[0]] = (None, [])
                grp, xs_n = grp[1:], xs_n[1:]
            if len(grp) >= 2 and self._levels_grouped(grp, xs_n, plan, allow_stack=not streamed):
                for i in grp:
                    plan["decoded"].add(i)
                    pend[i] = (None, [])
        for i in range(self.nl):
            if i not in pend:
                self.start_level(i, x[i], defer_ok=False)
        main = torch.cuda.current_stream(x[0].device)
        raw = []
        for i in range(self.nl):
            buf, joins = pend[i]
            for ev in joins:
                main.wait_event(ev)
            raw.append(buf)
        pend.clear()
        y = self._inference(raw)
        return y if self.export else (y, raw)

    def _inference(self, x: list) -> torch.Tensor:
        """Decode boxes and class probabilities of all levels into (B, 4+nc, A) float32 (head.py:151-169).  Levels whose
        branches already decoded in their last conv (`upa_detect_tail`) are skipped; x[i] may then be None."""
        nb = 4 * self.reg_max
        plan = self._plan().pop(R.current_tag(), None)
        done = plan["decoded"] if plan is not None else set()
        if plan is not None and (done or all(t is not None for t in x)):
            y, a_total = plan["y"], plan["a_total"]
        else:
            n = x[0].shape[0]
            a_total = sum(int(t.shape[2]) * int(t.shape[3]) for t in x)
            y = R.alloc_plain((n, 4 + self.nc, a_total), torch.float32, x[0].device, key=(id(self), "y"))
        a0 = 0
        for i, t in enumerate(x):
            if i in done:
                a0 += plan["hw"][i][0] * plan["hw"][i][1]
                continue
            vb, vc = R.view_of(t[:, :nb]), R.view_of(t[:, nb:])
            L.check(L.lib().upa_detect_decode(vb.ptr, vb.ld, vc.ptr, vc.ld, vb.n, vb.h, vb.w, self.reg_max, self.nc,
                                              float(self.stride[i]), y.data_ptr(), a_total, a0, vb.dtype,
                                              L.current_stream(t.device)), "detect_decode")
            a0 += vb.h * vb.w
        # NMS prefilter: valid only when every level's class branch wrote its keys in THIS forward
        hot = plan.get("hot") if plan is not None else None
        if hot is not None and plan["hot_levels"] == set(range(self.nl)) and y is plan["y"]:
            y._upa_hot = hot
        elif hasattr(y, "_upa_hot"):
            del y._upa_hot
        # keys-only mode (`scores_out = False`): rows 4.. of y were NOT written in this forward - mark the tensor so that every reader of
        # class scores (multi-label NMS, the validator) refuses it instead of reading stale memory
        if self._keys_only() and hasattr(y, "_upa_hot"):
            y._upa_keys_only = True
        elif hasattr(y, "_upa_keys_only"):
            del y._upa_keys_only
        return y

    def bias_init(self):
        """Initialize Detect() biases, requires stride availability (head.py:171-178)."""
        for a, b, s in zip(self.cv2, self.cv3, self.stride):
            a[-1].bias.data[:] = 1.0
            b[-1].bias.data[: self.nc] = math.log(5 / self.nc / (640 / s) ** 2)

    def train(self, mode: bool = True):
        self.invalidate_packed()
        return super().train(mode)


class ExtraDetect(Detect):
    """Detect plus one more per-level branch `cv4[l]` whose per-anchor output is laid into an `extra` (B, ne, A) f32 tensor: the
    shared part of `Segment` (mask coefficients) and `Pose` (keypoints).

    Eval forward returns the reference's `(cat([y, extra], 1), rest)`: y = Detect's (B, 4+nc, A) output, untouched (every fused Detect
    form and NMS kernel keeps its image stride), each level's cv4 output written into its anchor range of `extra`.  With
    `cat_out = False` the concatenated copy is not made and the first element is y itself.  Either way the first element carries
    `_upa_parts = (y, extra)`: `utils.nms` runs on y and gathers the extra columns of the kept rows, and the postprocess of
    `utils.ops` reads the parts.

    Scheduling: a level's cv4 branch runs when `start_level` is called for it (the moment its feature map exists); levels the executor
    did not start (a direct call, or the levels `Detect.forward` groups) run in `forward`.  Inference only: a train-mode forward raises
    (`_train_refusal`), the train-mode head is the trainer's tail op.

    A subclass states the width and the buffers (`_extra_alloc`), one level's work (`_extra_level`), what follows the first output
    (`_result`) and `_train_refusal`."""

    cat_out = True

    def _extra_plans(self):
        return self.__dict__.setdefault("_extra", {})

    def begin(self, n: int, level_hw, dtype, device) -> None:
        super().begin(n, level_hw, dtype, device)
        det = self._plan()[R.current_tag()]
        self._extra_begin(det["n"], det["hw"], det["a0"], det["a_total"], device)

    def _extra_begin(self, n: int, hw, a0, a_total: int, device):
        """The forward's plan of the cv4 branches: Detect's anchor ranges, the buffers of `_extra_alloc`, the levels done so far."""
        plan = dict(n=n, hw=hw, a0=a0, a_total=a_total, done=set(), **self._extra_alloc(n, a_total, device))
        self._extra_plans()[R.current_tag()] = plan
        return plan

    @staticmethod
    def _extra_fits(plan, i, x) -> bool:
        return plan["n"] == int(x.shape[0]) and plan["hw"][i] == (int(x.shape[2]), int(x.shape[3])) and plan["extra"].device == x.device

    def start_level(self, i: int, x: torch.Tensor, defer_ok: bool = True) -> None:
        super().start_level(i, x, defer_ok)
        plan = self._extra_plans().get(R.current_tag())
        if plan is not None and i not in plan["done"] and self._extra_fits(plan, i, x):
            self._extra_level(plan, i, x)
            plan["done"].add(i)

    def forward(self, x):
        if self.training:
            raise L.UpaError(self._train_refusal)
        det = super().forward(x)
        y, raw = (det, None) if self.export else det
        tag = R.current_tag()
        plan = self._extra_plans().get(tag)
        if plan is None or not all(self._extra_fits(plan, i, x[i]) for i in range(self.nl)):
            # a plan for other sizes, with Detect's own already consumed: the anchor ranges of the sizes that came
            hw = [(int(t.shape[2]), int(t.shape[3])) for t in x]
            ends = list(itertools.accumulate(h * w for h, w in hw))
            plan = self._extra_begin(int(x[0].shape[0]), hw, [0] + ends[:-1], ends[-1], x[0].device)
        for i in range(self.nl):
            if i not in plan["done"]:
                self._extra_level(plan, i, x[i])
        self._extra_plans().pop(tag, None)
        extra = plan["extra"]
        if self.cat_out or self.export:
            out = self._cat(y, extra)
        else:
            out = y
            y._upa_parts = (y, extra)
        return self._result(out, raw, plan)

    def _cat(self, y: torch.Tensor, extra: torch.Tensor) -> torch.Tensor:
        """(B, 4+nc+ne, A) = cat([y, extra], 1) with two strided copies: `upa_copy_view` over one 'pixel' per image when every row is
        a 16-byte multiple, else `upa_copy_rows` (any A)."""
        n, cy, a = y.shape
        ne = int(extra.shape[1])
        ct = cy + ne
        cat = R.alloc_plain((n, ct, a), torch.float32, y.device, key=(id(self), "cat"))
        stream = L.current_stream(y.device)
        lib = L.lib()
        for src, c, dst in ((y, cy, cat), (extra, ne, cat[:, cy:])):
            if (cy * a) % 4 == 0 and (ne * a) % 4 == 0:
                L.check(lib.upa_copy_view(src.data_ptr(), n, 1, 1, c * a, c * a, dst.data_ptr(), ct * a, L.UPA_F32, stream), "copy_view")
            else:
                L.check(lib.upa_copy_rows(src.data_ptr(), n, c * a, c * a, dst.data_ptr(), ct * a, stream), "copy_rows")
        cat._upa_parts = (y, extra)
        return cat

    def train(self, mode: bool = True):
        self.__dict__.pop("_extra", None)
        return super().train(mode)


class Segment(ExtraDetect):
    """YOLO Segment head (head.py:790-837): Detect + `proto = Proto(ch[0], npr, nm)` + per-level mask-coefficient branches
    `cv4[l] = Conv3x3 -> Conv3x3 -> nn.Conv2d(c4, nm, 1)`, c4 = max(ch[0] // 4, nm).

    Eval forward returns `(cat([y, mc], 1), (raw, mc, p))`: mc = (B, nm, A) f32 coefficients (`upa_mask_coef_rows` writes each level's
    map into its anchor range), p = the (B, nm, 2H0, 2W0) protos as an NHWC view; Proto runs with level 0.
    `utils.ops.segment_postprocess_raw` reads y, mc and p."""

    _train_refusal = ("training-mode Segment.forward is not on the HIP path: train a segmentation model with engine.trainer.SegmentationTrainer (its "
                      "SegmentT op holds the train-mode head)")

    def __init__(self, nc: int = 80, nm: int = 32, npr: int = 256, ch: tuple = ()):
        super().__init__(nc, ch)
        self.nm = nm
        self.npr = npr
        self.proto = Proto(ch[0], self.npr, self.nm)
        c4 = max(ch[0] // 4, self.nm)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, self.nm, 1)) for x in ch)

    def _extra_alloc(self, n, a_total, device):
        return dict(extra=R.alloc_plain((n, self.nm, a_total), torch.float32, device, key=(id(self), "mc")), p=None)

    def _extra_level(self, plan, i: int, x: torch.Tensor) -> None:
        """cv4[i] into mc[:, :, a0_i : a0_i + H_i W_i] (and Proto, for level 0)."""
        x = R.to_nhwc(x, x.dtype)
        seq = self.cv4[i]
        t = seq[1](seq[0](x))
        pk = self._packed(seq[2], None, x.device, x.dtype, False)
        c = hip_conv2d(t, pk, 1, 0, L.ACT_NONE, key=(id(self), "mc_map", i))
        vc = R.view_of(c)
        L.check(L.lib().upa_mask_coef_rows(vc.ptr, vc.n, vc.h, vc.w, vc.c, vc.ld, vc.dtype, plan["extra"].data_ptr(), self.nm, 0,
                                           plan["a_total"], plan["a0"][i], L.current_stream(x.device)), "mask_coef_rows")
        if i == 0:
            plan["p"] = self.proto(x)

    def _result(self, out, raw, plan):
        return (out, plan["p"]) if self.export else (out, (raw, plan["extra"], plan["p"]))


class Pose(ExtraDetect):
    """YOLO Pose head (head.py:1208-1273): Detect + per-level keypoint branches `cv4[l] = Conv3x3 -> Conv3x3 -> nn.Conv2d(c4, nk, 1)`,
    nk = kpt_shape[0] * kpt_shape[1], c4 = max(ch[0] // 4, nk).

    Eval forward returns `(cat([y, pred_kpt], 1), (raw, kpt))`: pred_kpt = (B, nk, A) f32 decoded keypoints and kpt the undecoded
    ones (None with `keep_raw = False`): one `upa_kpt_decode_rows` launch per level writes both into the level's anchor range.
    `utils.ops.pose_postprocess_raw` reads y and pred_kpt.

    51 channels: nk = 17 * 3 (and c4, for the n / s / m scales) is no multiple of the convolutions' 16-byte channel rule.  The
    state_dict keeps the reference's shapes; the PACKED weights are padded to multiples of 8 channels (`_packed_pad`): padded output
    channels have zero filters and zero folded bias (SiLU(0) = 0, so they stay zero), the next conv's padded input channels have zero
    filters (their products add exact zeros: the real channels are bit-identical to an unpadded convolution)."""

    _train_refusal = ("training-mode Pose.forward is not on the HIP path: pose training (v8PoseLoss) goes through "
                      "engine.trainer.PoseTrainer (its PoseT op holds the train-mode head)")
    PAD = 8  # channels per 16 bytes of bf16; a multiple of f32's 4, so one padded layout serves both dtypes

    def __init__(self, nc: int = 80, kpt_shape: tuple = (17, 3), ch: tuple = ()):
        try:
            nkpt, ndim = (int(v) for v in kpt_shape)
        except (TypeError, ValueError):
            raise L.UpaError(f"Pose: kpt_shape must be (keypoints, 2 | 3), got {kpt_shape!r}") from None
        if ndim not in (2, 3):
            raise L.UpaError(f"Pose: kpt_shape[1] = {ndim} - a keypoint is (x, y) or (x, y, visibility)")
        if nkpt < 1:
            raise L.UpaError(f"Pose: kpt_shape[0] = {nkpt} - at least one keypoint is needed")
        if nkpt * ndim > 128:
            raise L.UpaError(f"Pose: {nkpt * ndim} keypoint values per anchor are past upa_kpt_decode_rows' 128")
        super().__init__(nc, ch)
        self.kpt_shape = kpt_shape
        self.nk = nkpt * ndim
        c4 = max(ch[0] // 4, self.nk)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, self.nk, 1)) for x in ch)

    def _packed_pad(self, conv: nn.Conv2d, bn, device, dtype, pad_cin: int, pad_cout: int) -> PackedConv:
        """`_packed` with zero input channels appended up to `pad_cin` and zero filters / biases up to `pad_cout`."""
        cache = self.__dict__.setdefault("_pk_cache", {})
        key = (id(conv), str(device), dtype, "pose", pad_cin, pad_cout)
        ver = version_key(conv.weight, conv.bias, *(() if bn is None else (bn.weight, bn.bias, bn.running_mean,
                                                                           bn.running_var))) + ((bn.eps,) if bn is not None else ())
        hit = cache.get(key)
        if hit is not None and hit[0] == ver:
            return hit[1]
        w, b = fold_bn(conv, bn)
        co, ci, k, _ = w.shape
        wp = torch.zeros(max(pad_cout, co), max(pad_cin, ci), k, k)
        wp[:co, :ci] = w
        bp = torch.zeros(wp.shape[0])
        bp[:co] = b
        pk = PackedConv(wp, bp, k, device, dtype, False)
        cache[key] = (ver, pk)
        return pk

    def kpt_chain(self, i: int, x: torch.Tensor):
        """cv4[i] on the padded layout: (t0, t1, c) = the two 3x3 outputs (c4 rounded up to 8 channels) and the 1x1 output (nk rounded
        up to 8), NHWC views; channels past c4 / nk are zero."""
        x = R.to_nhwc(x, x.dtype)
        seq = self.cv4[i]
        for m in seq[:2]:
            if m.training:
                raise L.UpaError("Pose: a cv4 Conv is in train mode")
        up = lambda v: (v + self.PAD - 1) // self.PAD * self.PAD  # noqa: E731
        c4p, nkp = up(seq[0].conv.out_channels), up(self.nk)
        dev, dt = x.device, x.dtype
        pk0 = self._packed_pad(seq[0].conv, seq[0].bn, dev, dt, 0, c4p)
        pk1 = self._packed_pad(seq[1].conv, seq[1].bn, dev, dt, c4p, c4p)
        pk2 = self._packed_pad(seq[2], None, dev, dt, c4p, nkp)
        t0 = hip_conv2d(x, pk0, seq[0].conv.stride[0], seq[0].conv.padding[0], seq[0]._act_code(), key=(id(self), "kpt_t0", i))
        t1 = hip_conv2d(t0, pk1, seq[1].conv.stride[0], seq[1].conv.padding[0], seq[1]._act_code(), key=(id(self), "kpt_t1", i))
        c = hip_conv2d(t1, pk2, 1, 0, L.ACT_NONE, key=(id(self), "kpt_map", i))
        return t0, t1, c

    def _extra_alloc(self, n, a_total, device):
        shape = (n, self.nk, a_total)
        return dict(extra=R.alloc_plain(shape, torch.float32, device, key=(id(self), "pred_kpt")),
                    kpt=R.alloc_plain(shape, torch.float32, device, key=(id(self), "kpt")) if self.keep_raw else None)

    def _extra_level(self, plan, i: int, x: torch.Tensor) -> None:
        """cv4[i] decoded into pred_kpt[:, :, a0_i : a0_i + H_i W_i] (and the undecoded values into kpt)."""
        _, _, c = self.kpt_chain(i, x)
        vc = R.view_of(c)
        kpt = plan["kpt"]
        nkpt, ndim = (int(v) for v in self.kpt_shape)
        L.check(L.lib().upa_kpt_decode_rows(vc.ptr, vc.n, vc.h, vc.w, vc.c, vc.ld, vc.dtype, nkpt, ndim, float(self.stride[i]),
                                            plan["extra"].data_ptr(), plan["a_total"], plan["a0"][i],
                                            None if kpt is None else kpt.data_ptr(), L.current_stream(x.device)), "kpt_decode_rows")

    def _result(self, out, raw, plan):
        if not (self.cat_out or self.export):
            out._upa_pose = plan["extra"]  # what `_upa_parts[1]` was called on y before every head shared one convention: kept for its readers
        return out if self.export else (out, (raw, plan["kpt"]))


class Classify(nn.Module):
    """YOLO classification head (head.py:1481-1531): Conv(c1, 1280, 1) -> AdaptiveAvgPool2d(1) -> Dropout(0) -> Linear(1280, c2) ->
    softmax(1).  Eval forward returns the reference's `(probs, logits)`, (B, c2) float32 each (`probs` alone with `export`).

    Three launches: `upa_classify_pool` (conv + SiLU + pool: the (B, 1280, H, W) activation is never written; pooled rows are float32 in
    both modes), `upa_linear` (exact float32 on the pooled rows in BOTH modes - 1280 is past `upa_linear_bf16`'s depth and 16-bit
    products would only add error to 82 MFLOP) and `upa_softmax_topk`, which also leaves the indices of the min(c2, 5) largest logits
    of every row in `self.top5` (and on the returned probabilities as `_upa_top5`) for `ClassificationValidator`.  Rows are stored
    with c2 rounded up to 4 columns (16-byte rows for the GEMM's stores); the returned tensors are views of the first c2.

    `pool` and `drop` are the reference's children (no parameters; they keep the module list and state_dict layout) and never run.
    This module's forward is the inference path: train mode, a list input, k != 1, s != 1 and g != 1 raise.  Training lives in the
    trainer's op, as for every other layer: `engine.trainer.ClassificationTrainer` (`ClassifyT`: train-mode Conv, pool, linear, fused
    cross-entropy and their backward).  After its optimizer steps - raw-pointer writes that move no `_version` - `eval()` sees the new
    weights: both packed caches are keyed on `version_key`, which carries the process-wide weights generation the trainer bumps."""

    export = False

    def __init__(self, c1: int, c2: int, k: int = 1, s: int = 1, p: int | None = None, g: int = 1):
        super().__init__()
        if k != 1 or s != 1 or g != 1:
            raise L.UpaError(f"Classify: the HIP head is the 1x1 stride-1 groups-1 form (got k={k}, s={s}, g={g})")
        c_ = 1280  # efficientnet_b0 size
        self.conv = Conv(c1, c_, k, s, p, g)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.drop = nn.Dropout(p=0.0, inplace=True)
        self.linear = nn.Linear(c_, c2)
        self.top5 = None

    def _packed_linear(self, device) -> PackedConv:
        """float32 GEMM weights of `linear`, zero rows appended up to a multiple of 4 outputs; cached, validated by `version_key`
        (storage, `_version` and the weights generation `bump_weights_generation()` moves after the trainer's raw-pointer updates)."""
        cache = self.__dict__.setdefault("_pk_cache", {})
        lin = self.linear
        ver = version_key(lin.weight, lin.bias)
        hit = cache.get(str(device))
        if hit is not None and hit[0] == ver:
            return hit[1]
        nc, c_ = lin.weight.shape
        ncp = (nc + 3) // 4 * 4
        w = torch.zeros(ncp, c_, 1, 1)
        w[:nc, :, 0, 0] = lin.weight.detach().float().cpu()
        b = torch.zeros(ncp)
        if lin.bias is not None:
            b[:nc] = lin.bias.detach().float().cpu()
        pk = PackedConv(w, b, 1, device, torch.float32, False)
        cache[str(device)] = (ver, pk)
        return pk

    def forward(self, x):
        if isinstance(x, list):
            raise L.UpaError("Classify: a list input (channel concat) is not on the HIP path")
        if self.training:
            raise L.UpaError("training-mode Classify.forward is not on the HIP path: train a classification model with "
                             "engine.trainer.ClassificationTrainer (its ClassifyT op holds the train-mode head)")
        L.require_gpu(x, "Classify")
        if x.dtype not in (torch.float32, torch.bfloat16):
            raise L.UpaError(f"Classify: unsupported activation dtype {x.dtype}")
        x = R.to_nhwc(x, x.dtype, key=(id(self), "x"))
        vx = R.view_of(x)
        cv = self.conv
        if cv.training:
            raise L.UpaError("Classify: its Conv is in train mode")
        pk = cv._packed(cv.conv, getattr(cv, "bn", None), x.device, x.dtype, False)
        lib, stream, dev = L.lib(), L.current_stream(x.device), x.device
        n, nc = vx.n, self.linear.out_features
        pooled = R.alloc_plain((n, pk.cout), torch.float32, dev, key=(id(self), "pooled"))
        L.check(lib.upa_classify_pool(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, pk.w.data_ptr(), pk.bias.data_ptr(), pooled.data_ptr(), pk.cout,
                                      pk.cout, cv._act_code(), vx.dtype, R.opts_ptr(), stream), "classify_pool")
        pl = self._packed_linear(dev)
        ncp = pl.cout
        logits = R.alloc_plain((n, ncp), torch.float32, dev, key=(id(self), "logits"))
        L.check(lib.upa_linear(pooled.data_ptr(), n, pk.cout, pk.cout, pl.w.data_ptr(), pl.bias.data_ptr(), logits.data_ptr(), ncp, ncp,
                               None, 0, L.ACT_NONE, stream), "linear")
        probs = R.alloc_plain((n, ncp), torch.float32, dev, key=(id(self), "probs"))
        k5 = min(nc, 5)
        top = R.alloc_plain((n, k5), torch.int32, dev, key=(id(self), "top5"))
        L.check(lib.upa_softmax_topk(logits.data_ptr(), n, nc, ncp, probs.data_ptr(), ncp, k5, top.data_ptr(), stream), "softmax_topk")
        self.top5 = top
        y = probs[:, :nc]
        y._upa_top5 = top
        return y if self.export else (y, logits[:, :nc])

    def train(self, mode: bool = True):
        self.__dict__.pop("_pk_cache", None)
        return super().train(mode)
