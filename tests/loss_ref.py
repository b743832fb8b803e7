"""Float64 CPU restatement of the detection training loss of csrc/loss.hip (DFL decode, TaskAlignedAssigner top-k and resolve,
SlideLoss BCE, CIoU and DFL with the gradient wrt the raw head maps), the decidability report of an input, the input families and
the one case table that tests/test_loss_ref.py (CPU) and tests/test_hip_loss.py (GPU) both walk.

Plain torch on the CPU; nothing here imports the HIP package.  The reference takes what the C ABI takes: head maps per level
(NCHW here, the kernels see the same values as NHWC rows), gt (B, rows, 5) = [cls, x1, y1, x2, y2] in float32 pixels with n_gt (B,),
strides and gains.  Label preprocessing is not part of what is compared: both sides see the same float32 pixel values.

Discrete decisions.  The assignment is a chain of comparisons (in-box test, top-10 by alignment metric, argmax of the overlaps for
multiply-claimed anchors, the SlideLoss jump at 0.4, the min / max selectors of the CIoU gradient).  A correct float32 kernel can
only be compared with a float64 reference on inputs where every such comparison is decided by a margin far above float32
rounding.  `loss_ref(...).report` holds those margins for one input, `undecidable()` lists the ones that are too small.  Equal metrics in
the top-k go to the lower anchor index here as in the kernel; torch.topk leaves that order unspecified, which is why a tie makes
an input undecidable rather than a kernel wrong."""

import functools
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from ultralytics_pro_amd.utils import procedural as P

F64 = torch.float64
REG, TOPK = 16, 10
GAINS = (7.5, 0.5, 1.5)  # box, cls, dfl (cfg/default.yaml)
STRIDES = (8.0, 16.0, 32.0)
HW = ((12, 20), (6, 10), (3, 5))  # the default shape: a 160 x 96 image, A = 315 > 256 threads

# decidability thresholds: conditions on INPUTS, some 100 to 1000 times the float32 rounding of the quantity
REL_GAP, SLIDE_GAP, COORD_GAP = 1e-3, 1e-4, 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# the float64 statement
# ---------------------------------------------------------------------------------------------------------------------
def ciou(b1, b2, eps=1e-7):
    """CIoU of xyxy boxes (utils/metrics.py:77-150); alpha is a constant for the gradient."""
    x11, y11, x12, y12 = b1.unbind(-1)
    x21, y21, x22, y22 = b2.unbind(-1)
    w1, h1, w2, h2 = x12 - x11, y12 - y11 + eps, x22 - x21, y22 - y21 + eps
    inter = (torch.minimum(x12, x22) - torch.maximum(x11, x21)).clamp(min=0) * (torch.minimum(y12, y22) - torch.maximum(y11, y21)).clamp(min=0)
    union = w1 * h1 + w2 * h2 - inter + eps
    iou = inter / union
    cw = torch.maximum(x12, x22) - torch.minimum(x11, x21)
    ch = torch.maximum(y12, y22) - torch.minimum(y11, y21)
    c2 = cw ** 2 + ch ** 2 + eps
    rho2 = ((x21 + x22 - x11 - x12) ** 2 + (y21 + y22 - y11 - y12) ** 2) / 4
    v = (4 / math.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    alpha = (v / (v - iou + (1 + eps))).detach()
    return iou - (rho2 / c2 + v * alpha)


def anchors(hw, strides):
    """Anchor centres in grid units (A, 2) as (x, y), row-major per level, and the stride of every anchor (A,)."""
    pts, st = [], []
    for (h, w), s in zip(hw, strides):
        y, x = torch.meshgrid(torch.arange(h, dtype=F64) + 0.5, torch.arange(w, dtype=F64) + 0.5, indexing="ij")
        pts.append(torch.stack((x.flatten(), y.flatten()), 1))
        st.append(torch.full((h * w,), float(s), dtype=F64))
    return torch.cat(pts), torch.cat(st)


def _gap(hi, lo):
    return float((hi - lo) / hi) if hi > 0 else math.inf


def _assign_image(pbox_px, sig, anc_px, boxes):
    """One image.  pbox_px (A, 4) predicted boxes in pixels, sig (A, nc) class probabilities, anc_px (A, 2), boxes (G, 5) valid gt
    rows.  Returns the assigned row per anchor (-1: background), the target score, the claimant mask (G, A) before the resolve
    step, and the margins of every discrete decision taken."""
    A, G = pbox_px.shape[0], boxes.shape[0]
    agt = torch.full((A,), -1, dtype=torch.long)
    score = torch.zeros(A, dtype=F64)
    m = dict(topk_gap=math.inf, multi_gap=math.inf, dmin=math.inf, zero_fill=0, n_multi=0, n_steal=0, n_empty_box=0, on_centre=[])
    if G == 0:
        return agt, score, torch.zeros(0, A, dtype=torch.bool), m
    cls, bx = boxes[:, 0].long(), boxes[:, 1:5]
    d = torch.cat((anc_px[None] - bx[:, None, :2], bx[:, None, 2:] - anc_px[None]), 2).amin(2)  # (G, A)
    inbox = d > 1e-9
    nz = d.abs()[d != 0]
    if nz.numel():
        m["dmin"] = float(nz.min())
    m["on_centre"] = (d == 0).any(0).nonzero().flatten().tolist()
    m["n_empty_box"] = int((~inbox.any(1)).sum())
    ov = ciou(bx[:, None, :], pbox_px[None]).clamp(min=0) * inbox
    metric = sig[:, cls].T.sqrt() * ov ** 6 * inbox
    # top-k per box: metric descending, equal metrics by ascending anchor
    order = torch.sort(-metric, dim=1, stable=True).indices
    claim = torch.zeros(G, A, dtype=torch.bool)
    claim.scatter_(1, order[:, :TOPK], True)
    claim &= inbox
    srt = torch.gather(metric, 1, order)
    for g in range(G):
        npos = int((metric[g] > 0).sum())
        if npos > TOPK:
            m["topk_gap"] = min(m["topk_gap"], _gap(srt[g, TOPK - 1], srt[g, TOPK]))
        elif npos < TOPK:
            # the top-k is filled up with zero metrics, in an order torch.topk does not specify.  A zero-metric anchor has target score
            # 0 and carries no loss - unless another box overlaps it, where one more or one fewer claim changes who resolves it
            fill = inbox[g] & (metric[g] == 0)
            if fill.any() and G > 1:
                m["zero_fill"] += int((fill & (torch.cat((ov[:g], ov[g + 1:])).amax(0) > 0)).sum())
    # resolve: one claim -> that box; several -> argmax of the overlaps over ALL boxes (first maximum)
    nclaim = claim.sum(0)
    one = nclaim == 1
    agt[one] = claim[:, one].long().argmax(0)
    multi = (nclaim > 1).nonzero().flatten()
    m["n_multi"] = int(multi.numel())
    for a in multi.tolist():
        w = int(ov[:, a].argmax())
        agt[a] = w
        m["n_steal"] += int(not claim[w, a])
        same = (bx == bx[w]).all(1)  # rows with the winner's coordinates have its overlap exactly; argmax takes the first of them
        if ov[w, a] > 0 and (~same).any():
            m["multi_gap"] = min(m["multi_gap"], _gap(ov[w, a], ov[~same, a].max()))
    pos = agt >= 0
    ar = torch.arange(A)
    owner = torch.zeros(G, A, dtype=torch.bool)
    owner[agt[pos], ar[pos]] = True
    pos_align = (metric * owner).amax(1)
    pos_ov = (ov * owner).amax(1)
    g = agt[pos]
    score[pos] = metric[g, ar[pos]] * pos_ov[g] / (pos_align[g] + 1e-9)
    return agt, score, claim, m


@dataclass
class Ref:
    items: torch.Tensor        # (3,) box, cls, dfl
    grads: list                # per level (B, 64 + nc, H, W): d(loss * B) / d(head map)
    assign: torch.Tensor       # (B, A) gt row or -1
    score: torch.Tensor        # (B, A) target score
    claims: list               # per image (n_gt, A) bool: claimant boxes per anchor before the resolve step
    report: dict = field(default_factory=dict)


def loss_ref(feats, gt, n_gt, strides, nc, gains=GAINS):
    """The loss and its gradient in float64.  feats: per level (B, 64 + nc, H, W)."""
    B = feats[0].shape[0]
    hw = [tuple(f.shape[2:]) for f in feats]
    leaves = [f.detach().to(F64).requires_grad_(True) for f in feats]
    rows = torch.cat([x.flatten(2).transpose(1, 2) for x in leaves], 1)  # (B, A, 64 + nc)
    A = rows.shape[1]
    anc, st = anchors(hw, strides)
    logits, cls_logit = rows[..., :4 * REG].reshape(B, A, 4, REG), rows[..., 4 * REG:]
    dist = (logits.softmax(-1) * torch.arange(REG, dtype=F64)).sum(-1)
    pbox = torch.cat((anc - dist[..., :2], anc + dist[..., 2:]), -1)  # grid units
    gt64 = gt.to(F64)
    assign = torch.full((B, A), -1, dtype=torch.long)
    score = torch.zeros(B, A, dtype=F64)
    claims, margins = [], []
    with torch.no_grad():
        for b in range(B):
            a_, s_, c_, m_ = _assign_image(pbox[b] * st[:, None], cls_logit[b].sigmoid(), anc * st[:, None], gt64[b, :int(n_gt[b])])
            assign[b], score[b] = a_, s_
            claims.append(c_)
            margins.append(m_)
    tss = max(float(score.sum()), 1.0)
    # classification: SlideLoss(BCE with logits), auto_iou = 0.5
    pos = assign >= 0
    bi, ai = pos.nonzero(as_tuple=True)
    gi = assign[bi, ai]
    t = torch.zeros(B, A, nc, dtype=F64)
    t[bi, ai, gt64[bi, gi, 0].long()] = score[bi, ai]
    w = torch.where(t <= 0.4, torch.ones_like(t), torch.where(t < 0.5, torch.full_like(t, math.exp(0.5)), torch.exp(1.0 - t)))
    bce = cls_logit.clamp(min=0) - cls_logit * t + torch.log1p(torch.exp(-cls_logit.abs()))
    l_cls = (bce * w).sum()
    l_box = l_dfl = rows.sum() * 0
    coord_gap, n_clamp = math.inf, 0
    if bi.numel():
        tb = gt64[bi, gi, 1:5] / st[ai, None]
        wt = score[bi, ai]
        l_box = ((1.0 - ciou(pbox[bi, ai], tb)) * wt).sum()
        raw = torch.cat((anc[ai] - tb[:, :2], tb[:, 2:] - anc[ai]), 1)
        tg = raw.clamp(0, REG - 1 - 0.01)
        tl = tg.floor().long()
        wl = (tl + 1).to(F64) - tg
        logp = logits[bi, ai].log_softmax(-1)
        ce = -(logp.gather(-1, tl[..., None]).squeeze(-1) * wl + logp.gather(-1, tl[..., None] + 1).squeeze(-1) * (1 - wl))
        l_dfl = (ce.mean(-1) * wt).sum()
        live = wt > 0
        if live.any():
            coord_gap = float((pbox[bi, ai].detach() - tb)[live].abs().min())
            n_clamp = int((raw[live] > REG - 1 - 0.01).any(1).sum())
    items = torch.stack((l_box / tss * gains[0], l_cls / tss * gains[1], l_dfl / tss * gains[2]))
    (items.sum() * B).backward()
    ts = score[pos]
    rep = dict(
        topk_gap=min(m["topk_gap"] for m in margins), multi_gap=min(m["multi_gap"] for m in margins),
        zero_fill=sum(m["zero_fill"] for m in margins), dmin=min(m["dmin"] for m in margins),
        slide_gap=float((ts - 0.4).abs().min()) if ts.numel() else math.inf, coord_gap=coord_gap,
        # what the input contains
        n_pos=int((ts > 0).sum()), band_low=int(((ts > 0) & (ts <= 0.4)).sum()), band_mid=int(((ts > 0.4) & (ts < 0.5)).sum()),
        band_high=int((ts >= 0.5).sum()), n_zero_score=int((ts == 0).sum()), dfl_clamped=n_clamp,
        n_multi=sum(m["n_multi"] for m in margins), n_steal=sum(m["n_steal"] for m in margins),
        n_empty_box=sum(m["n_empty_box"] for m in margins), on_centre=[(b, a) for b, m in enumerate(margins) for a in m["on_centre"]],
        images_without_boxes=int((torch.as_tensor(n_gt) == 0).sum()), images_with_boxes=int((torch.as_tensor(n_gt) > 0).sum()),
        dup_rows=_count_pairs(gt, n_gt, same_class=True), same_box_two_classes=_count_pairs(gt, n_gt, same_class=False))
    return Ref(items.detach(), [x.grad for x in leaves], assign, score, claims, rep)


def _count_pairs(gt, n_gt, same_class):
    """Pairs of valid rows of one image with equal coordinates and equal (or different) classes."""
    n = 0
    for b in range(gt.shape[0]):
        r = gt[b, :int(n_gt[b])]
        eq = (r[:, None, 1:] == r[None, :, 1:]).all(-1) & ((r[:, None, 0] == r[None, :, 0]) == same_class)
        n += int(torch.triu(eq, 1).sum())
    return n


def undecidable(rep):
    """The decisions of an input that float32 rounding could take the other way; empty for a decidable input."""
    bad = []
    if rep["topk_gap"] < REL_GAP:
        bad.append(f"10th / 11th alignment metric of a box {rep['topk_gap']:.3g} apart (relative)")
    if rep["zero_fill"]:
        bad.append(f"{rep['zero_fill']} zero-metric anchors of a box with fewer than 10 positive ones lie under another box's overlap")
    if rep["multi_gap"] < REL_GAP:
        bad.append(f"largest / second overlap of a multiply-claimed anchor {rep['multi_gap']:.3g} apart (relative)")
    if rep["slide_gap"] < SLIDE_GAP:
        bad.append(f"a target score {rep['slide_gap']:.3g} from 0.4")
    if rep["dmin"] < COORD_GAP:
        bad.append(f"an anchor centre {rep['dmin']:.3g} px from a box edge")
    if rep["coord_gap"] < COORD_GAP:
        bad.append(f"a predicted coordinate {rep['coord_gap']:.3g} cells from its target")
    return bad


def on_centre_strides(rep, hw, strides):
    """Strides at which some anchor centre lies exactly on a box edge."""
    a0 = np.cumsum([0] + [h * w for h, w in hw])
    return sorted({float(strides[int(np.searchsorted(a0, a, side="right")) - 1]) for _, a in rep["on_centre"]})


# ---------------------------------------------------------------------------------------------------------------------
# the oracle (oracle/loss.py: the reference's operation order with autograd) on the same pixel values, in either precision
# ---------------------------------------------------------------------------------------------------------------------
def oracle_loss(feats, gt, n_gt, strides, nc, dtype):
    """oracle.loss.v8_detection_loss in `dtype` with its label preprocessing replaced by the packed gt rows.  Returns items (3,),
    the gradients of loss.sum() per level, the assignment (B, A) and the target score (B, A)."""
    import oracle.loss as O
    rows = int(max(int(n) for n in n_gt)) if len(n_gt) else 0
    seen = {}
    prep, call = O.preprocess_targets, O.TaskAlignedAssigner.__call__

    def record(self, *a):
        out = call(self, *a)
        seen["gt"], seen["score"] = torch.where(out[3].bool(), out[4].long(), -1), out[2].sum(-1)
        return out

    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    O.preprocess_targets = lambda *a: gt[:, :rows].to(dtype).clone()
    O.TaskAlignedAssigner.__call__ = record
    try:
        fr = [f.detach().to(dtype).requires_grad_(True) for f in feats]
        loss, items = O.v8_detection_loss(fr, dict(batch_idx=None, cls=None, bboxes=None), torch.tensor(list(strides), dtype=dtype), nc=nc,
                                          gains=dict(box=GAINS[0], cls=GAINS[1], dfl=GAINS[2]))
        loss.sum().backward()
    finally:
        torch.set_default_dtype(old)
        O.preprocess_targets, O.TaskAlignedAssigner.__call__ = prep, call
    return items, [f.grad for f in fr], seen["gt"], seen["score"]


def effective(assign, score):
    """The assignment as far as it carries loss: a positive anchor with target score 0 weighs nothing in any term, and whether the
    zero-metric fill of a short top-k makes it one is the unspecified part of torch.topk."""
    return torch.where(score > 0, assign, torch.full_like(assign, -1))


# ---------------------------------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------------------------------
def pack(per_image, max_gt):
    """per_image: list (one per image) of [cls, x1, y1, x2, y2] rows -> gt (B, max_gt, 5) float32, n_gt (B,) int32."""
    gt = torch.zeros(len(per_image), max_gt, 5)
    for b, r in enumerate(per_image):
        if len(r):
            gt[b, :len(r)] = torch.tensor(r, dtype=torch.float32)
    return gt, torch.tensor([len(r) for r in per_image], dtype=torch.int32)


def uniform_maps(key, B, hw, nc):
    """The family of tests/test_hip_train.py: every logit uniform in [-2, 2], the class logits moved to [-7, 1]."""
    feats = [P.uniform(f"{key}:{i}", (B, 4 * REG + nc, h, w), -2, 2) for i, (h, w) in enumerate(hw)]
    for f in feats:
        f[:, 4 * REG:] = f[:, 4 * REG:] * 2 - 3
    return feats


def trained_like_maps(key, B, hw, strides, nc, gt, n_gt, height=4.0, jitter=0.7, box_levels=None):
    """Head maps as a partly trained model gives them.  Every anchor inside a box predicts the smallest box around it: its DFL logits
    get a bump of `height` around the true distance, moved by up to `jitter` bins times a per-anchor sloppiness in [0, 2), and the class
    logit of that box (and of rows with the same coordinates) is raised by 2 on a background of -3 +- 0.6.  `box_levels[(b, g)]`
    restricts a box to some levels."""
    feats = []
    k = np.arange(REG, dtype=np.float64)
    for l, ((h, w), s) in enumerate(zip(hw, strides)):
        dfl0 = P.hash_uniform(f"{key}:dfl:{l}", B * h * w * 4 * REG).astype(np.float64).reshape(B, h, w, 4, REG) - 0.5
        cls0 = -3.0 + 0.6 * (2 * P.hash_uniform(f"{key}:cls:{l}", B * h * w * nc).astype(np.float64).reshape(B, h, w, nc) - 1)
        dfl, cls = dfl0.copy(), cls0.copy()
        jit = jitter * (2 * P.hash_uniform(f"{key}:jit:{l}", B * h * w * 4).astype(np.float64).reshape(B, h, w, 4) - 1)
        jit *= 2 * P.hash_uniform(f"{key}:sloppy:{l}", B * h * w).astype(np.float64).reshape(B, h, w, 1)
        cx, cy = np.meshgrid(np.arange(w) + 0.5, np.arange(h) + 0.5)
        for b in range(B):
            rows = gt[b, :int(n_gt[b])].double().numpy()
            area = (rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2]) if len(rows) else np.zeros(0)
            for g in np.argsort(-area, kind="stable"):  # smaller boxes overwrite larger ones
                if box_levels and l not in box_levels.get((b, int(g)), range(len(hw))):
                    continue
                x1, y1, x2, y2 = rows[g, 1:] / s
                inside = np.minimum(np.minimum(cx - x1, cy - y1), np.minimum(x2 - cx, y2 - cy)) > 0
                if not inside.any():
                    continue
                d = np.stack((cx - x1, cy - y1, x2 - cx, y2 - cy), -1)[inside] + jit[b][inside]
                d = np.clip(d, 0, REG - 1)
                dfl[b][inside] = dfl0[b][inside] + height * np.exp(-(k - d[..., None]) ** 2 / (2 * 0.6 ** 2))
                c0 = cls0[b][inside]
                for c in rows[(rows[:, 1:] == rows[g, 1:]).all(1), 0]:
                    c0[:, int(c)] += 2.0
                cls[b][inside] = c0
        f = np.concatenate((dfl.reshape(B, h, w, 4 * REG), cls), -1).astype(np.float32)
        feats.append(torch.from_numpy(f).permute(0, 3, 1, 2).contiguous())
    return feats


def set_prediction(feats, strides, b, level, y, x, box, cls_logits):
    """Make anchor (level, y, x) of image b predict `box` (pixels) and set some of its class logits.  Every distance must be a whole or
    half number of cells below 15: one bin (or two equal neighbours) at 30 above the rest gives that expectation to 1e-11."""
    s = strides[level]
    d = [x + 0.5 - box[0] / s, y + 0.5 - box[1] / s, box[2] / s - x - 0.5, box[3] / s - y - 0.5]
    for side, v in enumerate(d):
        assert 2 * v == int(2 * v) and 0 <= v < REG - 1, d
        feats[level][b, side * REG:(side + 1) * REG, y, x] = 0.0
        feats[level][b, side * REG + int(v), y, x] = 30.0
        if v != int(v):
            feats[level][b, side * REG + int(v) + 1, y, x] = 30.0
    for c, v in cls_logits.items():
        feats[level][b, 4 * REG + c, y, x] = v


def refusals_precede_launches():
    """True when, in the source of upa_detection_loss_scaled, the anchor-count and LDS-row checks stand before the first launch.  The
    refusal tests ask this before they hand the GPU a shape whose top-k would write out of range on a build without the checks."""
    from pathlib import Path
    src = (Path(__file__).resolve().parent.parent / "ultralytics_pro_amd" / "csrc" / "loss.hip").read_text()
    body = src[src.rindex('extern "C" int upa_detection_loss_scaled'):]
    first = min(body.index(k) for k in ("hipLaunchKernelGGL", "upa_zero_words"))
    return all(0 <= body.find(k) < first for k in ("UPA_CHECK_ARG(a >= TOPK", "do not fit the LDS metric row", "workspace too small"))


# ---------------------------------------------------------------------------------------------------------------------
# the case table: every input of tests/test_hip_loss.py
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class Inputs:
    feats: list
    gt: torch.Tensor
    n_gt: torch.Tensor
    hw: tuple
    strides: tuple
    nc: int

    @property
    def B(self):
        return int(self.gt.shape[0])

    @property
    def max_gt(self):
        return int(self.gt.shape[1])


@dataclass(frozen=True)
class Case:
    name: str
    pins: str                 # what the case is there for
    contains: tuple = ()      # report keys that must count at least 1 (checked on the CPU)
    layout: tuple = None      # GPU only: (pixel pitch, first float of the slice in its row); None = a dense map of pitch 64 + nc
    source: str = None        # the case whose input this one shares (layout cases)


# image 0 of the base input: a 160 x 96 image.  Row 0 covers the whole image and is shown to stride 8 only, where the anchors left
# of x = 40 and right of x = 120 are further than 14.99 cells from the far edge; the middle belongs to row 1.
_BASE_BOXES = [
    [[0, 0, 0, 160, 96], [1, 41, 3, 119, 93], [2, 9.3, 10.1, 38.2, 50.7], [3, 100.5, 30.2, 150.1, 90.3], [4, 60.7, 20.4, 110.2, 70.9],
     [4, 60.7, 20.4, 110.2, 70.9],          # a duplicated row
     [5, 100.5, 30.2, 150.1, 90.3],         # the box of row 3 under another class
     [6, 13, 60.5, 19, 67.5]],              # no anchor centre inside (stride-8 centres at 12 / 20, 60 / 68)
    [],                                      # an image without boxes
    [[7, 20.3, 8.8, 90.4, 80.2], [0, 70.1, 30.6, 140.8, 88.9], [2, 5.2, 40.3, 60.9, 92.1], [1, 118.4, 6.3, 154.7, 44.2]],
]


def _mod_classes(boxes, nc):
    return [[[r[0] % nc] + r[1:] for r in img] for img in boxes]


def _base(nc, hw=HW, strides=STRIDES, max_gt=64, key="base", jitter=0.7):
    gt, n_gt = pack(_mod_classes(_BASE_BOXES, nc), max_gt)
    feats = trained_like_maps(f"loss:{key}", 3, hw, strides, nc, gt, n_gt, jitter=jitter, box_levels={(0, 0): (0,)})
    return Inputs(feats, gt, n_gt, tuple(hw), tuple(strides), nc)


def _steal():
    """Image 0: rows 0 and 1 are small boxes around the stride-8 anchor (y 6, x 6), centre (52, 52), with at most 6 anchors inside
    each, so each claims every one of them.  That anchor predicts (28, 28, 84, 76), all but row 2, and scores row 2's class at -12: its
    overlap with row 2 is the largest, its alignment metric for row 2 is far from row 2's ten best."""
    boxes = [[[0, 43, 43, 59, 59], [1, 45, 45, 61, 61], [2, 28.8, 27.4, 83.1, 76.9], [3, 100.5, 10.2, 150.1, 60.3]],
             [[4, 20.3, 8.8, 90.4, 80.2]], [[5, 70.1, 30.6, 140.8, 88.9], [6, 5.2, 40.3, 60.9, 92.1]]]
    gt, n_gt = pack(boxes, 64)
    feats = trained_like_maps("loss:steal", 3, HW, STRIDES, 8, gt, n_gt)
    set_prediction(feats, STRIDES, 0, 0, 6, 6, (28, 28, 84, 76), {0: 1.0, 1: 1.0, 2: -12.0})
    return Inputs(feats, gt, n_gt, HW, STRIDES, 8)


# image 0 of the on-centre input: (level, y, x, row) of one anchor on the left edge of each row that predicts the row exactly
ON_EDGE = ((0, 2, 1, 0), (1, 1, 1, 1), (2, 1, 0, 2))


def _on_centre():
    """Box edges exactly on anchor centres: row 0 on stride-8 centres (4 + 8 k), row 1 on stride-16 centres (8 + 16 k), row 2 on
    stride-32 centres (16 + 32 k), each on no centre of the other strides.  All values are exact in float32.  One edge anchor per
    row predicts that row exactly and scores its class high: an in-box test that lets the edge in makes it the row's best positive."""
    boxes = [[[0, 12, 12, 60, 60], [1, 24, 8, 88, 72], [2, 16, 16, 112, 80]], [[3, 76, 20, 148, 84]], [[4, 8, 24, 72, 88], [5, 48, 16, 144, 80]]]
    gt, n_gt = pack(boxes, 64)
    feats = trained_like_maps("loss:centre", 3, HW, STRIDES, 8, gt, n_gt)
    for level, y, x, g in ON_EDGE:  # were the edge inside, these would be the best anchors of their boxes
        set_prediction(feats, STRIDES, 0, level, y, x, boxes[0][g][1:], {g: 3.0})
    return Inputs(feats, gt, n_gt, HW, STRIDES, 8)


def _empty(max_gt):
    gt, n_gt = pack([[], [], []], max_gt)
    return Inputs(trained_like_maps(f"loss:empty{max_gt}", 3, HW, STRIDES, 8, gt, n_gt), gt, n_gt, HW, STRIDES, 8)


def _uniform():
    """The [-2, 2] family: every DFL expectation is about 7.5 bins, so every predicted box is about 15 cells wide.  The boxes are as
    wide as the stride-8 predictions (and the image), so that more than ten anchors per box have a positive overlap."""
    boxes = [[[0, 20.5, 3.3, 140.2, 93.1], [5, 2.2, 2.7, 118.6, 90.4]], [[3, 40.9, 1.6, 158.3, 94.8]], [[6, 10.4, 5.1, 150.7, 91.2]]]
    gt, n_gt = pack(boxes, 64)
    return Inputs(uniform_maps("loss:uniform", 3, HW, 8), gt, n_gt, HW, STRIDES, 8)


def _one_box_each():
    boxes = [[[0, 20.3, 8.8, 90.4, 80.2]], [[1, 70.1, 30.6, 140.8, 88.9]], [[2, 5.2, 40.3, 60.9, 92.1]]]
    gt, n_gt = pack(boxes, 1)
    return Inputs(trained_like_maps("loss:maxgt1", 3, HW, STRIDES, 8, gt, n_gt), gt, n_gt, HW, STRIDES, 8)


def _crowd192():
    """Image 0: 192 boxes of 6.6 x 6.6 px, each around one stride-8 anchor centre and holding no other centre; image 1: three boxes."""
    tiny = [[(i * 7) % 8, 4 + 8 * (i % 16) - 3.3, 4 + 8 * (i // 16) - 3.3, 4 + 8 * (i % 16) + 3.3, 4 + 8 * (i // 16) + 3.3] for i in range(192)]
    gt, n_gt = pack([tiny, _BASE_BOXES[2][:3]], 192)
    return Inputs(trained_like_maps("loss:crowd", 2, HW, STRIDES, 8, gt, n_gt), gt, n_gt, HW, STRIDES, 8)


def _cap1024():
    gt, n_gt = pack([_BASE_BOXES[2][:3], _BASE_BOXES[2][1:3]], 1024)
    return Inputs(trained_like_maps("loss:cap", 2, HW, STRIDES, 8, gt, n_gt), gt, n_gt, HW, STRIDES, 8)


def _full_grid():
    """The 640 x 640 anchor grid (A = 8400) with 6 boxes."""
    hw = ((80, 80), (40, 40), (20, 20))
    boxes = [[[0, 50.3, 60.8, 250.4, 300.2], [1, 300.1, 100.6, 600.8, 400.9], [2, 100.2, 400.3, 180.9, 520.1], [3, 400.5, 450.5, 440.5, 500.5]],
             [[4, 20.4, 30.3, 620.7, 610.2], [5, 200.6, 250.1, 330.3, 390.8]]]
    gt, n_gt = pack(boxes, 64)
    return Inputs(trained_like_maps("loss:full", 2, hw, STRIDES, 8, gt, n_gt), gt, n_gt, hw, STRIDES, 8)


_BUILDERS = {
    "base": lambda: _base(8, key="base7"),
    "steal": _steal,
    "on_centre": _on_centre,
    "empty_maxgt1": lambda: _empty(1),
    "empty_maxgt64": lambda: _empty(64),
    "uniform": _uniform,
    "nc1": lambda: _base(1, key="nc1"),
    "nc6": lambda: _base(6, key="nc6"),
    "nc80": lambda: _base(80, key="nc80"),
    "levels1": lambda: _base(8, hw=HW[:1], strides=STRIDES[:1], key="levels1"),
    "levels2": lambda: _base(8, hw=HW[:2], strides=STRIDES[:2], key="levels2"),
    "maxgt1": _one_box_each,
    "maxgt192_full": _crowd192,
    "maxgt1024": _cap1024,
    "a8400": _full_grid,
}

_BASE_HOLDS = ("band_low", "band_mid", "band_high", "dfl_clamped", "n_empty_box", "dup_rows", "same_box_two_classes", "images_without_boxes",
               "images_with_boxes", "n_multi")

CASES = [
    Case("base", "trained-like maps, nc 8: an image without boxes, all three SlideLoss bands, a duplicated row, one box under two classes, "
         "a box with no anchor centre inside, a box covering the whole image (DFL clamp at stride 8)", _BASE_HOLDS),
    Case("steal", "an anchor claimed by two boxes and won by a third that did not claim it", ("n_steal",)),
    Case("on_centre", "box edges exactly on anchor centres at strides 8, 16 and 32", ("n_pos",)),
    Case("empty_maxgt1", "no boxes at all, max_gt 1"),
    Case("empty_maxgt64", "no boxes at all, max_gt 64"),
    Case("uniform", "the [-2, 2] logits of tests/test_hip_train.py with wide boxes", ("n_pos",)),
    Case("nc1", "one class: the scalar class kernel", ("n_pos",)),
    Case("nc6", "six classes: the scalar class kernel", ("n_pos",)),
    Case("nc80", "eighty classes: the four-wide class kernel", ("n_pos",)),
    Case("pitch75", "pixel pitch 75: ld % 4 != 0, the scalar class kernel on nc 8", layout=(75, 0), source="base"),
    Case("pitch80_off1", "pixel pitch 80, the slice one float into the row: pointers not 16-byte aligned", layout=(80, 1), source="base"),
    Case("pitch96", "pixel pitch 96, aligned slice: the four-wide class kernel on a strided view", layout=(96, 0), source="base"),
    Case("levels1", "n_levels 1, a (12, 20) map at stride 8", ("n_pos",)),
    Case("levels2", "n_levels 2", ("n_pos",)),
    Case("maxgt1", "max_gt 1 with one box per image", ("n_pos",)),
    Case("maxgt192_full", "max_gt 192 with n_gt == max_gt in image 0 (tiny boxes)", ("n_pos",)),
    Case("maxgt1024", "max_gt at its cap of 1024 with 3 valid rows", ("n_pos",)),
    Case("a8400", "the 640 x 640 anchor grid, B = 2, 6 boxes: 33.6 KB of the LDS metric row", ("n_pos",)),
]
CASE = {c.name: c for c in CASES}
INPUT_NAMES = [c.name for c in CASES if c.source is None]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """The input of a case (shared, never modified)."""
    return _BUILDERS[CASE[name].source or name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """loss_ref of a case's input, computed once per process."""
    i = inputs(name)
    return loss_ref(i.feats, i.gt, i.n_gt, i.strides, i.nc)


@functools.lru_cache(maxsize=None)
def oracle32(name):
    """The float32 oracle of a case's input: what a float32 implementation in the reference's operation order achieves."""
    i = inputs(name)
    return oracle_loss(i.feats, i.gt, i.n_gt, i.strides, i.nc, torch.float32)
