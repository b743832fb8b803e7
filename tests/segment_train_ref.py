"""float64 references of the two segmentation-training entries (test infrastructure): the gradients of ConvTranspose2d(2, 2, 0) and the
mask term of v8SegmentationLoss (utils/loss.py:622-709, crop_mask's comparison branch utils/ops.py:510-513) with its gradients, each
with the operand-magnitude sums the kernel tests build their bounds from (tests/kernel_check.py: K u S + u |ref|).  Written out by hand
- no autograd - so that tests/test_segment_train_ref.py can hold them to torch autograd of the reference formula."""

import torch
import torch.nn.functional as F

from tests.kernel_check import ZERO_PASS_ITEMS, ZERO_PASS_LEVELS
from tests.kernel_check import zero_pass_items as _zero_pass_items


def convt_bwd_ref(x, dy, w):
    """x (n, h, w, cin), dy (n, 2h, 2w, cout), w (cin, cout, 2, 2), any dtype -> float64 (dx, dw, db) and the magnitude sums
    (sum of |products|) of each."""
    x, dy, w = x.double(), dy.double(), w.double()
    n, h, ww, _ = x.shape
    u = dy.view(n, h, 2, ww, 2, -1)  # [n, y, i, x, j, co]
    dx = torch.einsum("nyixjo,coij->nyxc", u, w)
    dw = torch.einsum("nyxc,nyixjo->coij", x, u)
    db = dy.sum((0, 1, 2))
    mags = (torch.einsum("nyixjo,coij->nyxc", u.abs(), w.abs()), torch.einsum("nyxc,nyixjo->coij", x.abs(), u.abs()), dy.abs().sum((0, 1, 2)))
    return (dx, dw, db), mags


def mask_boxes(gt, imgsz_h, imgsz_w, mh, mw):
    """loss.py:683-689 in float32, as the reference computes it: (boxes in mask units (..., 4) f32, normalised area (...) f32)."""
    g = gt[..., 1:5].float()
    scale = torch.tensor([imgsz_w, imgsz_h, imgsz_w, imgsz_h], dtype=torch.float32)
    nb = g / scale
    area = (nb[..., 2] - nb[..., 0]) * (nb[..., 3] - nb[..., 1])
    return nb * torch.tensor([mw, mh, mw, mh], dtype=torch.float32), area


def mask_loss_ref(proto, coefs, assign, gt, n_gt, mask_id, masks, imgsz_h, imgsz_w, gain, scale, u_in=2.0 ** -24, **_):
    """proto (b, mh, mw, nm); coefs: per level (b, h, w, nm); assign (b, A) gt row or -1 (rows >= n_gt: background); gt (b, G, 5) pixel
    xyxy behind the class; mask_id (b, G); masks (b, mh, mw) integers.  The crop decisions and the box scaling are float32 (the
    reference's own arithmetic), everything else float64.  Returns dict(item, dproto, dcoefs (per level), and *_err: the float32
    evaluation-error bounds of each, without the output rounding) for gradients of item * b * scale.
    Error model of the kernels (u = 2^-24): pred = an nm-term f32 dot -> |d pred| <= (nm + 2) u sum|c p|; sigmoid / BCE of it: slope
    <= 1/4 / <= 1, plus 8 u for expf / log1pf / the divide; a sum of N f32 products: (N + 8) u sum|terms|."""
    b, mh, mw, nm = proto.shape
    P = proto.double()
    flat = torch.cat([c.double().reshape(b, -1, nm) for c in coefs], 1)  # (b, A, nm)
    A = flat.shape[1]
    mbox, area = mask_boxes(gt, imgsz_h, imgsz_w, mh, mw)
    xs = torch.arange(mw, dtype=torch.float32).view(1, -1)
    ys = torch.arange(mh, dtype=torch.float32).view(-1, 1)
    fg = [(i, a, int(assign[i, a])) for i in range(b) for a in range(A) if 0 <= int(assign[i, a]) < int(n_gt[i])]
    ntot = len(fg)
    dproto, dflat = torch.zeros_like(P), torch.zeros_like(flat)
    eproto, eflat = torch.zeros_like(P), torch.zeros_like(flat)
    mproto = torch.zeros_like(P)
    item = item_err = 0.0
    per_img = [sum(1 for f in fg if f[0] == i) for i in range(b)]
    for i, a, g in fg:
        x1, y1, x2, y2 = (mbox[i, g, k] for k in range(4))
        crop = ((xs >= x1) & (xs < x2) & (ys >= y1) & (ys < y2)).double()  # (mh, mw)
        wgt = 1.0 / (mh * mw) / float(area[i, g].double())
        c = flat[i, a]
        pred = P[i] @ c
        t = (masks[i].long() == int(mask_id[i, g])).double()
        bce = F.binary_cross_entropy_with_logits(pred, t, reduction="none")
        dpred_err = (nm + 2) * u_in * (P[i].abs() @ c.abs())
        npx = float(crop.sum())
        item += wgt * float((bce * crop).sum())
        item_err += wgt * (float(((dpred_err + 8 * u_in * (bce + 1)) * crop).sum()) + (npx / 64 + 72) * u_in * float((bce * crop).sum()))
        k = gain * b * scale / ntot * wgt
        dp = (torch.sigmoid(pred) - t) * crop
        dp_err = (0.25 * dpred_err + 8 * u_in) * crop
        dflat[i, a] = k * (dp.unsqueeze(-1) * P[i]).sum((0, 1))
        eflat[i, a] = k * ((dp_err.unsqueeze(-1) * P[i].abs()).sum((0, 1)) + (npx / 64 + 72) * u_in * (dp.abs().unsqueeze(-1) * P[i].abs()).sum((0, 1)))
        dproto[i] += k * dp.unsqueeze(-1) * c
        eproto[i] += k * dp_err.unsqueeze(-1) * c.abs()
        mproto[i] += k * dp.abs().unsqueeze(-1) * c.abs()
    for i in range(b):
        eproto[i] += (per_img[i] + 8) * u_in * mproto[i]
    if ntot:
        item, item_err = gain * item / ntot, gain * item_err / ntot + 4 * u_in * gain * item / ntot
    out = dict(item=item, item_err=item_err, dproto=dproto, dproto_err=eproto, n_fg=ntot, dcoefs=[], dcoefs_err=[])
    a0 = 0
    for cf in coefs:
        _, h, w, _ = cf.shape
        out["dcoefs"].append(dflat[:, a0:a0 + h * w].reshape(b, h, w, nm))
        out["dcoefs_err"].append(eflat[:, a0:a0 + h * w].reshape(b, h, w, nm))
        a0 += h * w
    return out


def mask_loss_autograd(proto, coefs, assign, gt, n_gt, mask_id, masks, imgsz_h, imgsz_w, gain, scale, **_):
    """The reference formula itself (tests/segment_train_oracle.mask_term's ops) under float64 autograd: (item, dproto, dcoefs)."""
    from tests.segment_train_oracle import crop_mask_compare
    b, mh, mw, nm = proto.shape
    P = proto.double().clone().requires_grad_(True)
    cs = [c.double().clone().requires_grad_(True) for c in coefs]
    flat = torch.cat([c.reshape(b, -1, nm) for c in cs], 1)
    mbox, area = mask_boxes(gt, imgsz_h, imgsz_w, mh, mw)
    fgm = (assign >= 0) & (assign < n_gt.view(-1, 1))
    loss = 0
    for i in range(b):
        if not fgm[i].any():
            continue
        g = assign[i][fgm[i]].long()
        gt_mask = (masks[i].long() == mask_id[i][g].long().view(-1, 1, 1)).double()
        pred = torch.einsum("in,nhw->ihw", flat[i][fgm[i]], P[i].permute(2, 0, 1))
        bce = F.binary_cross_entropy_with_logits(pred, gt_mask, reduction="none")
        loss = loss + (crop_mask_compare(bce, mbox[i][g].double()).mean(dim=(1, 2)) / area[i][g].double()).sum()
    if not bool(fgm.any()):
        return 0.0, torch.zeros_like(P), [torch.zeros_like(c) for c in cs]
    item = loss / fgm.sum() * gain
    (item * b * scale).backward()
    return float(item.detach()), P.grad, [c.grad for c in cs]


def mask_case_no_foreground(dtype=torch.float32):
    """Image 0 of `mask_case` alone (b = 1) with every anchor background."""
    c = mask_case(dtype=dtype)
    for k in ("proto", "assign", "gt", "n_gt", "mask_id", "masks"):
        c[k] = c[k][:1].clone()
    c["coefs"] = [t[:1].clone() for t in c["coefs"]]
    c["assign"][:] = -1
    return c


def mask_case(b=3, mh=12, mw=20, nm=32, levels=((4, 5), (2, 3), (1, 2)), imgsz=(48, 80), dtype=torch.float32):
    """The kernel test's inputs (values representable in `dtype`): image 0 - three gts: two anchors on gt 0, a box reaching past the
    mask edge (gt 1), a box narrower than one mask pixel between two pixel centres (gt 2: no pixel passes, the term is exactly 0), mask
    ids that are not row + 1 and instance ids above 1 painted over each other; image 1 - gts but no foreground anchor; image 2 -
    assignments but n_gt = 0."""
    from ultralytics_pro_amd.utils import procedural as P

    def rnd(name, shape, lo, hi):
        return P.uniform(f"seg_train:{name}", shape, lo, hi).to(dtype).float()
    proto = rnd("proto", (b, mh, mw, nm), -1.0, 1.0)
    coefs = [rnd(f"coef{l}", (b, h, w, nm), -0.5, 0.5) for l, (h, w) in enumerate(levels)]
    A = sum(h * w for h, w in levels)
    G = 4
    ih, iw = imgsz  # mask units = pixels / 4
    gt = torch.zeros(b, G, 5)
    gt[0, 0, 1:] = torch.tensor([9.0, 6.0, 50.0, 37.0])      # an ordinary box (mask units 2.25 .. 12.5, 1.5 .. 9.25)
    gt[0, 1, 1:] = torch.tensor([41.0, 18.0, 90.0, 55.0])    # reaches past the right and bottom edges
    gt[0, 2, 1:] = torch.tensor([20.5, 10.0, 23.5, 30.0])    # mask units x in (5.125, 5.875): no integer x passes x >= x1 & x < x2
    gt[1, 0, 1:] = torch.tensor([5.0, 5.0, 30.0, 30.0])
    gt[1, 1, 1:] = torch.tensor([30.0, 10.0, 60.0, 40.0])
    gt[2, 0, 1:] = torch.tensor([8.0, 8.0, 40.0, 40.0])
    n_gt = torch.tensor([3, 2, 0], dtype=torch.int32)
    mask_id = torch.zeros(b, G, dtype=torch.int32)
    mask_id[0, :3] = torch.tensor([2, 4, 5], dtype=torch.int32)  # a dropped box in front of gt 0 and another before gt 1: not row + 1
    mask_id[1, :2] = torch.tensor([1, 2], dtype=torch.int32)
    mask_id[2, 0] = 1
    masks = torch.zeros(b, mh, mw, dtype=torch.uint8)
    masks[0, 1:9, 2:12] = 2
    masks[0, 4:12, 9:20] = 4      # painted over instance 2
    masks[0, 2:8, 5:7] = 5        # ... and over both
    masks[0, 0:3, 0:4] = 3        # an instance nobody is assigned to
    masks[1, 1:8, 1:8] = 1
    masks[2, 2:10, 2:10] = 1
    assign = torch.full((b, A), -1, dtype=torch.int32)
    assign[0, 6] = 0
    assign[0, 7] = 0              # two anchors on the same gt
    assign[0, 13] = 1
    assign[0, 21] = 1             # level 1
    assign[0, 27] = 2             # level 2: the sub-pixel box
    assign[2, 3] = 0              # n_gt = 0: background whatever the array says
    assign[2, 25] = 0
    return dict(proto=proto, coefs=coefs, assign=assign, gt=gt, n_gt=n_gt, mask_id=mask_id, masks=masks, imgsz_h=ih, imgsz_w=iw,
                gain=7.5, scale=1.0)


# ---- case families past one tile (tests/test_segment_train_ref.py asserts that each holds what its name says) ---------------------------
REFUSALS = ("null pointer", "mask_loss: bad shape", "outside f32 | bf16", "coefficients, a multiple of 16 bytes", "bad view",
            "stride / address must be multiples of 16 bytes", "past the kernels' index range", "workspace too small")
TURN_LEVELS = ((20, 20), (10, 10), (5, 5))          # A = 525: three 256-anchor compaction turns, the last of 13 anchors
DEPTHS = {torch.float32: (4, 12, 20, 64, 128), torch.bfloat16: (8, 24, 64, 128)}
CONVT_EXTRA = {  # (n, h, w, cin, cout) past one 64 x 64 tile, per dtype (cin, cout: multiples of 16 bytes)
    torch.float32: [(1, 6, 5, 72, 16), (2, 5, 7, 24, 8), (1, 9, 4, 40, 24), (1, 3, 3, 128, 128), (1, 33, 31, 16, 16), (2, 64, 64, 16, 16)],
    torch.bfloat16: [(1, 6, 5, 80, 16), (2, 5, 7, 24, 8), (1, 9, 4, 40, 24), (1, 3, 3, 128, 128), (1, 33, 31, 16, 16), (2, 64, 64, 16, 16)],
}


def refusals_precede_launches():
    """True when, in the source of upa_mask_loss, every refusal stands before the first launch (tests/pose_train_ref's check for
    upa_kpt_loss).  The GPU refusal test asks this before it hands the entry sizes a build without the checks would read out of
    range with."""
    from pathlib import Path
    src = (Path(__file__).resolve().parent.parent / "ultralytics_pro_amd" / "csrc" / "segment_train.hip").read_text()
    body = src[src.rindex('extern "C" int upa_mask_loss('):]
    first = body.index("hipLaunchKernelGGL")
    return all(0 <= body.find(k) < first for k in REFUSALS)


def ctb_splits(cin, cout, npix, kdepth):
    """csrc/segment_train.hip's split-K arithmetic of the weight gradient: (splits, pixels per split)."""
    cdiv = (lambda a, b: (a + b - 1) // b)
    cap = min(max(512 // (cdiv(4 * cout, 64) * cdiv(cin, 64)), 1), 64)
    splits = min(max(cdiv(npix, 128), 1), cap)
    kc = cdiv(cdiv(npix, splits), kdepth) * kdepth
    return cdiv(npix, kc), kc


def anchor_lanes(case):
    """The slot lanes upa_mask_loss launches per image: min(10 max_gt, A, 512)."""
    A = case["assign"].shape[1]
    return min(10 * case["gt"].shape[1], A, 512)


def zero_pass_items(case, dtype):
    """The 16-byte stores of ml_zero_bg_kernel's index space: b A (nm / vec)."""
    return _zero_pass_items(case["assign"].numel(), case["proto"].shape[3], dtype)


def foreground(case):
    """Per image: the sorted foreground anchor indices."""
    a, n = case["assign"], case["n_gt"]
    return [((a[i] >= 0) & (a[i] < n[i])).nonzero().flatten().tolist() for i in range(a.shape[0])]


def _scene(tag, b, mh, mw, nm, levels, G, dtype):
    from ultralytics_pro_amd.utils import procedural as P

    def rnd(name, shape, lo, hi):
        return P.uniform(f"seg_train:{tag}:{name}", shape, lo, hi).to(dtype).float()
    A = sum(h * w for h, w in levels)
    return dict(proto=rnd("proto", (b, mh, mw, nm), -1.0, 1.0),
                coefs=[rnd(f"coef{l}", (b, h, w, nm), -0.5, 0.5) for l, (h, w) in enumerate(levels)],
                assign=torch.full((b, A), -1, dtype=torch.int32), gt=torch.zeros(b, G, 5), n_gt=torch.zeros(b, dtype=torch.int32),
                mask_id=torch.zeros(b, G, dtype=torch.int32), masks=torch.zeros(b, mh, mw, dtype=torch.uint8), imgsz_h=4 * mh,
                imgsz_w=4 * mw, gain=7.5, scale=1.0)


def _paint(case, i, boxes):
    """gt rows, ids (row + 2: never row + 1) and the overlap mask of image i: each box's interior painted over the earlier ones."""
    mh, mw = case["masks"].shape[1:]
    sy, sx = case["imgsz_h"] / mh, case["imgsz_w"] / mw
    for g, bx in enumerate(boxes):
        case["gt"][i, g, 1:] = torch.tensor(bx)
        case["mask_id"][i, g] = g + 2
        x1, y1, x2, y2 = (int(min(max(v, 0), 10 ** 6)) for v in (bx[0] / sx + 1, bx[1] / sy + 1, bx[2] / sx - 1, bx[3] / sy - 1))
        if x2 > x1 and y2 > y1:
            case["masks"][i, y1:y2, x1:x2] = g + 2
    case["n_gt"][i] = len(boxes)


# pixel xyxy on the 160 x 96 image of a 40 x 24 mask (mask units = pixels / 4): a box wholly inside the 8 x 8 tile at (16, 8); the
# whole mask (960 pixels: fifteen 64-pixel turns of the anchor kernel); 27 x 18 = 486 mask pixels (more than 4 x 64 and no multiple of
# 64: a partial last turn); a box past the right and bottom edges
TURN_BOXES = [(66.0, 34.0, 90.0, 58.0), (0.0, 0.0, 160.0, 96.0), (13.0, 9.0, 123.0, 79.5), (101.0, 50.0, 190.0, 120.0)]


def turns_case(dtype=torch.float32, permute=0):
    """b = 3 on TURN_LEVELS, nm 32, mask 24 x 40, G = 4.  Image 0: foreground at 0, 255, 256, 399, 400 (first of level 1), 499, 500
    (first of level 2), 524.  Image 1: nothing in 0..255, six in 256..511.  Image 2: every anchor, on gt (7 a + 2 + permute) % 4: 525
    slots on 40 lanes.  permute: the same foreground anchors on other gts."""
    c = _scene("turns", 3, 24, 40, 32, TURN_LEVELS, 4, dtype)
    for i in range(3):
        _paint(c, i, TURN_BOXES if i != 1 else TURN_BOXES[:3])
    for j, a in enumerate((0, 255, 256, 399, 400, 499, 500, 524)):
        c["assign"][0, a] = (j + permute) % 4
    for j, a in enumerate((256, 261, 356, 399, 400, 511)):
        c["assign"][1, a] = (j + permute) % 3
    c["assign"][1, 7] = 3                     # row 3 >= n_gt[1] = 3: background, inside the empty first turn
    c["assign"][2] = ((torch.arange(525) * 7 + 2 + permute) % 4).to(torch.int32)
    return c


def clamp_case(dtype=torch.float32, permute=0):
    """b = 2 on TURN_LEVELS with G = 52: image 0 has every anchor foreground on gt (7 a + permute) % 52 - 525 slots on the 512 lanes
    the grid is clamped to, lanes 0..12 take a second turn; image 1 has three foreground anchors.  The boxes are procedural, on
    quarter pixels."""
    from ultralytics_pro_amd.utils import procedural as P
    c = _scene("clamp", 2, 24, 40, 32, TURN_LEVELS, 52, dtype)
    xy = P.uniform("seg_train:clamp:xy", (2, 52, 2), 0.0, 1.0)
    wh = P.uniform("seg_train:clamp:wh", (2, 52, 2), 0.05, 0.6)
    for i in range(2):
        boxes = []
        for g in range(52):
            x1, y1 = float(xy[i, g, 0]) * 130.0 - 5.0, float(xy[i, g, 1]) * 80.0 - 5.0
            bx = (x1, y1, x1 + float(wh[i, g, 0]) * 160.0 + 2.0, y1 + float(wh[i, g, 1]) * 96.0 + 2.0)
            boxes.append(tuple(round(v * 4) / 4 for v in bx))
        _paint(c, i, boxes)
    c["assign"][0] = ((torch.arange(525) * 7 + permute) % 52).to(torch.int32)
    for j, a in enumerate((3, 300, 520)):
        c["assign"][1, a] = (11 * j + permute) % 52
    return c


def levels_case(n_levels, dtype=torch.float32):
    """The default scene cut down to its first one or two levels (anchors past them and their assignments dropped)."""
    c = mask_case(dtype=dtype)
    c["coefs"] = c["coefs"][:n_levels]
    A = sum(t.shape[1] * t.shape[2] for t in c["coefs"])
    c["assign"] = c["assign"][:, :A].clone()
    return c


def stride_case(dtype=torch.float32):
    """nm 128 on ZERO_PASS_LEVELS (A = 4164), mask 8 x 8, with the smallest b at which b A (nm / vec) is past ZERO_PASS_ITEMS: 4 in f32
    (16656 x 32), 8 in bf16 (33312 x 16).  Six foreground anchors per image: the first two, the last of level 0, the first of levels 1
    and 2 and the very last - of the batch, in the first and the last image."""
    b = 8 if dtype == torch.bfloat16 else 4
    c = _scene("stride", b, 8, 8, 128, ZERO_PASS_LEVELS, 2, dtype)
    for i in range(b):
        _paint(c, i, [(3.0, 2.0, 27.0, 22.0), (9.0, 5.0, 40.0, 30.5)])
        for j, a in enumerate((0, 1, 4095, 4096, 4160, 4163)):
            c["assign"][i, a] = (i + j) % 2
    return c


def _mask_unit(v, size, msize, reciprocal=False):
    """float32 (v / size) * msize as `mask_boxes` (and the kernel) computes it - or, reciprocal, with the divide replaced by a multiply
    with float32(1 / size)."""
    import numpy as np
    v, s, m = np.float32(v), np.float32(size), np.float32(msize)
    return (v * (np.float32(1.0) / s) if reciprocal else v / s) * m


def _edge_kind(v, size, msize):
    """The mask-unit value of v against the nearest integer k: (k, -1 | 0 | +1) for the float32 just below k, k itself, just above k;
    None for anything else."""
    import numpy as np
    r = _mask_unit(v, size, msize)
    k = np.float32(np.rint(r))
    for kind, want in ((0, k), (-1, np.nextafter(k, np.float32(-np.inf))), (1, np.nextafter(k, np.float32(np.inf)))):
        if r == want:
            return int(k), kind
    return None


def edge_values(size, msize, per_kind=2):
    """Pixel-unit float32 values v, searched within 6 float32 steps of k size / msize for k = 1 .. msize - 1, whose mask-unit value is
    exactly an integer (kind 0), the float32 just below one (-1) or just above one (+1): {kind: [(v, k, flips)]}.  Pixel k passes
    k >= x1 iff x1 <= k and passes k < x2 iff x2 > k: for either edge the decision is whether the value is above k.  `flips` says that
    the reciprocal-multiply form of the rule decides that the other way - those values come first."""
    import numpy as np
    found = {-1: [], 0: [], 1: []}
    for k in range(1, msize):
        v0 = np.float32(k * size / msize)
        cands = [v0]
        lo = hi = v0
        for _ in range(6):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
            cands += [lo, hi]
        for v in cands:
            got = _edge_kind(v, size, msize)
            if got is None or got[0] != k:
                continue
            flips = bool((_mask_unit(v, size, msize, reciprocal=True) > k) != (got[1] > 0))
            found[got[1]].append((float(v), k, flips))
    out = {}
    for kind, rows in found.items():
        rows.sort(key=lambda t: (not t[2], abs(t[1] - msize // 2)))
        picked, seen = [], set()
        for row in rows:
            if row[1] not in seen:
                picked.append(row)
                seen.add(row[1])
        out[kind] = picked[:per_kind]
    return out


EDGE_IMGSZ, EDGE_MASK = (96, 80), (24, 20)   # (h, w): 96 / 24 = 80 / 20 = 4, but v / 96 and v / 80 are inexact in float32


def edges_case(dtype=torch.float32):
    """b = 1, mask 24 x 20 of a 96 x 80 image (neither size a power of two times its mask size: the quotient gt / imgsz is inexact),
    default small levels, nm 32.  For each of x1, y1, x2, y2 and each of the three kinds of `edge_values` two boxes with that edge on
    the searched value and ordinary other edges (24 boxes), then a box wholly left of and above the mask and one wholly past its right
    and bottom edges (exactly-zero terms): G = 26, box g on anchor g.  Asserts that the search found every kind for every edge;
    the case's "edge_rows" lists what it placed: [(g, edge 0..3, kind, k, flips)] (the references ignore the key)."""
    ih, iw = EDGE_IMGSZ
    mh, mw = EDGE_MASK
    c = _scene("edges", 1, mh, mw, 32, ((4, 5), (2, 3), (1, 2)), 26, dtype)
    c["imgsz_h"], c["imgsz_w"] = ih, iw
    fx, fy = edge_values(iw, mw), edge_values(ih, mh)
    boxes, rows = [], []
    for e in range(4):
        found = fx if e % 2 == 0 else fy
        size, msize = (iw, mw) if e % 2 == 0 else (ih, mh)
        for kind in (0, -1, 1):
            assert len(found[kind]) == 2, f"edge {e}: kind {kind} not found twice for {size} -> {msize}"
            for v, k, flips in found[kind]:
                # the ordinary edges: between pixel centres, the box at least two mask pixels wide
                bx = [9.5, 10.5, iw - 9.5, ih - 10.5]
                bx[e] = v
                if e < 2 and k > msize - 4:
                    bx[e + 2] = float(size + 6)
                if e >= 2 and k < 4:
                    bx[e - 2] = -6.5
                rows.append((len(boxes), e, kind, k, flips))
                boxes.append(tuple(bx))
    boxes.append((-30.0, -20.0, -5.0, -3.0))
    boxes.append((iw + 5.0, ih + 4.0, iw + 40.0, ih + 34.0))
    _paint(c, 0, boxes)
    c["assign"][0, :26] = torch.arange(26, dtype=torch.int32)
    c["edge_rows"] = rows
    return c


def crop_decisions(gt_boxes, imgsz_h, imgsz_w, mh, mw, reciprocal=False):
    """numpy float32 emulation of the kernel's crop rule on (G, 4) pixel boxes: (G, mh, mw) bool.  reciprocal: the perturbed rule."""
    import numpy as np
    g = gt_boxes.numpy().astype(np.float32)
    size = np.array([imgsz_w, imgsz_h, imgsz_w, imgsz_h], dtype=np.float32)
    nb = g * (np.float32(1.0) / size) if reciprocal else g / size
    mb = nb * np.array([mw, mh, mw, mh], dtype=np.float32)
    xs, ys = np.arange(mw, dtype=np.float32)[None, None, :], np.arange(mh, dtype=np.float32)[None, :, None]
    x1, y1, x2, y2 = (mb[:, k, None, None] for k in range(4))
    return (xs >= x1) & (xs < x2) & (ys >= y1) & (ys < y2)


FAMILIES = {  # name: builder(dtype)
    "turns": turns_case,
    "turns_permuted": (lambda dtype=torch.float32: turns_case(dtype, permute=1)),
    "clamp": clamp_case,
    "clamp_permuted": (lambda dtype=torch.float32: clamp_case(dtype, permute=5)),
    "levels1": (lambda dtype=torch.float32: levels_case(1, dtype)),
    "levels2": (lambda dtype=torch.float32: levels_case(2, dtype)),
    "stride": stride_case,
    "edges": edges_case,
}
FAMILIES.update({f"depth{nm}": (lambda dtype=torch.float32, nm=nm: mask_case(nm=nm, dtype=dtype)) for nm in sorted(set(sum(DEPTHS.values(), ())))})


def family_names(dtype):
    """The families that exist in `dtype` (a depth must be a multiple of 16 bytes)."""
    return [n for n in FAMILIES if not n.startswith("depth") or int(n[5:]) in DEPTHS[dtype]]


_CASE, _REF = {}, {}


def family(name, dtype=torch.float32):
    """The case of a family, built once per process; treat it as read-only."""
    if (name, dtype) not in _CASE:
        _CASE[name, dtype] = FAMILIES[name](dtype)
    return _CASE[name, dtype]


def reference(name, dtype=torch.float32):
    """mask_loss_ref of a family, computed once per process and left unchanged (the all-foreground images cost seconds)."""
    if (name, dtype) not in _REF:
        _REF[name, dtype] = mask_loss_ref(**family(name, dtype))
    return _REF[name, dtype]
