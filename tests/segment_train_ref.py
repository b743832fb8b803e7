"""float64 references of the two segmentation-training entries (test infrastructure): the gradients of ConvTranspose2d(2, 2, 0) and the
mask term of v8SegmentationLoss (utils/loss.py:622-709, crop_mask's comparison branch utils/ops.py:510-513) with its gradients, each
with the operand-magnitude sums the kernel tests build their bounds from (tests/kernel_check.py: K u S + u |ref|).  Written out by hand
- no autograd - so that tests/test_segment_train_ref.py can hold them to torch autograd of the reference formula."""

import torch
import torch.nn.functional as F


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


def mask_loss_ref(proto, coefs, assign, gt, n_gt, mask_id, masks, imgsz_h, imgsz_w, gain, scale, u_in=2.0 ** -24):
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


def mask_loss_autograd(proto, coefs, assign, gt, n_gt, mask_id, masks, imgsz_h, imgsz_w, gain, scale):
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
