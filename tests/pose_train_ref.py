"""Float64 references of the pose-training kernel (tests/test_hip_pose_train.py, tests/test_pose_train_ref.py): the keypoint terms of
v8PoseLoss with their gradients and the float32 evaluation-error bounds of both, an autograd restatement of the reference's own
formulas, and the case builders.  CPU only."""

import torch
import torch.nn.functional as F

from tests.kernel_check import ZERO_PASS_ITEMS, ZERO_PASS_LEVELS
from tests.kernel_check import zero_pass_items as _zero_pass_items
from tests.loss_ref import HW, STRIDES

U32 = 2.0 ** -24
TINY32 = 2.0 ** -149  # the spacing of float32's subnormals: what a rounding costs where u |x| is less


REFUSALS = ("null pointer", "a keypoint is (x, y)", "keypoint values per anchor, at most", "outside f32 | bf16", "channels hold no",
            "16 bytes at a time", "stride / address must be multiples of 16 bytes", "workspace too small")


def refusals_precede_launches():
    """True when, in the source of upa_kpt_loss, every refusal stands before the first launch.  The GPU refusal test asks this before
    it hands the kernel arguments a build without the checks would read or write out of range with."""
    from pathlib import Path
    src = (Path(__file__).resolve().parent.parent / "ultralytics_pro_amd" / "csrc" / "pose_train.hip").read_text()
    body = src[src.rindex('extern "C" int upa_kpt_loss'):]
    first = body.index("hipLaunchKernelGGL")
    return all(0 <= body.find(k) < first for k in REFUSALS)


def _fg(assign, n_gt):
    b, A = assign.shape
    return [(i, a, int(assign[i, a])) for i in range(b) for a in range(A) if 0 <= int(assign[i, a]) < int(n_gt[i])]


def _cells(hw):
    """(A, 3): cell x, cell y, level of every anchor, level by level, row-major."""
    out = []
    for l, (h, w) in enumerate(hw):
        for y in range(h):
            for x in range(w):
                out.append((x, y, l))
    return out


def kpt_loss_ref(kpts, assign, gt, n_gt, gt_kpt, strides, sigma, kpt_shape, gain_pose, gain_kobj, scale, u=U32, **_):
    """kpts: per level (b, h, w, c) with the nk = nkpt * ndim values of an anchor in front; assign (b, A) gt row or -1 (rows >= n_gt:
    background); gt (b, G, 5) pixel xyxy behind the class; gt_kpt (b, G, nkpt, 3) pixels; sigma (nkpt,) as the kernel gets it (f32).
    Everything in float64.  Returns dict(items (2,), items_err (2,), dkpts / dkpts_err per level (b, h, w, c), n_fg): the gradients are
    those of (pose + kobj) * b * scale and the *_err are bounds of a float32 evaluation's error, without the output's rounding.
    Error model (u = 2^-24).  px = 2 v + cell and the difference px - gx are one rounding each (2 v and kpt / stride, a power of two,
    are exact): |d(px - gx)| <= u (|px| + |px - gx|).  d, the area (three roundings), the denominator (three more) and the division
    give e a relative error of 10 u on top of what the differences carry.  expf, log1pf and the sigmoid's division are taken at 2 u of
    their result; a K-term sum in a fixed order at K u of the sum of magnitudes; a product of n factors at n u.  Far from its keypoint
    exp(-e) is a float32 subnormal (or underflows to 0) and every rounding costs up to TINY32 whatever the magnitude: exp(-e) and the
    gradient built on it carry 4 TINY32 each on top, the former scaled by the coefficient it is multiplied with (the kernel forms that
    coefficient first, in the normal range, so no subnormal intermediate is scaled up again)."""
    nkpt, ndim = kpt_shape
    nk = nkpt * ndim
    b = assign.shape[0]
    hw = [tuple(t.shape[1:3]) for t in kpts]
    cells = _cells(hw)
    a0 = [0]
    for h, w in hw:
        a0.append(a0[-1] + h * w)
    fg = _fg(assign, n_gt)
    n = len(fg)
    sg = torch.as_tensor(sigma, dtype=torch.float32).double()
    dk = [torch.zeros(t.shape, dtype=torch.float64) for t in kpts]
    ek = [torch.zeros(t.shape, dtype=torch.float64) for t in kpts]
    pose = kobj = pose_err = kobj_err = 0.0
    for i, a, g in fg:
        x, y, l = cells[a]
        s = float(strides[l])
        v = kpts[l][i, y, x, :nk].double().view(nkpt, ndim)
        box = gt[i, g, 1:5].double() / s
        area = (box[2] - box[0]) * (box[3] - box[1])
        gk = gt_kpt[i, g].double()
        m = (gk[:, 2] != 0).double() if ndim == 3 else torch.ones(nkpt, dtype=torch.float64)
        px, py = 2 * v[:, 0] + x, 2 * v[:, 1] + y
        dx, dy = px - gk[:, 0] / s, py - gk[:, 1] / s
        ddx, ddy = u * (px.abs() + dx.abs()), u * (py.abs() + dy.abs())
        denom = (2 * sg) ** 2 * (area + 1e-9) * 2
        e = (dx * dx + dy * dy) / denom
        de = (2 * dx.abs() * ddx + 2 * dy.abs() * ddy) / denom + 10 * u * e
        ex = torch.exp(-e)
        dex = ex * (de + 2 * u) + 4 * TINY32
        factor = nkpt / (m.sum() + 1e-9)
        tp = (1 - ex) * m
        pose += float(factor * tp.sum())
        pose_err += float(factor * ((dex + u) * m).sum() + (nkpt + 4) * u * factor * tp.sum())
        kp = gain_pose * b * scale / (n * nkpt)
        kfac = kp * factor * m * ex * 4 / denom
        dk[l][i, y, x, 0:nk:ndim] = kfac * dx
        dk[l][i, y, x, 1:nk:ndim] = kfac * dy
        # subnormals: exp(-e)'s 4 TINY32 through the coefficient it meets, the product's own rounding through the difference, the result's
        floor = (kp * factor * 4 / denom * 4 + 2) * TINY32 * m
        ek[l][i, y, x, 0:nk:ndim] = kfac * (dx.abs() * (de + 16 * u) + ddx) + floor * dx.abs() + 4 * TINY32 * m
        ek[l][i, y, x, 1:nk:ndim] = kfac * (dy.abs() * (de + 16 * u) + ddy) + floor * dy.abs() + 4 * TINY32 * m
        if ndim == 3:
            bce = F.binary_cross_entropy_with_logits(v[:, 2], m, reduction="none")
            kobj += float(bce.sum())
            kobj_err += float((8 * u * (bce + 1)).sum() + (nkpt + 4) * u * bce.sum())
            kk = gain_kobj * b * scale / (n * nkpt)
            dv = torch.sigmoid(v[:, 2]) - m
            dk[l][i, y, x, 2:nk:ndim] = kk * dv
            ek[l][i, y, x, 2:nk:ndim] = kk * (4 * u + 6 * u * dv.abs())
    items, errs = [0.0, 0.0], [0.0, 0.0]
    if n:
        items = [gain_pose * pose / (n * nkpt), gain_kobj * kobj / (n * nkpt) if ndim == 3 else 0.0]
        errs = [gain_pose * pose_err / (n * nkpt) + 4 * u * items[0], (gain_kobj * kobj_err / (n * nkpt) + 4 * u * items[1]) if ndim == 3 else 0.0]
    return dict(items=torch.tensor(items, dtype=torch.float64), items_err=torch.tensor(errs, dtype=torch.float64), dkpts=dk, dkpts_err=ek,
                n_fg=n)


def kpt_loss_autograd(kpts, assign, gt, n_gt, gt_kpt, strides, sigma, kpt_shape, gain_pose, gain_kobj, scale, **_):
    """loss.py:396-412 (KeypointLoss.forward), :791-798 (kpts_decode) and :829-870 (calculate_keypoints_loss) restated on the packed
    rows, under float64 autograd: (items (2,), dkpts per level) for gradients of (pose + kobj) * b * scale."""
    nkpt, ndim = kpt_shape
    nk = nkpt * ndim
    b = assign.shape[0]
    ks = [t.double().clone().requires_grad_(True) for t in kpts]
    hw = [tuple(t.shape[1:3]) for t in kpts]
    pred = torch.cat([t[..., :nk].reshape(b, -1, nk) for t in ks], 1).view(b, -1, nkpt, ndim)
    cells = torch.tensor(_cells(hw), dtype=torch.float64)
    anchor_points = cells[:, :2] + 0.5                                     # make_anchors(feats, stride, 0.5)
    stride_tensor = torch.tensor([float(strides[int(l)]) for l in cells[:, 2]], dtype=torch.float64).view(-1, 1)
    y = pred.clone()                                                       # kpts_decode
    y[..., :2] = y[..., :2] * 2.0
    y[..., 0] = y[..., 0] + (anchor_points[:, [0]] - 0.5)
    y[..., 1] = y[..., 1] + (anchor_points[:, [1]] - 0.5)
    masks = (assign >= 0) & (assign < n_gt.view(-1, 1))
    if not bool(masks.any()):
        return torch.zeros(2, dtype=torch.float64), [torch.zeros_like(t) for t in ks]
    idx = assign.clamp(min=0).long()
    target_bboxes = torch.gather(gt[..., 1:5].double(), 1, idx.unsqueeze(-1).expand(-1, -1, 4)) / stride_tensor.view(1, -1, 1)
    selected = torch.gather(gt_kpt.double(), 1, idx.view(b, -1, 1, 1).expand(-1, -1, nkpt, 3)).clone()
    selected[..., :2] = selected[..., :2] / stride_tensor.view(1, -1, 1, 1)
    gt_k = selected[masks]
    tb = target_bboxes[masks]
    area = ((tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])).view(-1, 1)     # xyxy2xywh(...)[:, 2:].prod(1, keepdim=True)
    pred_kpt = y[masks]
    kpt_mask = (gt_k[..., 2] != 0) if ndim == 3 else torch.full_like(gt_k[..., 0], True)
    sig = torch.as_tensor(sigma, dtype=torch.float32).double()
    d = (pred_kpt[..., 0] - gt_k[..., 0]).pow(2) + (pred_kpt[..., 1] - gt_k[..., 1]).pow(2)
    # (.double(): an integer sum + 1e-9 is promoted to the DEFAULT dtype, float32, where the 1e-9 vanishes)
    factor = kpt_mask.shape[1] / (torch.sum(kpt_mask != 0, dim=1).double() + 1e-9)
    e = d / ((2 * sig).pow(2) * (area + 1e-9) * 2)
    pose = (factor.view(-1, 1) * ((1 - torch.exp(-e)) * kpt_mask)).mean() * gain_pose
    kobj = torch.zeros((), dtype=torch.float64)
    if ndim == 3:
        kobj = F.binary_cross_entropy_with_logits(pred_kpt[..., 2], kpt_mask.double()) * gain_kobj
    ((pose + kobj) * b * scale).backward()
    return torch.stack([pose.detach(), kobj.detach()]), [t.grad for t in ks]


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
_BOXES = [  # pixel xyxy of a 160 x 96 image
    [(9.0, 6.0, 70.0, 57.0), (41.0, 18.0, 150.0, 90.0), (100.5, 10.0, 143.5, 50.0), (20.0, 40.0, 60.0, 80.0)],
    [(5.0, 5.0, 60.0, 60.0), (70.0, 10.0, 150.0, 80.0)],
    [(8.0, 8.0, 120.0, 88.0)],
]
CASES = {  # name: (kpt_shape, c, variant)
    "coco17": ((17, 3), 56, "base"),
    "five2d": ((5, 2), 16, "base"),
    "one3d": ((1, 3), 8, "base"),
    "all_fg": ((17, 3), 56, "all"),
    "none_fg": ((17, 3), 56, "none"),
    "all_wide": ((17, 3), 56, "all"),
    "stride": ((17, 3), 56, "stride"),
}
# Cases off the default geometry.  "all_wide": the anchor kernel launches min((min(10 G, A) + 3) / 4, 128) workgroups per image, so the
# clamp needs 10 G >= 510 AND A >= 510 - on the default levels (A = 315) G = 60 gives 79 workgroups and no clamp; these levels have
# A = 630: 150 clamped to 128, and the 158 four-slot groups of an all-foreground image give workgroups 0..29 a second turn.
# "stride": c = 56 on tests/kernel_check's ZERO_PASS_LEVELS with the smallest b at which b A (c / vec) is past the zero pass's
# ZERO_PASS_ITEMS: 9 images in f32 (37476 x 14), 18 in bf16 (74952 x 7).
WIDE_HW = ((20, 24), (10, 12), (5, 6))


def geometry(name, dtype=torch.float32):
    """(b, G, hw) of a case."""
    if name == "all_wide":
        return 3, 60, WIDE_HW
    if name == "stride":
        return (18 if dtype == torch.bfloat16 else 9), 6, ZERO_PASS_LEVELS
    return 3, 6, HW


def anchor_groups(case):
    """(workgroups per image that upa_kpt_loss launches, the count before the clamp to 128)."""
    A, G = case["assign"].shape[1], case["gt"].shape[1]
    want = (min(10 * G, A) + 3) // 4
    return min(want, 128), want


def zero_pass_items(case, dtype):
    return _zero_pass_items(case["assign"].numel(), case["c"], dtype)


def kpt_case(name, dtype=torch.float32, hw=None, strides=STRIDES, b=None, G=None):
    """The kernel test's inputs (values representable in `dtype`); b, G and the levels default to `geometry(name, dtype)`: b = 3, G = 6
    on tests/loss_ref's default levels (A = 315, past one 256-thread workgroup) for every case but "all_wide" and "stride".
    variant "base": image 0 - gt 0 on two anchors of level 0 and one of level 1 (the area is taken at two strides), gt 1 on a level-1 anchor (index past 256) and a level-2 anchor, gt 2 with EVERY keypoint invisible, gt 3 unassigned;
    image 1 - an anchor assigned to row 2 >= n_gt = 2 and one to row -5 (background both), one real assignment; image 2 - assignments
    but n_gt = 0.  Keypoints lie around the first anchor of their gt (so 1 - exp(-e) is neither 0 nor 1 there), some outside their box,
    some with visibility 0 or 2.  "all": every anchor foreground; "none": no anchor; "stride": image i has the boxes of image i % 3, the
    first image is foreground at anchors 0, 1 and the last of level 0, the last image at the first anchors of levels 1 and 2 and at the
    very last anchor."""
    from ultralytics_pro_amd.utils import procedural as P
    from ultralytics_pro_amd.utils.metrics import OKS_SIGMA
    kpt_shape, c, variant = CASES[name]
    nkpt, ndim = kpt_shape
    nk = nkpt * ndim
    gb, gG, ghw = geometry(name, dtype)
    b, G, hw = gb if b is None else b, gG if G is None else G, ghw if hw is None else hw

    def rnd(key, shape, lo, hi):
        return P.uniform(f"pose_train:{name}:{key}", shape, lo, hi)
    kpts = [rnd(f"k{l}", (b, h, w, c), -1.5, 1.5).to(dtype).float() for l, (h, w) in enumerate(hw)]
    A = sum(h * w for h, w in hw)
    a1, a2 = hw[0][0] * hw[0][1], hw[0][0] * hw[0][1] + hw[1][0] * hw[1][1]
    gt = torch.zeros(b, G, 5)
    for i in range(b):
        for g, bx in enumerate(_BOXES[i % 3]):
            gt[i, g, 1:] = torch.tensor(bx)
    n_gt = torch.tensor([(4, 2, 0)[i % 3] for i in range(b)], dtype=torch.int32)
    assign = torch.full((b, A), -1, dtype=torch.int32)
    if variant == "base":
        w0, w1, w2 = hw[0][1], hw[1][1], hw[2][1]
        assign[0, 2 * w0 + 3] = 0
        assign[0, 3 * w0 + 4] = 0
        assign[0, a1 + 1 * w1 + 2] = 0      # level 1: the same gt at another stride
        assign[0, a1 + 2 * w1 + 6] = 1      # anchor 266: the second 256-anchor turn of the compaction
        assign[0, a2 + 1 * w2 + 3] = 1      # level 2
        assign[0, 1 * w0 + 15] = 2          # every keypoint invisible
        assign[1, 4 * w0 + 2] = 0
        assign[1, 5 * w0 + 5] = 2           # row 2 >= n_gt[1] = 2: background
        assign[1, 7] = -5
        assign[2, 3] = 0                    # n_gt = 0: background whatever the array says
        assign[2, a2 + 4] = 0
    elif variant == "all":
        n_gt = torch.tensor([(4, 2, 1)[i % 3] for i in range(b)], dtype=torch.int32)
        for i in range(b):
            assign[i] = (torch.arange(A) * 7 + i) % int(n_gt[i])
    elif variant == "stride":
        n_gt = torch.tensor([(4, 2, 1)[i % 3] for i in range(b)], dtype=torch.int32)
        assign[0, 0], assign[0, 1], assign[0, a1 - 1] = 0, 1, 3
        assign[b - 1, a1], assign[b - 1, a2], assign[b - 1, A - 1] = 0, 0, 0
    # keypoints of gt (i, g): around the decoded prediction of the first anchor assigned to it, up to 0.6 cells away
    cells = _cells(hw)
    gt_kpt = torch.zeros(b, G, nkpt, 3)
    noise = rnd("noise", (b, G, nkpt, 2), -0.6, 0.6)
    vis = (rnd("vis", (b, G, nkpt), 0.0, 3.0)).floor().clamp(0, 2)
    for i in range(b):
        for g in range(G):
            x1, y1, x2, y2 = (float(v) for v in gt[i, g, 1:])
            first = (assign[i] == g).nonzero().flatten().tolist()
            if first:
                x, y, l = cells[first[0]]
                v = kpts[l][i, y, x, :nk].view(nkpt, ndim)
                gt_kpt[i, g, :, 0] = (2 * v[:, 0] + x + noise[i, g, :, 0]) * strides[l]
                gt_kpt[i, g, :, 1] = (2 * v[:, 1] + y + noise[i, g, :, 1]) * strides[l]
            else:
                gt_kpt[i, g, :, 0] = x1 + (x2 - x1) * (noise[i, g, :, 0] + 0.5)
                gt_kpt[i, g, :, 1] = y1 + (y2 - y1) * (noise[i, g, :, 1] + 0.5)
            gt_kpt[i, g, :, 2] = vis[i, g]
    gt_kpt[..., :2] = (gt_kpt[..., :2] * 4).round() / 4   # quarter pixels: kpt / stride is exact
    if variant == "base":
        gt_kpt[0, 2, :, 2] = 0.0            # the label without a visible keypoint
        gt_kpt[0, 0, 0, 2] = 0.0            # at least one invisible and one visible keypoint on an ordinary label
        gt_kpt[0, 0, nkpt - 1, 2] = 2.0
    sigma = torch.tensor(OKS_SIGMA, dtype=torch.float32) if kpt_shape == (17, 3) else torch.full((nkpt,), 1.0 / nkpt)
    return dict(kpts=kpts, assign=assign, gt=gt, n_gt=n_gt, gt_kpt=gt_kpt, strides=strides, sigma=sigma, kpt_shape=kpt_shape, c=c,
                gain_pose=12.0, gain_kobj=1.0, scale=1.0)


_REF = {}


def reference(name, dtype=torch.float32, scale=1.0):
    """kpt_loss_ref of a case, computed once per process and left unchanged."""
    key = (name, dtype, scale)
    if key not in _REF:
        _REF[key] = kpt_loss_ref(**dict(kpt_case(name, dtype), scale=scale))
    return _REF[key]
