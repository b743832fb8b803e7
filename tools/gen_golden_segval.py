"""Generate the segmentation-validation fixtures under tests/golden/ by running the IMPORTED REFERENCE (via oracle/ref_shim.py, as
tools/gen_golden_segment.py does) on procedural inputs, and cross-check the integer CPU checker tests/segval_ref.py against it.

Run on a machine that has the reference checkout:   python -m tools.gen_golden_segval [ops] [map]
Outputs (data only):
  tests/golden/ops_segval.npz          small mask sets: packed predicted and label masks, classes, the reference's `mask_iou`
                                       (utils/metrics.py:146-161) and `match_predictions` (engine/validator.py:267-308) outputs
  tests/golden/map_yolov8n-seg.npz     the synthetic mask-mAP set: yolov8n-seg on procedural weights and images -> val-mode NMS ->
                                       process_mask at 160 x 160 -> labels cut from the model's own masks -> box and mask TP matrices,
                                       mask IoU matrices, ap_per_class tables and means (models/yolo/segment/val.py:94-172)
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
GOLD = ROOT / "tests" / "golden"

from oracle.ref_shim import import_reference  # noqa: E402
from tests import segment_oracle as S  # noqa: E402
from tests import segval_ref as V  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

# name, predictions N, labels M, map (h, w): the shapes tests/test_hip_segval.py runs (N in {0, 1, 37, 300}, M in {0, 1, 5, 64, 70})
OPS_CASES = [("n0_m5", 0, 5, (20, 28)), ("n1_m1", 1, 1, (8, 8)), ("n37_m5", 37, 5, (20, 28)), ("n37_m70", 37, 70, (20, 28)),
             ("n300_m64", 300, 64, (40, 40)), ("n5_m0", 5, 0, (8, 8)), ("n300_m1", 300, 1, (20, 28))]
PRED_BITS_LIMIT = 1 << 20  # no committed file above 1 MiB


class _V:  # match_predictions only needs self.iouv (detect/val.py:59)
    iouv = torch.linspace(0.5, 0.95, 10)


def _blob(u, hw):
    """A filled ellipse from 4 hash values: centre anywhere, radii 2 px .. a third of the map."""
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = u[0] * h, u[1] * w
    ry, rx = 2.0 + u[2] * h / 3, 2.0 + u[3] * w / 3
    return ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0


def _shift(m, dy, dx):
    """m moved by (dy, dx) pixels, zero filled."""
    out = np.zeros_like(m)
    h, w = m.shape
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[yd, xd] = m[ys, xs]
    return out


def _dilate(m):
    out = m.copy()
    for dy, dx in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        out |= _shift(m, dy, dx)
    return out


def ops_case_inputs(name, n, m, hw):
    """Label masks: ellipses; predicted masks: a label's ellipse moved by 0-3 px with hash-flipped pixels (IoU spread over (0, 1]), or
    an unrelated ellipse.  Classes 0-2, plus class 7 on labels only and class 9 on predictions only."""
    h, w = hw
    ug = P.hash_uniform(f"segval:{name}:gt", 8 * max(m, 1)).reshape(-1, 8)
    up = P.hash_uniform(f"segval:{name}:pred", 8 * max(n, 1)).reshape(-1, 8)
    gt = np.stack([_blob(ug[k, :4], hw) for k in range(m)]) if m else np.zeros((0, h, w), bool)
    gcls = np.array([7.0 if ug[k, 4] < 0.1 else float(int(ug[k, 4] * 3) % 3) for k in range(m)], np.float32)
    pred, pcls = [], []
    for i in range(n):
        if m and up[i, 0] < 0.8:
            k = int(up[i, 1] * m) % m
            base = _shift(gt[k], int(up[i, 2] * 4) - 1, int(up[i, 3] * 4) - 1)
            flip = P.hash_uniform(f"segval:{name}:flip:{i}", h * w).reshape(h, w) < 0.04 * up[i, 4]
            pred.append(base ^ flip)
            pcls.append(gcls[k] if up[i, 5] > 0.2 else float((int(gcls[k]) + 1) % 3))
        else:
            pred.append(_blob(up[i, 4:8], hw))
            pcls.append(9.0 if up[i, 1] < 0.3 else float(int(up[i, 2] * 3) % 3))
    pred = np.stack(pred) if n else np.zeros((0, h, w), bool)
    if n > 2:
        pred[2] = False  # an empty prediction
    return pred, np.array(pcls, np.float32), gt, gcls


def assert_no_decisive_tie(iou, pcls, gcls, what, strict):
    """The reference sorts the candidate pairs with an unstable sort, so equal IoUs leave its answer undefined.  `strict`: no two
    same-class candidate pairs (IoU >= 0.5) of the image are equal.  Otherwise: no DETECTION has two equal best candidates - the
    only place the order among equal keys can reach the result (labels take their smallest detection index, not the first in sort order)."""
    c = (iou * (gcls[:, None] == pcls[None])).astype(np.float32)
    if strict:
        v = c[c >= 0.5]
        assert len(np.unique(v)) == len(v), f"{what}: {len(v) - len(np.unique(v))} exactly equal candidate IoUs"
    else:
        for j in range(c.shape[1]):
            v = c[:, j][c[:, j] >= 0.5]
            assert len(v) < 2 or np.sort(v)[-1] != np.sort(v)[-2], f"{what}: detection {j} has two equal best labels"


def ref_mask_stats(rmet, BaseValidator, pred, pcls, gt, gcls):
    """The reference's own calls of SegmentationValidator._process_batch (val.py:165-170) -> (IoU (M, N) f32, TP (N, 10) bool)."""
    n, m = len(pcls), len(gcls)
    if n == 0 or m == 0:
        return np.zeros((m, n), np.float32), np.zeros((n, 10), bool)
    iou = rmet.mask_iou(torch.from_numpy(gt.reshape(m, -1)).float(), torch.from_numpy(pred.reshape(n, -1).astype(np.uint8)).float())
    tp = BaseValidator.match_predictions(_V, torch.from_numpy(pcls), torch.from_numpy(gcls), iou).numpy()
    return iou.numpy(), tp


def ops(rt):
    from ultralytics.engine.validator import BaseValidator
    from ultralytics.utils import metrics as rmet
    G = {"cases": np.array([c[0] for c in OPS_CASES])}
    for name, n, m, hw in OPS_CASES:
        pred, pcls, gt, gcls = ops_case_inputs(name, n, m, hw)
        iou, tp = ref_mask_stats(rmet, BaseValidator, pred, pcls, gt, gcls)
        assert_no_decisive_tie(iou, pcls, gcls, name, strict=False)
        iou_c, tp_c = V.process_batch_masks(pred, pcls, gt, gcls)
        assert np.array_equal(iou, iou_c) and np.array_equal(tp, tp_c), f"{name}: tests/segval_ref.py != reference"
        assert np.array_equal(V.unpack_bits(V.pack_bits(pred), hw[0] * hw[1]).reshape(pred.shape), pred)
        G[f"{name}_hw"] = np.array(hw)
        G[f"{name}_pred_bits"], G[f"{name}_pred_cls"] = V.pack_bits(pred), pcls
        G[f"{name}_gt_bits"], G[f"{name}_gt_cls"] = V.pack_bits(gt), gcls
        G[f"{name}_iou"], G[f"{name}_tp"] = iou, tp
        print(f"ops {name}: {n} x {m} on {hw}: TP@0.5 {int(tp[:, 0].sum())} TP@0.95 {int(tp[:, 9].sum())}, "
              f"IoU >= 0.5 pairs {int((iou >= 0.5).sum())}")
    np.savez_compressed(GOLD / "ops_segval.npz", **G)


def _tied_labels(miou, pcls, gcls):
    """Labels that take part in two exactly equal same-class candidate pairs (IoU >= 0.5), the lowest label of each group left out
    when the group spans several labels."""
    c = (miou * (gcls[:, None] == pcls[None])).astype(np.float32)
    vals, cnt = np.unique(c[c >= 0.5], return_counts=True)
    bad = set()
    for v in vals[cnt > 1]:
        ls = sorted(set(np.nonzero(c == v)[0].tolist()))
        bad.update(ls[1:] if len(ls) > 1 else ls)
    return sorted(bad)


def synthetic_mask_labels(det, masks, image_index, mask_iou_fn, rounds=12):
    """Labels of the synthetic mask-mAP set, in the style of oracle/gen_golden.py's synthetic_ground_truth: every third of the first 90
    detections whose mask has >= 16 pixels; the box jittered as there; the mask moved by a hash-driven 0-6 px and, for a third of
    the labels, dilated by one pixel; 15 % wrong classes.  The reference's unstable sort leaves exactly equal candidate IoUs
    undefined (an unmoved, undilated label has IoU 1.0 with its source, so would every second one): a label whose candidates tie is
    drawn again from the next hash stream, and dropped if `rounds` draws do not separate it (two detections with the same mask)."""
    n = det.shape[0]
    streams = {}

    def draw(i, attempt):
        if attempt not in streams:
            key = f"segmap:gt:{image_index}" + (f":{attempt}" if attempt else "")
            streams[attempt] = P.hash_uniform(key, 12 * max(n, 1)).reshape(-1, 12)
        u = streams[attempt]
        b = det[i, :4].clone()
        w, h = (b[2] - b[0]).clamp(min=1.0), (b[3] - b[1]).clamp(min=1.0)
        jit = torch.from_numpy(u[i, :4].copy()) - 0.5
        scale = 0.02 + 0.5 * float(u[i, 4]) ** 2
        box = b + jit * scale * torch.stack([w, h, w, h])
        c = det[i, 5] if u[i, 5] > 0.15 else (det[i, 5] + 1) % 80
        s = int(7 * float(u[i, 6]) ** 2)  # 0 .. 6 px, most of them small
        ang = 2 * np.pi * float(u[i, 7])
        m = _shift(masks[i], int(round(s * np.sin(ang))), int(round(s * np.cos(ang))))
        return box, c, (_dilate(m) if u[i, 8] < 1 / 3 else m)

    src = [i for i in range(0, min(n, 90), 3) if int(masks[i].sum()) >= 16]
    lab = [draw(i, 0) for i in src]
    pcls = det[:, 5].numpy()
    for attempt in range(1, rounds + 1):
        if not lab:
            break
        gcls = torch.stack([c for _, c, _ in lab]).numpy().astype(np.float32)
        bad = _tied_labels(mask_iou_fn(np.stack([m for _, _, m in lab])), pcls, gcls)
        if not bad:
            break
        if attempt == rounds:
            src, lab = [v for k, v in enumerate(src) if k not in bad], [v for k, v in enumerate(lab) if k not in bad]
            break
        for k in bad:
            lab[k] = draw(src[k], attempt)
    if not lab:
        return torch.zeros((0, 4)), torch.zeros((0,)), np.zeros((0,) + masks.shape[1:], bool)
    return torch.stack([b for b, _, _ in lab]), torch.stack([c for _, c, _ in lab]), np.stack([m for _, _, m in lab])


def map_golden(rt):
    import ultralytics.utils.ops as rops
    from ultralytics.engine.validator import BaseValidator
    from ultralytics.utils import metrics as rmet
    from ultralytics.utils.nms import non_max_suppression as r_nms

    from tools.gen_golden_segment import _ref_model
    from ultralytics_pro_amd.utils import metrics as pmet

    name = "yolov8n-seg"
    ref = _ref_model(rt, name)
    P.apply_procedural_weights(ref, family=name)
    ref.eval().fuse(verbose=False)
    x = P.synthetic_images(4)
    yr, (_, _, pr) = ref(x)
    dets = r_nms(yr.clone(), conf_thres=0.001, iou_thres=0.7, nc=80, max_det=300, multi_label=True, max_time_img=1e9)
    G, near = {}, 0
    acc = {k: [] for k in ("tp", "tp_m", "conf", "pcls", "tcls")}
    for i, d in enumerate(dets):
        n = d.shape[0]
        # the validator's default mask path (segment/val.py:109: process_mask, upsample = False): (n, 160, 160) at proto resolution
        pm = rops.process_mask(pr[i], d[:, 6:], d[:, :4].clone(), (640, 640), upsample=False)
        # the product runs crop_mask's comparison form, the branch the reference takes from 50 masks on; the fixture pins that one
        assert n >= 50 and torch.equal(pm, S.process_mask(pr[i], d[:, 6:], d[:, :4].clone(), (640, 640), branch="compare")), \
            f"image {i}: {n} detections - the reference's CPU call took the rounded-loop crop"
        pm = pm.numpy().astype(bool)
        gb, gc, gm = synthetic_mask_labels(d, pm, i, lambda g: V.mask_iou(g, pm))
        pcls, gcls = d[:, 5].numpy(), gc.numpy().astype(np.float32)
        tp = BaseValidator.match_predictions(_V, d[:, 5], gc, rmet.box_iou(gb, d[:, :4])).numpy()
        miou, tp_m = ref_mask_stats(rmet, BaseValidator, pm, pcls, gm, gcls)
        assert_no_decisive_tie(miou, pcls, gcls, f"image {i}", strict=True)
        iou_c, tp_c = V.process_batch_masks(pm, pcls, gm, gcls)
        assert np.array_equal(miou, iou_c) and np.array_equal(tp_m, tp_c), f"image {i}: tests/segval_ref.py != reference"
        cand = (miou * (gcls[:, None] == pcls[None]))[:, :, None]
        near += int((np.abs(cand - V.IOUV[None, None]) <= 1e-3).sum())
        G[f"det{i}"], G[f"gt_boxes{i}"], G[f"gt_cls{i}"], G[f"gt_bits{i}"] = d.numpy(), gb.numpy(), gcls, V.pack_bits(gm)
        G[f"tp{i}"], G[f"tp_m{i}"], G[f"mask_iou{i}"] = tp, tp_m, miou
        if i == 0:
            G["pred_bits0"] = V.pack_bits(pm)
        for k, v in zip(acc, (tp, tp_m, d[:, 4].numpy(), pcls, gcls)):
            acc[k].append(v)
        print(f"map image {i}: {n} detections, {len(gcls)} labels, box TP@0.5 {int(tp[:, 0].sum())}, mask TP@0.5 {int(tp_m[:, 0].sum())} "
              f"@0.95 {int(tp_m[:, 9].sum())}")
    tp, tp_m, conf, pc, tc = (np.concatenate(acc[k], 0) for k in ("tp", "tp_m", "conf", "pcls", "tcls"))
    for tag, t in (("", tp), ("seg_", tp_m)):
        res = rmet.ap_per_class(t, conf, pc, tc)
        p_, r_, f1_, ap_, uc_ = res[2], res[3], res[4], res[5], res[6]
        po, ro, fo, apo, uco = pmet.ap_per_class(t, conf, pc, tc)  # the product's host AP arithmetic
        assert np.array_equal(ap_, apo) and np.array_equal(p_, po) and np.array_equal(r_, ro) and np.array_equal(uc_, uco)
        G.update({tag + "p": p_, tag + "r": r_, tag + "f1": f1_, tag + "ap": ap_, tag + "classes": uc_,
                  tag + "mean": np.array([p_.mean(), r_.mean(), ap_[:, 0].mean(), ap_.mean()])})
    # the fixture must not be vacuous
    assert int(tp_m[:, 0].sum()) > int(tp_m[:, 9].sum()) > 0, (int(tp_m[:, 0].sum()), int(tp_m[:, 9].sum()))
    assert 0.05 < G["seg_mean"][3] < 0.95 and G["seg_mean"][3] != G["mean"][3], (G["seg_mean"], G["mean"])
    G["near_threshold"] = np.array(near)
    print(f"map {name}: box {G['mean']}, mask {G['seg_mean']}, near_threshold {near}")
    out = GOLD / f"map_{name}.npz"
    np.savez_compressed(out, **G)
    if out.stat().st_size > PRED_BITS_LIMIT:  # image 0's masks push the file past the limit: its first 120
        G["pred_bits0"] = G["pred_bits0"][:120]
        np.savez_compressed(out, **G)
    assert out.stat().st_size <= PRED_BITS_LIMIT, out.stat().st_size
    print(f"   {out.name}: {out.stat().st_size} bytes, pred_bits0 {G['pred_bits0'].shape}")


def main():
    torch.manual_seed(0)
    rt = import_reference()
    which = sys.argv[1:] or ["ops", "map"]
    with torch.no_grad():
        if "ops" in which:
            ops(rt)
        if "map" in which:
            map_golden(rt)


if __name__ == "__main__":
    main()
