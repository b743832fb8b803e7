"""Generate the pose fixtures under tests/golden/ by running the IMPORTED REFERENCE (via oracle/ref_shim.py, as
tools/gen_golden_segment.py and tools/gen_golden_segval.py do) on procedural weights and inputs, and cross-check the CPU oracle
tests/pose_oracle.py against it.  The reference is only read.

Run on a machine that has the reference checkout:   python -m tools.gen_golden_pose [builder] [ops] [e2e] [map]
Outputs (data only):
  tests/golden/builder_yolov{8,11}n-pose.json       layer table / save list / strides / parameter total / state_dict keys + shapes
  tests/golden/ops_pose.npz                         Pose heads (legacy and DWConv class branch, nc = 1; a (5, 2) keypoint shape) on three
                                                    tiny maps with their undecoded keypoints, scale_coords cases, kpt_iou / pose
                                                    _process_batch cases (the ragged matching batch of tests/test_hip_poseval.py)
  tests/golden/e2e_yolov{8,11}n-pose[_smooth].npz   B = 2 at 640 x 640: sampled head rows, (n, 6 + 51) NMS rows
  tests/golden/map_yolov8n-pose.npz                 the synthetic pose-mAP set: val-mode NMS rows, labels derived from them, the
                                                    reference's tp / tp_p / OKS matrices and box / pose ap_per_class tables
Every kpt_iou-bearing file is written only after the no-tie condition holds on the reference's own f32 values (pose_oracle.
no_tie_violations == 0): no same-class OKS within 1e-5 of a threshold, no detection with two candidate labels closer than 1e-5.
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
GOLD = ROOT / "tests" / "golden"

from oracle.ref_shim import import_reference  # noqa: E402
from tests import pose_oracle as PO  # noqa: E402
from tests.pose_cases import COORD_CASES, HEAD_CASES, HEAD_CH, HEAD_MAPS, MATCH_CASES, match_case_inputs  # noqa: E402
from tools.gen_golden_segment import bn_fix, layer_table, maxdiff  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

REF_YAML = {"yolov8n-pose": "/root/reference/ultralytics/cfg/models/v8/Pose/yolov8-pose.yaml",
            "yolov11n-pose": "/root/reference/ultralytics/cfg/models/v11/Pose/yolov11-pose.yaml"}
LIMIT = 1 << 20  # no committed file above 1 MiB


class _V:  # match_predictions only needs self.iouv (detect/val.py:59)
    iouv = torch.linspace(0.5, 0.95, 10)


def _ref_model(rt, name):
    import yaml
    d = yaml.safe_load(Path(REF_YAML[name]).read_text())
    d["scale"] = "n"
    return rt.PoseModel(d, ch=3, nc=None, verbose=False)


def builder_tables(rt):
    for name in REF_YAML:
        ref = _ref_model(rt, name)
        mine = PO.PoseModel(name + ".yaml")
        rsd, msd = ref.state_dict(), mine.state_dict()
        assert list(rsd) == list(msd) and all(tuple(rsd[k].shape) == tuple(msd[k].shape) for k in rsd), f"{name}: state_dict differs"
        assert layer_table(ref)[:-1] == layer_table(mine)[:-1], f"{name}: layer tables differ"
        assert list(ref.save) == list(mine.save) and torch.equal(ref.stride.float(), mine.stride.float())
        out = dict(config=name, layers=layer_table(ref), save=list(ref.save), stride=[float(x) for x in ref.stride], nc=int(ref.yaml["nc"]),
                   kpt_shape=[int(v) for v in ref.model[-1].kpt_shape], n_params=int(sum(p.numel() for p in ref.parameters())),
                   state_dict=[[k, list(v.shape)] for k, v in rsd.items()])
        (GOLD / f"builder_{name}.json").write_text(json.dumps(out, separators=(",", ":")))
        print(f"builder {name}: {out['n_params']} params, {len(out['layers'])} layers, nc={out['nc']}, save={out['save']}")


def head_case(rh, legacy, nc, kpt_shape, fam):
    old = rh.Pose.legacy
    rh.Pose.legacy = legacy
    try:
        r = bn_fix(rh.Pose(nc, kpt_shape, HEAD_CH))
    finally:
        rh.Pose.legacy = old
    o = bn_fix((PO.Pose if legacy else PO.Pose11)(nc, kpt_shape, HEAD_CH))
    for m in (r, o):
        m.stride = torch.tensor([8.0, 16.0, 32.0])
        m.bias_init()
        P.apply_procedural_weights(m, family=fam)
    xs = [P.uniform(f"unit:pose:{i}", (2, c, *hw), -1.0, 1.0) for i, (c, hw) in enumerate(zip(HEAD_CH, HEAD_MAPS))]
    return r, o, xs


def ref_pose_stats(rmet, BaseValidator, pred, pcls, boxes, gcls, gkpt, sigma):
    """The reference's own calls of PoseValidator._process_batch (pose/val.py:187-196) -> (OKS (M, N) f32, tp_p (N, 10) bool)."""
    import ultralytics.utils.ops as rops
    n, m = len(pcls), len(gcls)
    if n == 0 or m == 0:
        return np.zeros((m, n), np.float32), np.zeros((n, 10), bool)
    area = rops.xyxy2xywh(torch.from_numpy(boxes))[:, 2:].prod(1) * 0.53
    iou = rmet.kpt_iou(torch.from_numpy(gkpt), torch.from_numpy(pred), sigma=sigma, area=area)
    tp = BaseValidator.match_predictions(_V, torch.from_numpy(pcls), torch.from_numpy(gcls), iou).numpy()
    return iou.numpy(), tp


def check_against_oracle(iou, tp, pred, pcls, boxes, gcls, gkpt, sigma, what):
    assert PO.no_tie_violations(iou, pcls, gcls) == 0, f"{what}: the no-tie condition fails on the reference's own OKS"
    io, tpo = PO.process_batch_pose(torch.from_numpy(pred), torch.from_numpy(pcls), torch.from_numpy(boxes), torch.from_numpy(gcls),
                                    torch.from_numpy(gkpt), sigma)
    assert np.array_equal(np.asarray(io), iou) and np.array_equal(tpo, tp), f"{what}: tests/pose_oracle.py != reference"


def ops(rt):
    import ultralytics.nn.modules.head as rh
    import ultralytics.utils.ops as rops
    from ultralytics.engine.validator import BaseValidator
    from ultralytics.utils import metrics as rmet

    G = {}
    for tag, legacy, nc, kshape in HEAD_CASES:
        r, o, xs = head_case(rh, legacy, nc, kshape, "yolov8n-pose")
        assert list(r.state_dict()) == list(o.state_dict())
        yr, yo = r([t.clone() for t in xs]), o([t.clone() for t in xs])
        d = maxdiff(yr[0], yo[0])
        assert d <= 1e-4 and maxdiff(yr[1][1], yo[1][1]) <= 1e-4, d
        G[tag], G[tag + "_kpt"] = yr[0].numpy(), yr[1][1].numpy()
        print(f"op {tag}: out {tuple(yr[0].shape)} raw kpt {tuple(yr[1][1].shape)} oracle-vs-ref {d:.2e}")
    for name, img1, img0, padding, ndim, rp in COORD_CASES:
        c = P.uniform(f"unit:coords:{name}", (23, 17, ndim), -40.0, max(img1) + 40.0)
        ref = rops.scale_coords(img1, c.clone(), img0, ratio_pad=rp, padding=padding)
        assert torch.equal(ref, PO.scale_coords(img1, c, img0, ratio_pad=rp, padding=padding)), name
        G[f"coords_{name}"] = ref.numpy()
    G["match_cases"] = np.array([c[0] for c in MATCH_CASES])
    for name, n, m in MATCH_CASES:
        pred, pcls, boxes, gcls, gkpt, sigma = match_case_inputs(name, n, m)
        iou, tp = ref_pose_stats(rmet, BaseValidator, pred, pcls, boxes, gcls, gkpt, sigma)
        check_against_oracle(iou, tp, pred, pcls, boxes, gcls, gkpt, sigma, name)
        for k, v in (("pred", pred), ("pred_cls", pcls), ("gt_boxes", boxes), ("gt_cls", gcls), ("gt_kpt", gkpt), ("oks", iou), ("tp_p", tp)):
            G[f"match_{name}_{k}"] = v
        print(f"match {name}: {n} x {m}: TP@0.5 {int(tp[:, 0].sum())} TP@0.95 {int(tp[:, 9].sum())}, OKS >= 0.5 pairs {int((iou >= 0.5).sum())}")
    tp = G["match_two_cls_tp_p"]
    assert int(tp[:, 0].sum()) > int(tp[:, 9].sum()) > 0, "the matching batch is vacuous"
    np.savez_compressed(GOLD / "ops_pose.npz", **G)


def e2e(rt, name, smooth):
    from ultralytics.utils.nms import non_max_suppression as r_nms

    fam = ("smooth:" if smooth else "") + name
    ref = _ref_model(rt, name)
    P.apply_procedural_weights(ref, family=fam)
    ref.eval().fuse(verbose=False)
    mine = PO.PoseModel(name + ".yaml")
    P.apply_procedural_weights(mine, family=fam)
    mine.fuse()
    x = P.synthetic_images(2)
    nc = int(ref.yaml["nc"])
    with torch.no_grad():
        yr = ref(x.clone())[0]
        yo = mine(x.clone())[0]
    d = maxdiff(yr, yo)
    print(f"e2e {fam}: y {tuple(yr.shape)} oracle-vs-ref max|d| = {d:.3e}")
    assert d <= 2e-3, d
    A = yr.shape[-1]
    sel = np.unique(np.concatenate([np.arange(0, A, max(1, A // 256)), np.arange(64), np.arange(A - 64, A)]))
    G = {"oracle_vs_ref_maxdiff": np.array([d]), "anchor_sel": sel, "y_sel": yr[:, :, sel].numpy(), "nc": np.array(nc)}
    # conf 0.25 where scores reach it; procedural weights at nc = 1 put none there: then the middle of the widest gap between
    # neighbouring scores among the 150th - 250th largest, so that no score sits on the threshold
    cand = int((yr[:, 4:4 + nc] > 0.25).sum())
    top = yr[:, 4:4 + nc].flatten().topk(251).values
    k = 150 + int((top[150:250] - top[151:251]).argmax())
    conf = 0.25 if cand >= 20 else float((top[k] + top[k + 1]) / 2)
    near = float((yr[:, 4:4 + nc] - conf).abs().min())
    assert near > 1e-5, f"{fam}: a score sits {near:.1e} from the threshold"
    out_r = r_nms(yr.clone(), nc=nc, max_time_img=1e9, conf_thres=conf, iou_thres=0.7, max_det=300)
    G["conf_thres"] = np.array(conf)
    G["predict_n"] = np.array([o.shape[0] for o in out_r])
    G["predict_rows"] = torch.cat(out_r, 0).numpy()
    print(f"   predict (conf {conf:.4g}): n={[o.shape[0] for o in out_r]} rows {tuple(G['predict_rows'].shape)}")
    assert G["predict_rows"].shape[0] > 0 and G["predict_rows"].shape[1] == 6 + 51
    out = GOLD / f"e2e_{name}{'_smooth' if smooth else ''}.npz"
    np.savez_compressed(out, **G)
    assert out.stat().st_size <= LIMIT, out.stat().st_size


def synthetic_pose_labels(det, image_index):
    """Labels of the synthetic pose-mAP set, in the style of gen_golden_segval.synthetic_mask_labels: every third of the first 90
    detections; the box jittered; the keypoints moved by a hash-driven fraction of the box size, most of them small, so that OKS
    falls on both sides of every threshold; visibility in {0, 1, 2}; 15 % wrong classes."""
    n = det.shape[0]
    u = P.hash_uniform(f"posemap:gt:{image_index}", 8 * max(n, 1)).reshape(-1, 8)
    uk = P.hash_uniform(f"posemap:gtk:{image_index}", 3 * 17 * max(n, 1)).reshape(-1, 17, 3)
    boxes, cls, kpts = [], [], []
    for i in range(0, min(n, 90), 3):
        b = det[i, :4].clone()
        w, h = (b[2] - b[0]).clamp(min=1.0), (b[3] - b[1]).clamp(min=1.0)
        jit = torch.from_numpy(u[i, :4].copy()).float() - 0.5
        scale = 0.02 + 0.5 * float(u[i, 4]) ** 2
        boxes.append(b + jit * scale * torch.stack([w, h, w, h]))
        cls.append(det[i, 5] if u[i, 5] > 0.15 else det[i, 5] + 1)
        k = det[i, 6:].reshape(17, 3).clone()
        s = 0.3 * float(u[i, 6]) ** 2 * float(torch.sqrt(w * h))
        k[:, 0] += s * (torch.from_numpy(uk[i, :, 0].copy()).float() - 0.5)
        k[:, 1] += s * (torch.from_numpy(uk[i, :, 1].copy()).float() - 0.5)
        k[:, 2] = torch.floor(torch.from_numpy(uk[i, :, 2].copy()).float() * 3)
        kpts.append(k)
    if not boxes:
        return torch.zeros((0, 4)), torch.zeros((0,)), torch.zeros((0, 17, 3))
    return torch.stack(boxes), torch.stack(cls), torch.stack(kpts)


def map_golden(rt):
    from ultralytics.engine.validator import BaseValidator
    from ultralytics.utils import metrics as rmet
    from ultralytics.utils.nms import non_max_suppression as r_nms

    from ultralytics_pro_amd.utils import metrics as pmet

    name = "yolov8n-pose"
    ref = _ref_model(rt, name)
    P.apply_procedural_weights(ref, family=name)
    ref.eval().fuse(verbose=False)
    x = P.synthetic_images(4)
    yr = ref(x)[0]
    dets = r_nms(yr.clone(), conf_thres=0.001, iou_thres=0.7, nc=1, max_det=300, multi_label=True, max_time_img=1e9)
    G = {}
    acc = {k: [] for k in ("tp", "tp_p", "conf", "pcls", "tcls")}
    for i, d in enumerate(dets):
        gb, gc, gk = synthetic_pose_labels(d, i)
        pcls, gcls = d[:, 5].numpy(), gc.numpy().astype(np.float32)
        tp = BaseValidator.match_predictions(_V, d[:, 5], gc, rmet.box_iou(gb, d[:, :4])).numpy() if len(gcls) and len(pcls) \
            else np.zeros((len(pcls), 10), bool)
        pred = d[:, 6:].reshape(-1, 17, 3).numpy()
        oks, tp_p = ref_pose_stats(rmet, BaseValidator, pred, pcls, gb.numpy(), gcls, gk.numpy(), PO.OKS_SIGMA)
        check_against_oracle(oks, tp_p, pred, pcls, gb.numpy(), gcls, gk.numpy(), PO.OKS_SIGMA, f"image {i}")
        G[f"det{i}"], G[f"gt_boxes{i}"], G[f"gt_cls{i}"], G[f"gt_kpt{i}"] = d.numpy(), gb.numpy(), gcls, gk.numpy()
        G[f"tp{i}"], G[f"tp_p{i}"], G[f"oks{i}"] = tp, tp_p, oks
        for k, v in zip(acc, (tp, tp_p, d[:, 4].numpy(), pcls, gcls)):
            acc[k].append(v)
        print(f"map image {i}: {d.shape[0]} detections, {len(gcls)} labels, box TP@0.5 {int(tp[:, 0].sum())}, pose TP@0.5 "
              f"{int(tp_p[:, 0].sum())} @0.95 {int(tp_p[:, 9].sum())}")
    tp, tp_p, conf, pc, tc = (np.concatenate(acc[k], 0) for k in ("tp", "tp_p", "conf", "pcls", "tcls"))
    for tag, t in (("", tp), ("pose_", tp_p)):
        res = rmet.ap_per_class(t, conf, pc, tc)
        p_, r_, f1_, ap_, uc_ = res[2], res[3], res[4], res[5], res[6]
        po, ro, fo, apo, uco = pmet.ap_per_class(t, conf, pc, tc)  # the product's host AP arithmetic
        assert np.array_equal(ap_, apo) and np.array_equal(p_, po) and np.array_equal(r_, ro) and np.array_equal(uc_, uco)
        G.update({tag + "p": p_, tag + "r": r_, tag + "f1": f1_, tag + "ap": ap_, tag + "classes": uc_,
                  tag + "mean": np.array([p_.mean(), r_.mean(), ap_[:, 0].mean(), ap_.mean()])})
    assert int(tp_p[:, 0].sum()) > int(tp_p[:, 9].sum()) > 0, (int(tp_p[:, 0].sum()), int(tp_p[:, 9].sum()))
    assert 0.02 < G["pose_mean"][3] < 0.98 and G["pose_mean"][3] != G["mean"][3], (G["pose_mean"], G["mean"])
    print(f"map {name}: box {G['mean']}, pose {G['pose_mean']}")
    out = GOLD / f"map_{name}.npz"
    np.savez_compressed(out, **G)
    assert out.stat().st_size <= LIMIT, out.stat().st_size
    print(f"   {out.name}: {out.stat().st_size} bytes")


def main():
    torch.manual_seed(0)
    rt = import_reference()
    which = sys.argv[1:] or ["builder", "ops", "e2e", "map"]
    with torch.no_grad():
        if "builder" in which:
            builder_tables(rt)
        if "ops" in which:
            ops(rt)
        if "e2e" in which:
            for name in REF_YAML:
                e2e(rt, name, smooth=False)
                e2e(rt, name, smooth=True)
        if "map" in which:
            map_golden(rt)


if __name__ == "__main__":
    main()
