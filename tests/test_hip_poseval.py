"""-m gpu: pose validation on the HIP path: `upa_pose_match` (OKS + the claim step) against the reference's `kpt_iou` and
`match_predictions` outputs (tests/golden/ops_pose.npz, map_yolov8n-pose.npz) and the float64 restatement tests/pose_oracle.py, the public
`kpt_iou`, the refusals, `PoseValidator` on the reference's detections, and a captured `update`."""

import numpy as np
import pytest
import torch

from tests import kernel_check as KC
from tests import pose_oracle as PO
from tests import pose_cases as GP
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _batch(cases, max_det, max_gt, dev):
    """The named cases of ops_pose.npz's matching batch as one ragged batch; rows past counts / ngt are NaN."""
    b = len(cases)
    kshape = (5, 2) if cases[0][0] == "k5" else (17, 3)
    nkpt, ndim = kshape
    rows = torch.full((b, max_det, 6 + nkpt * ndim), NAN)
    gt, gk = torch.full((b, max_gt, 5), NAN), torch.full((b, max_gt, nkpt, 3), NAN)
    cnt, ngt, ins = [], [], []
    for i, (name, n, m) in enumerate(cases):
        pred, pcls, boxes, gcls, gkpt, sigma = GP.match_case_inputs(name, n, m)
        rows[i, :n, :5], rows[i, :n, 5], rows[i, :n, 6:] = 0.0, torch.from_numpy(pcls), torch.from_numpy(pred).reshape(n, nkpt * ndim)
        gt[i, :m, 0], gt[i, :m, 1:], gk[i, :m] = torch.from_numpy(gcls), torch.from_numpy(boxes), torch.from_numpy(gkpt)
        cnt.append(n)
        ngt.append(m)
        ins.append((pred, pcls, boxes, gcls, gkpt, sigma))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
    return rows.to(dev), i32(cnt), gt.to(dev), i32(ngt), gk.to(dev), kshape, ins


@KC.stop_after_fault
@pytest.mark.parametrize("group", ["ragged", "max_gt_1", "k5"])
def test_pose_match_against_the_reference(group, golden_dir):
    """tp_p equals the reference's exactly; the OKS matrix against the float64 restatement within four times the f32 reference's own
    distance from float64 on the same case (floored at 1e-6).  Measured on an MI355X (two_cls / one_label / k5): the f32 reference
    sits 5.7e-8 / 1.3e-7 / 5.6e-8 from float64 - so the floor, 1e-6, is the gate - and the kernel 1.2e-7 / 1.4e-7 / 5.6e-8.
    ragged: an image with 0 labels, one with 0 detections, a label with every keypoint invisible, a zero-area label box, two classes,
    NaN past counts / ngt; max_gt_1: 300 detections on one label in a max_gt = 1 batch; k5: five two-value keypoints, sigma = 1 / 5."""
    from ultralytics_pro_amd.utils import metrics as M
    DEV = KC.env()[0]
    g = np.load(golden_dir / "ops_pose.npz")
    by = {c[0]: c for c in GP.MATCH_CASES}
    cases, max_det, max_gt = {"ragged": ([by["two_cls"], by["no_labels"], by["no_dets"]], 44, 7),
                              "max_gt_1": ([by["one_label"]], 300, 1), "k5": ([by["k5"]], 32, 6)}[group]
    rows, cnt, gt, ngt, gk, kshape, ins = _batch(cases, max_det, max_gt, DEV)
    sigma = ins[0][5]

    def run():
        tp = KC.out_buf((len(cases), max_det), 10, torch.uint8, spare=1, fill=0xEE)
        oks = KC.out_buf((len(cases), max_det), max_gt, torch.float32, spare=1)
        M.match_keypoints_batched(rows, cnt, gt, ngt, gk, kshape, sigma, out=tp[:len(cases)], oks_out=oks[:len(cases)])
        torch.cuda.synchronize()
        return tp, oks
    tp, oks = KC.twice(run, "pose_match")
    tp_ = KC.payload(tp, len(cases), 10, group, fill=0xEE)
    oks_ = KC.payload(oks, len(cases), max_gt, group)
    for i, (name, n, m) in enumerate(cases):
        pred, pcls, boxes, gcls, gkpt, _ = ins[i]
        assert np.array_equal(tp_[i, :n].numpy().astype(bool), g[f"match_{name}_tp_p"]), f"{name}: tp_p differs from the reference's"
        assert not bool(tp_[i, n:].any()) and not bool(oks_[i, n:].any()) and not bool(oks_[i, :, m:].any()), name
        if n and m:
            same = torch.from_numpy(gcls)[:, None] == torch.from_numpy(pcls)[None]
            o64 = PO.kpt_iou_f64(torch.from_numpy(gkpt), torch.from_numpy(pred), PO.label_area(torch.from_numpy(boxes)), sigma) * same
            ref32 = torch.from_numpy(g[f"match_{name}_oks"]).double() * same
            own = float((ref32 - o64).abs().max())
            tol = max(4 * own, 1e-6)
            err = float((oks_[i, :n, :m].t().double() - o64).abs().max())
            print(f"pose_match {name}: f32 reference vs f64 {own:.2e}, kernel vs f64 {err:.2e} (gate {tol:.2e})")
            assert err <= tol, (name, err, tol)


@KC.stop_after_fault
def test_public_kpt_iou(golden_dir):
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.utils import metrics as M
    DEV = KC.env()[0]
    g = np.load(golden_dir / "ops_pose.npz")
    for name in ("two_cls", "k5"):
        pred, pcls, boxes, gcls, gkpt, sigma = GP.match_case_inputs(name, *[c[1:] for c in GP.MATCH_CASES if c[0] == name][0])
        keep = np.array([k for k in range(len(gcls)) if boxes[k, 2] > boxes[k, 0]])  # the public form divides area by 0.53: no zero areas
        area = PO.label_area(torch.from_numpy(boxes))[keep]
        out = M.kpt_iou(torch.from_numpy(gkpt[keep]).to(DEV), torch.from_numpy(pred).to(DEV), area.to(DEV), sigma)
        ref = PO.kpt_iou_f64(torch.from_numpy(gkpt[keep]), torch.from_numpy(pred), area, sigma)
        assert out.shape == ref.shape and float((out.cpu().double() - ref).abs().max()) <= 1e-5
    k = torch.zeros((3, 17, 3), device=DEV)
    assert M.kpt_iou(k[:0], k, torch.zeros(0, device=DEV), PO.OKS_SIGMA).shape == (0, 3)
    with pytest.raises(UpaError):
        M.kpt_iou(torch.zeros(2, 17, 3), torch.zeros(2, 17, 3), torch.ones(2), PO.OKS_SIGMA)  # CPU tensors: no fallback
    assert np.array_equal(M.OKS_SIGMA, PO.OKS_SIGMA)


@KC.stop_after_fault
def test_pose_match_refusals_leave_every_buffer_untouched():
    DEV, L, lib, stream = KC.env()
    b, max_det = 1, 4
    thr = np.ascontiguousarray(np.linspace(0.5, 0.95, 10).astype(np.float32))

    def call(nkpt=17, ndim=3, ld=None, max_gt=4, n_thr=10, null=None):
        ld = ld or 6 + nkpt * ndim
        sg = np.ones(max(nkpt, 1), np.float32)
        rows = torch.zeros((b, max_det, max(ld, 1)), device=DEV)
        cnt = torch.full((b,), max_det, dtype=torch.int32, device=DEV)
        gt = torch.zeros((b, max_gt, 5), device=DEV)
        ngt = torch.full((b,), min(max_gt, 4), dtype=torch.int32, device=DEV)
        gk = torch.zeros((b, max_gt, max(nkpt, 1), 3), device=DEV)
        tp = torch.full((b, max_det, 10), 0xFF, dtype=torch.uint8, device=DEV)
        oks = torch.full((b, max_det, max_gt), NAN, device=DEV)
        ptr = dict(rows=rows.data_ptr(), counts=cnt.data_ptr(), gt=gt.data_ptr(), ngt=ngt.data_ptr(), gt_kpt=gk.data_ptr(), sigma=sg.ctypes.data,
                   thr=thr.ctypes.data, tp=tp.data_ptr())
        if null:
            ptr[null] = None
        rc = lib.upa_pose_match(ptr["rows"], ld, b, max_det, ptr["counts"], ptr["gt"], ptr["ngt"], max_gt, ptr["gt_kpt"], nkpt, ndim,
                                ptr["sigma"], ptr["thr"], n_thr, ptr["tp"], oks.data_ptr(), stream)
        torch.cuda.synchronize()
        return rc, bool((tp == 0xFF).all()) and bool(torch.isnan(oks).all())

    assert call() == (0, False)                                   # the accepted form writes
    assert call(ndim=4) == (L.UPA_EUNSUPPORTED, True)
    assert call(nkpt=65) == (L.UPA_EUNSUPPORTED, True)            # sigma travels by value: 64 keypoints
    assert call(ld=56) == (L.UPA_EINVAL, True)                    # rows narrower than 6 + nk
    assert call(n_thr=9) == (L.UPA_EINVAL, True)
    assert call(max_gt=1024) == (L.UPA_EINVAL, True)              # 1024 x (10 + 51 + 3) x 4 B of label tables > LDS
    for name in ("rows", "counts", "gt", "ngt", "gt_kpt", "sigma", "thr", "tp"):
        assert call(null=name) == (L.UPA_EINVAL, True), name


def _map_labels(MAP, dev, max_gt=64):
    gt, gk, ngt = torch.zeros(4, max_gt, 5), torch.zeros(4, max_gt, 17, 3), []
    for i in range(4):
        m = MAP[f"gt_cls{i}"].shape[0]
        gt[i, :m, 0], gt[i, :m, 1:], gk[i, :m] = (torch.from_numpy(MAP[f"{k}{i}"]) for k in ("gt_cls", "gt_boxes", "gt_kpt"))
        ngt.append(m)
    return gt.to(dev), torch.tensor(ngt, dtype=torch.int32, device=dev), gk.to(dev)


@KC.stop_after_fault
def test_pose_validator_reproduces_the_reference_map(golden_dir):
    """The reference's own val-mode detections (map_yolov8n-pose.npz) through PoseValidator.update_detections, as one batch and as two
    batches of two: tp and tp_p equal the reference's, box and pose P / R / mAP50 / mAP50-95 to 1e-7.  pack_keypoints on the same
    labels gives the stored rows."""
    from ultralytics_pro_amd.engine.validator import PoseValidator
    DEV = KC.env()[0]
    MAP = np.load(golden_dir / "map_yolov8n-pose.npz")
    gt, ngt, gk = _map_labels(MAP, DEV)
    rows = torch.zeros(4, 300, 57)
    cnt = []
    for i in range(4):
        d = torch.from_numpy(MAP[f"det{i}"])
        rows[i, :d.shape[0]] = d
        cnt.append(d.shape[0])
    rows, cnt = rows.to(DEV), torch.tensor(cnt, dtype=torch.int32, device=DEV)
    lab = dict(batch_idx=torch.cat([torch.full((int(k),), i) for i, k in enumerate(ngt.tolist())]),
               keypoints=torch.cat([torch.from_numpy(MAP[f"gt_kpt{i}"]) for i in range(4)]))
    assert torch.equal(PoseValidator().pack_keypoints(lab, 4, DEV), gk)
    ref_tp = np.concatenate([MAP[f"tp{i}"] for i in range(4)], 0)
    ref_tpp = np.concatenate([MAP[f"tp_p{i}"] for i in range(4)], 0)
    for split in ((0, 4),), ((0, 2), (2, 4)):
        v = PoseValidator(kpt_shape=(17, 3))
        for a, b in split:
            v.update_detections(rows[a:b].contiguous(), cnt[a:b].contiguous(), gt[a:b].contiguous(), ngt[a:b].contiguous(), gk[a:b].contiguous())
        st = v.get_stats()
        assert np.array_equal(st["tp"], ref_tp) and np.array_equal(st["tp_p"], ref_tpp)
        box, pose = np.array(st["mean"]), np.array(st["pose"]["mean"])
        print(f"validator {split}: box {box} (reference {MAP['mean']}), pose {pose} (reference {MAP['pose_mean']})")
        assert np.abs(box - MAP["mean"]).max() <= 1e-7 and np.abs(pose - MAP["pose_mean"]).max() <= 1e-7
        assert np.abs(st["pose"]["ap"] - MAP["pose_ap"]).max() <= 1e-7


@KC.stop_after_fault
def test_update_step_graph_replay_equals_eager(golden_dir):
    from ultralytics_pro_amd.engine.validator import PoseValidator
    from ultralytics_pro_amd.nn.tasks import PoseModel
    DEV = KC.env()[0]
    MAP = np.load(golden_dir / "map_yolov8n-pose.npz")
    m = PoseModel("yolov8n-pose.yaml")
    P.apply_procedural_weights(m, family="yolov8n-pose")
    m = m.to(DEV).eval()
    x = P.synthetic_images(2).to(DEV).contiguous()
    gt, ngt, gk = (t[:2].contiguous() for t in _map_labels(MAP, DEV))
    v = PoseValidator(m)
    post = lambda o: v.update(o, gt, ngt, gk, key="poseval_replay", record=False)  # noqa: E731
    with torch.no_grad():
        e = post(m(x))
        torch.cuda.synchronize()
        eager = [t.clone() for t in e]
        run = m.compile(x, post=post)
        r1 = [t.clone() for t in run()]
        r2 = run()
    torch.cuda.synchronize()
    assert int(eager[1].sum()) > 0 and bool(eager[3].any())
    for a, b_, c in zip(eager, r1, r2):
        assert torch.equal(a, b_) and torch.equal(a, c)
    v.add_batch_stats(r2[0], r2[1], r2[2], gt, ngt, r2[3])
    st = v.get_stats()
    assert st["tp_p"].shape[0] == int(eager[1].sum()) and "pose" in st
