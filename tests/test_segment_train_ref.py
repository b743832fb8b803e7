"""CPU (-m "not gpu"): the float64 references of the segmentation-training kernels against torch autograd of the reference formula; the
CPU oracle step against the imported reference's record (tests/golden/train_yolov8n-seg.npz); the mask-id packing; SegmentationTrainer's
refusals (all raised before a device is touched); include/upa.h against the ctypes table for the new entries."""

import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import segment_train_ref as SR
from ultralytics_pro_amd.utils import procedural as P

ROOT = Path(__file__).resolve().parents[1]
CONVT_SHAPES = [(2, 5, 7, 16, 16), (1, 20, 20, 64, 64), (3, 9, 4, 32, 64)]


@pytest.mark.parametrize("shape", CONVT_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv_transpose_reference_is_autograd_of_conv_transpose2d(shape):
    n, h, w, cin, cout = shape
    x = P.uniform("ctb:x", (n, h, w, cin), -1.0, 1.0).double()
    wt = P.uniform("ctb:w", (cin, cout, 2, 2), -1.0, 1.0).double()
    dy = P.uniform("ctb:dy", (n, 2 * h, 2 * w, cout), -1.0, 1.0).double()
    (dx, dw, db), mags = SR.convt_bwd_ref(x, dy, wt)
    xa, wa = x.permute(0, 3, 1, 2).clone().requires_grad_(True), wt.clone().requires_grad_(True)
    ba = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    y = torch.nn.functional.conv_transpose2d(xa, wa, ba, stride=2)
    (y * dy.permute(0, 3, 1, 2)).sum().backward()
    for got, want, mag in ((dx, xa.grad.permute(0, 2, 3, 1), mags[0]), (dw, wa.grad, mags[1]), (db, ba.grad, mags[2])):
        assert got.shape == want.shape and bool(((got - want).abs() <= 1e-13 * mag + 1e-300).all())


def test_mask_loss_reference_is_autograd_of_the_reference_formula():
    case = SR.mask_case()
    ref = SR.mask_loss_ref(**case)
    item, dproto, dcoefs = SR.mask_loss_autograd(**case)
    assert ref["n_fg"] == 5
    assert abs(ref["item"] - item) <= 1e-12 * abs(item) and item > 0
    assert float((ref["dproto"] - dproto).abs().max()) <= 1e-12 * float(dproto.abs().max())
    for a, b in zip(ref["dcoefs"], dcoefs):
        assert float((a - b).abs().max()) <= 1e-12 * float(dproto.abs().max())
    # the cases the inputs are built for
    assert float(ref["dcoefs"][2][0].abs().max()) == 0.0          # the sub-pixel box: no pixel passes, the term and its gradient are 0
    assert float(ref["dcoefs"][0][0, 1, 1].abs().max()) > 0 and float(ref["dcoefs"][0][0, 1, 2].abs().max()) > 0  # anchors 6 and 7
    assert float(ref["dproto"][1].abs().max()) == 0.0 and float(ref["dproto"][2].abs().max()) == 0.0
    assert float(ref["dproto"][0].abs().max()) > 0


def test_mask_loss_reference_without_foreground_is_zero():
    case = SR.mask_case_no_foreground()
    ref = SR.mask_loss_ref(**case)
    assert ref["item"] == 0.0 and float(ref["dproto"].abs().max()) == 0.0 and all(float(d.abs().max()) == 0.0 for d in ref["dcoefs"])


def test_oracle_step_reproduces_the_reference_golden(golden_dir):
    from oracle import train as otr
    from tests import segment_oracle as S
    from tests import segment_train_oracle as ST
    G = np.load(golden_dir / "train_yolov8n-seg.npz")
    bs, imgsz, steps = (int(v) for v in G["a_shape"])
    assert float(G["a_oracle_vs_ref"][0]) <= 1e-6 and int(G["crop_mask_calls"][1]) > 0
    m = S.SegmentationModel("yolov8n-seg.yaml")
    P.apply_procedural_weights(m, family="yolov8n-seg")
    st = otr.TrainState(m)
    keys = [str(k) for k in G["a_param_keys"]]
    for step in range(steps):
        x, lab = P.synthetic_images(bs, h=imgsz, w=imgsz, seed=step), P.synthetic_labels(bs, seed=step)
        lab["masks"] = ST.overlap_masks(lab, bs, imgsz // 4, imgsz // 4)
        items, norm = ST.train_step(m, st, {"img": x, **lab})
        # the tolerances of the sibling CPU records (tests/test_detect_train11_golden.py): torch's f32 CPU convolutions sum in an order that
        # follows the thread count, so a re-run differs from the record in the last bits
        np.testing.assert_allclose(items.detach().numpy(), G[f"a_loss_items_{step}"], rtol=1e-4)
        np.testing.assert_allclose(norm, float(G[f"a_grad_norm_{step}"][0]), rtol=1e-4)
        named = dict(m.named_parameters())
        l2 = np.array([float(named[k].grad.double().norm()) for k in keys])
        np.testing.assert_allclose(l2, G[f"a_grad_l2_{step}"], rtol=1e-3, atol=1e-6 * float(G[f"a_grad_l2_{step}"].max()))
        for k in ("model.22.proto.upsample.weight", "model.22.proto.upsample.bias", "model.22.cv4.0.2.weight"):
            want = G[f"a_grad[{k}]_{step}"]
            # (atol: these are 1600-term f32 sums over n h w = 4 x 20 x 20 of sign-mixed products, re-associated by the thread count:
            # K u = 1600 x 2^-24 = 1e-4 of the magnitude sum, which is at least the tensor's largest element)
            np.testing.assert_allclose(named[k].grad.numpy(), want, rtol=1e-3, atol=1e-4 * float(np.abs(want).max()), err_msg=k)
        np.testing.assert_allclose(m.state_dict()["model.0.conv.weight"].numpy(), G[f"a_w_stem_{step}"], rtol=0, atol=1e-6)


def test_mask_ids_are_original_positions_when_a_zero_box_precedes_real_ones():
    from ultralytics_pro_amd.engine.trainer import pack_mask_ids, pack_targets
    lab = dict(batch_idx=torch.tensor([0.0, 0, 0, 1, 1, 0]), cls=torch.tensor([1.0, 2, 3, 4, 5, 6]),
               bboxes=torch.tensor([[0.0, 0, 0, 0], [0.5, 0.5, 0.2, 0.2], [0.3, 0.3, 0.1, 0.1], [0.0, 0, 0, 0], [0.6, 0.6, 0.2, 0.2],
                                    [0.7, 0.7, 0.1, 0.1]]))
    gt, ngt = pack_targets(lab, 2, 64, 64)
    mid = pack_mask_ids(lab, 2, 64, 64, int(gt.shape[1]))
    assert ngt.tolist() == [3, 1] and gt[0, :3, 0].tolist() == [2.0, 3.0, 6.0] and gt[1, 0, 0].item() == 5.0
    assert mid[0, :4].tolist() == [2, 3, 4, 0] and mid[1, :2].tolist() == [2, 0]   # position + 1, not row + 1
    assert mid.dtype == torch.int32 and tuple(mid.shape) == (2, int(gt.shape[1]))


def test_trainers_refuse_what_is_not_built_before_touching_a_device():
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer, SegmentationTrainer
    from ultralytics_pro_amd.nn.tasks import DetectionModel, SegmentationModel
    seg = SegmentationModel("yolov8n-seg.yaml")
    with pytest.raises(L.UpaError, match="SegmentationTrainer"):
        DetectionTrainer(seg, device="cuda:0")
    with pytest.raises(L.UpaError, match="overlap_mask=False"):
        SegmentationTrainer(seg, device="cuda:0", overlap_mask=False)
    with pytest.raises(L.UpaError, match="Segment head"):
        SegmentationTrainer(DetectionModel("yolov8n.yaml"), device="cuda:0")
    seg11 = SegmentationModel("yolov11n-seg.yaml")
    with pytest.raises(L.UpaError, match="yolo11=True"):
        SegmentationTrainer(seg11, device="cuda:0")
    with pytest.raises(L.UpaError, match="yolov8 Segment head only"):
        SegmentationTrainer(seg11, device="cuda:0", yolo11=True)
    assert all(p.device.type == "cpu" for p in seg.parameters())
    with pytest.raises(L.UpaError):
        seg.train()(torch.zeros(1, 3, 64, 64))  # the module itself keeps refusing train mode


def test_label_upload_refuses_masks_it_cannot_read():
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine.trainer import SegmentationTrainer as T
    ok = T.check_masks(dict(masks=torch.zeros(2, 40, 40)), 2, 40, 40)
    assert ok.dtype == torch.uint8 and tuple(ok.shape) == (2, 40, 40)
    with pytest.raises(L.UpaError, match="prototype resolution"):
        T.check_masks(dict(masks=torch.zeros(2, 160, 160)), 2, 40, 40)
    with pytest.raises(L.UpaError, match="overlap mask is"):
        T.check_masks(dict(masks=torch.zeros(5, 1, 40, 40)), 2, 40, 40)
    with pytest.raises(L.UpaError, match="integers in"):
        T.check_masks(dict(masks=torch.full((2, 40, 40), 300.0)), 2, 40, 40)
    with pytest.raises(L.UpaError, match='need "masks"'):
        T.check_masks(dict(cls=torch.zeros(1)), 2, 40, 40)


def test_mask_ids_share_the_keep_rule_of_the_gt_rows():
    """One statement of the rule (`_pixel_boxes`): the number of ids per image is the number of gt rows, whatever mix of zero boxes."""
    from ultralytics_pro_amd.engine.trainer import pack_mask_ids, pack_targets
    lab = P.synthetic_labels(4, seed=3)
    lab["bboxes"] = lab["bboxes"].clone()
    lab["bboxes"][::3] = 0.0
    gt, ngt = pack_targets(lab, 4, 160, 160)
    mid = pack_mask_ids(lab, 4, 160, 160, int(gt.shape[1]))
    assert ((mid > 0).sum(1).to(torch.int32) == ngt).all() and int(ngt.sum()) > 0


NEW_ENTRIES = ["upa_conv_transpose2x2_bwd_workspace_bytes", "upa_conv_transpose2x2_bwd", "upa_pack_conv_transpose2x2_weight_dev",
               "upa_detection_loss_assignment", "upa_mask_loss_workspace_bytes", "upa_mask_loss"]


def test_header_and_bindings_agree_on_the_new_signatures():
    import ctypes as C
    from ultralytics_pro_amd import _lib as L
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "upa.h").read_text(), flags=re.S)

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return C.c_void_p
        base = decl.rsplit(" ", 1)[0].replace("const", "").strip() if " " in decl else decl
        return {"int": C.c_int, "float": C.c_float, "size_t": C.c_size_t, "long": C.c_long}[base]
    for name in NEW_ENTRIES:
        m = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*[ \*])\s*" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, f"{name} not declared in include/upa.h"
        ret = C.c_void_p if "*" in m.group(1) else ctype(m.group(1).strip() + " x")
        args = [ctype(a) for a in m.group(2).split(",")]
        res, bound = L.PROTOTYPES[name]
        assert res == ret, (name, res, ret)
        assert bound == args, (name, [a.__name__ for a in bound], [a.__name__ for a in args])
