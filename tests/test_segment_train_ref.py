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


@pytest.mark.parametrize("shape", CONVT_SHAPES + sorted(set(sum(SR.CONVT_EXTRA.values(), []))), ids=lambda s: "x".join(str(v) for v in s))
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


F32, BF16 = torch.float32, torch.bfloat16
# every family in f32; in bf16 those whose shape follows the dtype (the depths, the zero pass's stride)
FAMILY_CASES = [(n, F32) for n in SR.family_names(F32)] + [(n, BF16) for n in SR.family_names(BF16) if n.startswith(("depth", "stride"))]


@pytest.mark.parametrize("name,dtype", FAMILY_CASES, ids=lambda v: v if isinstance(v, str) else str(v).split(".")[-1])
def test_family_reference_is_autograd_of_the_reference_formula(name, dtype):
    """The default scene's tolerances on every family: 1e-12 of the item, 1e-12 of dproto's largest element for the gradients."""
    case, ref = SR.family(name, dtype), SR.reference(name, dtype)
    item, dproto, dcoefs = SR.mask_loss_autograd(**case)
    assert ref["n_fg"] == sum(len(f) for f in SR.foreground(case)) > 0
    assert abs(ref["item"] - item) <= 1e-12 * abs(item) and item > 0
    assert float((ref["dproto"] - dproto).abs().max()) <= 1e-12 * float(dproto.abs().max())
    for a, b in zip(ref["dcoefs"], dcoefs):
        assert float((a - b).abs().max()) <= 1e-12 * float(dproto.abs().max())


def _crops(case, i):
    """(G, mh, mw) bool: the reference's own float32 crop decisions for the gt rows of image i."""
    mh, mw = case["masks"].shape[1:]
    mbox, _ = SR.mask_boxes(case["gt"], case["imgsz_h"], case["imgsz_w"], mh, mw)
    xs, ys = torch.arange(mw, dtype=torch.float32).view(1, 1, -1), torch.arange(mh, dtype=torch.float32).view(1, -1, 1)
    x1, y1, x2, y2 = (mbox[i, :, k].view(-1, 1, 1) for k in range(4))
    return (xs >= x1) & (xs < x2) & (ys >= y1) & (ys < y2)


def test_turns_family_holds_its_turns():
    case = SR.family("turns")
    fg, A = SR.foreground(case), case["assign"].shape[1]
    starts = [0, 400, 500]
    assert A == 525 and -(-A // 256) == 3 and A % 256 == 13 and starts == [0, 20 * 20, 20 * 20 + 10 * 10]
    assert fg[0] == [0, 255, 256, 399, 400, 499, 500, 524]          # both sides of 255 / 256 and of each level start, the last anchor
    assert min(fg[1]) == 256 and max(fg[1]) == 511 and len(fg[1]) == 6 and int(case["assign"][1, 7]) >= int(case["n_gt"][1])
    assert fg[2] == list(range(A))
    lanes = SR.anchor_lanes(case)
    assert lanes == 40 and -(-len(fg[2]) // lanes) == 14 and len(fg[2]) // lanes == 13   # every workgroup takes 13 or 14 turns
    assert -(-len(fg[2]) // 256) == 3                                                   # ml_finish_kernel's strides
    crops = _crops(case, 2)
    npx = crops.flatten(1).sum(1).tolist()
    assert npx[1] == 24 * 40 and npx[2] > 4 * 64 and npx[2] % 64 != 0
    ys, xs = crops[0].nonzero(as_tuple=True)
    assert len(ys) > 0 and len(set((ys // 8).tolist())) == 1 and len(set((xs // 8).tolist())) == 1   # wholly inside one 8 x 8 tile
    assert bool(crops[3][:, -1].any()) and bool(crops[3][-1].any())                                   # reaches the right / bottom edge
    # records per 8 x 8 tile of image 2: every tile is met by the whole-mask box's records at least
    per_gt = torch.bincount(case["assign"][2].long(), minlength=4)
    tiles = crops.view(4, 3, 8, 5, 8).any(4).any(2)  # (gt, tile row, tile column)
    assert int((tiles * per_gt.view(4, 1, 1)).sum(0).min()) >= 100


def test_clamp_family_fills_the_clamped_grid():
    case = SR.family("clamp")
    fg, A, G = SR.foreground(case), case["assign"].shape[1], case["gt"].shape[1]
    assert G == 52 and 10 * G > 512 and A > 512 and SR.anchor_lanes(case) == 512
    assert fg[0] == list(range(A)) and len(fg[0]) - 512 == 13 and len(fg[1]) == 3
    assert len(set(case["assign"][0].tolist())) == 52
    for perm in ("turns_permuted", "clamp_permuted"):
        base, other = SR.family(perm.split("_")[0]), SR.family(perm)
        assert SR.foreground(base) == SR.foreground(other) and not torch.equal(base["assign"], other["assign"])


def test_depth_level_and_stride_families_hold_their_shapes():
    for dtype, vec in ((F32, 4), (BF16, 8)):
        assert all(nm % vec == 0 and nm <= 128 for nm in SR.DEPTHS[dtype]) and 128 in SR.DEPTHS[dtype] and min(SR.DEPTHS[dtype]) == vec
        assert all(SR.family(f"depth{nm}", dtype)["proto"].shape[3] == nm for nm in SR.DEPTHS[dtype])
        case = SR.family("stride", dtype)
        b, A = case["assign"].shape
        assert SR.zero_pass_items(case, dtype) > SR.ZERO_PASS_ITEMS >= SR.zero_pass_items(case, dtype) // b * (b - 1)   # the smallest b
        fg = SR.foreground(case)
        assert all(f == [0, 1, 4095, 4096, 4160, 4163] for f in fg) and A == 4164 and fg[-1][-1] == A - 1
    one, two = SR.family("levels1"), SR.family("levels2")
    assert len(one["coefs"]) == 1 and one["assign"].shape[1] == 20 and SR.reference("levels1")["n_fg"] == 3
    assert len(two["coefs"]) == 2 and two["assign"].shape[1] == 26 and SR.reference("levels2")["n_fg"] == 4


def test_edges_family_decides_every_pixel_as_float32_does_and_sees_a_reciprocal_multiply():
    """Sizes 96 x 80 -> 24 x 20: v / 96 and v / 80 are inexact in float32.  A numpy float32 emulation of the crop rule gives the
    reference's decision at every pixel of every box; with the divide replaced by a multiply with the float32 reciprocal at least one
    pixel is decided the other way, so a kernel that did that would leave the reference's exact zeros."""
    case = SR.family("edges")
    rows = case["edge_rows"]
    assert {(e, kind) for _, e, kind, _, _ in rows} == {(e, kind) for e in range(4) for kind in (-1, 0, 1)} and len(rows) == 24
    assert SR.foreground(case) == [list(range(26))] and int(case["n_gt"][0]) == 26
    mh, mw = SR.EDGE_MASK
    mbox, _ = SR.mask_boxes(case["gt"], case["imgsz_h"], case["imgsz_w"], mh, mw)
    for g, e, kind, k, _ in rows:  # the built boxes carry the searched kinds
        want = np.float32(k) if kind == 0 else np.nextafter(np.float32(k), np.float32(kind * np.inf))
        assert np.float32(mbox[0, g, e]) == want, (g, e, kind, k)
    ref_crops = _crops(case, 0).numpy()
    boxes = case["gt"][0, :, 1:5]
    assert np.array_equal(SR.crop_decisions(boxes, case["imgsz_h"], case["imgsz_w"], mh, mw), ref_crops)
    other = SR.crop_decisions(boxes, case["imgsz_h"], case["imgsz_w"], mh, mw, reciprocal=True)
    assert int((other != ref_crops).sum()) >= 1 and any(f for *_, f in rows)
    # the two boxes outside the mask: exactly-zero terms
    ref = SR.reference("edges")
    flat = torch.cat([d.reshape(1, -1, 32) for d in ref["dcoefs"]], 1)[0]
    ferr = torch.cat([d.reshape(1, -1, 32) for d in ref["dcoefs_err"]], 1)[0]
    zero = [a for a in range(26) if float(flat[a].abs().max()) == 0.0 and float(ferr[a].max()) == 0.0]
    assert zero == [24, 25] and not ref_crops[24:].any() and all(ref_crops[g].any() for g in range(24))


def test_split_arithmetic_of_the_new_conv_transpose_shapes():
    assert SR.ctb_splits(16, 16, 1023, 4) == (8, 128) and SR.ctb_splits(16, 16, 1023, 32) == (8, 128) and 1023 % 128 != 0
    assert SR.ctb_splits(16, 16, 8192, 4)[0] == 64 and SR.ctb_splits(16, 16, 8192, 32)[0] == 64
    assert SR.ctb_splits(128, 128, 9, 4)[0] == 1 and SR.ctb_splits(64, 64, 400, 4)[0] == 4
    for dtype, vec in ((F32, 4), (BF16, 8)):
        assert all(s[3] % vec == 0 and s[4] % vec == 0 for s in SR.CONVT_EXTRA[dtype])
        assert any(s[3] > 64 and s[3] % 64 for s in SR.CONVT_EXTRA[dtype]) and any(4 * s[4] % 64 for s in SR.CONVT_EXTRA[dtype])


def test_mask_loss_refusals_stand_before_the_first_launch():
    assert SR.refusals_precede_launches()


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
