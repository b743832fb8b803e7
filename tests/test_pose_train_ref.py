"""CPU: the float64 reference of the keypoint loss against the autograd restatement of the reference's formulas, `pack_keypoints`
beside `pack_targets`, and `PoseTrainer`'s refusals (all of them on the host, before anything is uploaded or launched)."""

import importlib
from pathlib import Path

import pytest
import torch

from tests import pose_train_ref as PR

F32, BF16 = torch.float32, torch.bfloat16


@pytest.mark.parametrize("name", sorted(PR.CASES))
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_reference_equals_the_autograd_restatement(name, dtype):
    """Items and every gradient element to float64 rounding, on every case of the kernel test: an item is a sum of n_fg * nkpt terms
    taken in two different orders, (terms + 64) * 2^-52 of it; a gradient element is a product of a dozen factors, 1e-12 of the largest
    element.  The reference's zeros (background rows, pad columns, invisible keypoints) are zeros under autograd too."""
    case = dict(PR.kpt_case(name, dtype), scale=3.0 * 0.375)
    ref = PR.kpt_loss_ref(**case)
    items, grads = PR.kpt_loss_autograd(**case)
    rtol = (ref["n_fg"] * case["kpt_shape"][0] + 64) * 2.0 ** -52
    assert torch.allclose(ref["items"], items, rtol=rtol, atol=0), (ref["items"] - items, rtol)
    for want, got in zip(ref["dkpts"], grads):
        assert float((want - got).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1e-30)
        assert bool((got[want == 0] == 0).all())
    nk = case["kpt_shape"][0] * case["kpt_shape"][1]
    assert all(float(g[..., nk:].abs().max()) == 0.0 for g in ref["dkpts"] if g.shape[-1] > nk)
    if name == "none_fg":
        assert ref["n_fg"] == 0 and float(ref["items"].abs().max()) == 0.0
    else:
        assert ref["n_fg"] > 0 and float(ref["items"][0]) > 0
        assert (float(ref["items"][1]) > 0) == (case["kpt_shape"][1] == 3)


def test_base_case_holds_what_it_is_there_for():
    case = PR.kpt_case("coco17")
    ref = PR.kpt_loss_ref(**case)
    assert ref["n_fg"] == 7  # six on image 0, one on image 1; row >= n_gt, row -5 and the n_gt = 0 image are background
    # the label without a visible keypoint: its location gradients are exactly 0, its visibility gradients are not
    w0 = case["kpts"][0].shape[2]
    row = ref["dkpts"][0][0, 1, 15]
    assert float(row[0:51:3].abs().max()) == 0.0 and float(row[1:51:3].abs().max()) == 0.0 and float(row[2:51:3].abs().min()) > 0
    assert w0 == 20
    # the same gt at two strides
    assert float(ref["dkpts"][1][0, 1, 2].abs().max()) > 0 and float(ref["dkpts"][0][0, 2, 3].abs().max()) > 0


def test_wide_and_stride_cases_reach_the_clamp_and_the_zero_pass_stride():
    """On the default levels min(10 G, A) = 315 whatever G is: 79 workgroups, no clamp.  "all_wide" has A = 630 and G = 60."""
    assert PR.anchor_groups(PR.kpt_case("all_fg", G=60)) == (79, 79)
    wide = PR.kpt_case("all_wide")
    A = wide["assign"].shape[1]
    groups, want = PR.anchor_groups(wide)
    assert A == 630 and wide["gt"].shape[1] == 60 and (groups, want) == (128, 150)
    n_img = ((wide["assign"] >= 0) & (wide["assign"] < wide["n_gt"].view(-1, 1))).sum(1).tolist()
    assert n_img == [A] * 3 and -(-A // 4) - groups == 30  # workgroups 0..29 take a second turn
    for dtype, b_want in ((F32, 9), (BF16, 18)):
        case = PR.kpt_case("stride", dtype)
        b, A = case["assign"].shape
        items = PR.zero_pass_items(case, dtype)
        assert b == b_want and A == 4164 and items > PR.ZERO_PASS_ITEMS >= items // b * (b - 1)  # the smallest b
        fg = ((case["assign"] >= 0) & (case["assign"] < case["n_gt"].view(-1, 1))).nonzero().tolist()
        assert fg == [[0, 0], [0, 1], [0, 4095], [b - 1, 4096], [b - 1, 4160], [b - 1, A - 1]]


def _labels(boxes, kpts, bi):
    return dict(batch_idx=torch.tensor(bi, dtype=torch.float32), cls=torch.zeros(len(bi)), bboxes=torch.tensor(boxes, dtype=torch.float32),
                keypoints=kpts)


def test_pack_keypoints_lines_up_with_pack_targets_behind_a_zero_box():
    from ultralytics_pro_amd.engine.train.targets import pack_keypoints, pack_targets
    boxes = [[0, 0, 0, 0], [0.5, 0.5, 0.2, 0.4], [0.25, 0.25, 0.1, 0.1], [0.6, 0.4, 0.3, 0.3]]
    kp = torch.arange(4 * 3 * 3, dtype=torch.float32).view(4, 3, 3) / 100
    lab = _labels(boxes, kp, [0, 0, 1, 0])
    gt, ngt = pack_targets(lab, 2, 96, 160)
    out = pack_keypoints(lab, 2, 96, 160, int(gt.shape[1]), (3, 3))
    assert tuple(out.shape) == (2, int(gt.shape[1]), 3, 3) and ngt.tolist() == [2, 1]
    scale = torch.tensor([160.0, 96.0, 1.0])
    assert torch.equal(out[0, 0], kp[1] * scale) and torch.equal(out[0, 1], kp[3] * scale) and torch.equal(out[1, 0], kp[2] * scale)
    assert float(out[0, 2:].abs().max()) == 0.0 and float(out[1, 1:].abs().max()) == 0.0
    # the box of gt row 0 of image 0 is label 1's, not the dropped label 0's
    assert torch.allclose(gt[0, 0, 1:], torch.tensor([64.0, 28.8, 96.0, 67.2]))
    out2 = pack_keypoints(_labels(boxes, kp[..., :2].contiguous(), [0, 0, 1, 0]), 2, 96, 160, 4, (3, 2))
    assert bool((out2[0, :2, :, 2] == 1).all()) and torch.equal(out2[0, 0, :, :2], kp[1, :, :2] * scale[:2])


def test_targets_still_import_without_the_library():
    src = (Path(__file__).resolve().parent.parent / "ultralytics_pro_amd" / "engine" / "train" / "targets.py").read_text()
    assert "lib()" not in src and "import ctypes" not in src
    mod = importlib.import_module("ultralytics_pro_amd.engine.train.targets")
    assert hasattr(mod, "pack_keypoints")


class _NoDevice(Exception):
    pass


def _no_launch(monkeypatch):
    """Anything that would reach the device raises: the base trainer's constructor (it moves the model and allocates) and the base
    label upload."""
    from ultralytics_pro_amd.engine.train import trainer as T

    def boom(*a, **k):
        raise _NoDevice()
    monkeypatch.setattr(T.DetectionTrainer, "__init__", boom)
    monkeypatch.setattr(T.DetectionTrainer, "_upload_labels", boom)
    return T


def test_constructor_refusals_fire_on_the_host(monkeypatch):
    T = _no_launch(monkeypatch)
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.nn.tasks import DetectionModel, PoseModel
    with pytest.raises(UpaError, match="ends in a Pose head"):
        T.PoseTrainer(DetectionModel("yolov8n.yaml"))
    for kw in ({}, {"yolo11": True}):
        with pytest.raises(UpaError, match="yolov8 Pose head only"):
            T.PoseTrainer(PoseModel("yolov11n-pose.yaml"), **kw)
    with pytest.raises(_NoDevice):  # a yolov8 pose model passes every refusal and reaches the base constructor
        T.PoseTrainer(PoseModel("yolov8n-pose.yaml"))


def test_detection_trainer_still_refuses_a_pose_model_and_names_pose_trainer():
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer
    from ultralytics_pro_amd.nn.tasks import PoseModel
    with pytest.raises(UpaError, match="pose training") as ei:
        DetectionTrainer(PoseModel("yolov8n-pose.yaml"), device="cpu")
    assert "PoseTrainer" in str(ei.value)


def test_label_refusals_fire_before_the_upload(monkeypatch):
    T = _no_launch(monkeypatch)
    from ultralytics_pro_amd._lib import UpaError
    tr = object.__new__(T.PoseTrainer)
    tr.kpt_shape, tr._imgsz = (17, 3), (96, 160)
    boxes = [[0.5, 0.5, 0.2, 0.4], [0.25, 0.25, 0.1, 0.1]]
    good = torch.rand(2, 17, 3)
    lab = _labels(boxes, good, [0, 1])
    no_kp = {k: v for k, v in lab.items() if k != "keypoints"}
    with pytest.raises(UpaError, match='need "keypoints"'):
        tr._upload_labels(no_kp, 2)
    for bad in (torch.rand(2, 17, 2), torch.rand(3, 17, 3), torch.rand(2, 51)):
        with pytest.raises(UpaError, match="keypoints of shape"):
            tr._upload_labels(dict(lab, keypoints=bad), 2)
    for v in (float("nan"), float("inf")):
        bad = good.clone()
        bad[1, 3, 0] = v
        with pytest.raises(UpaError, match="non-finite"):
            tr._upload_labels(dict(lab, keypoints=bad), 2)
    with pytest.raises(_NoDevice):  # good labels pass every refusal and reach the upload
        tr._upload_labels(lab, 2)


def test_kpt_loss_refusals_precede_its_launches():
    """In the source of upa_kpt_loss every refusal stands before the first launch (the GPU refusal test relies on it); no atomics."""
    assert PR.refusals_precede_launches()
    src = (Path(__file__).resolve().parent.parent / "ultralytics_pro_amd" / "csrc" / "pose_train.hip").read_text()
    assert "atomicAdd" not in src


def test_oracle_step_reproduces_the_reference_golden(golden_dir):
    """The recorded `a_oracle_vs_ref` is within the generator's 1e-6, and the CPU oracle, run again here, follows the record at the
    tolerances of the sibling CPU records (tests/test_segment_train_ref.py: torch's f32 CPU convolutions sum in an order that follows
    the thread count, so a re-run differs from the record in the last bits)."""
    import numpy as np
    from oracle import train as otr
    from tests import pose_oracle as PO
    from tests import pose_train_oracle as PT
    from ultralytics_pro_amd.utils import procedural as P
    G = np.load(golden_dir / "train_yolov8n-pose.npz")
    bs, imgsz, steps = (int(v) for v in G["a_shape"])
    seed = int(G["a_label_seed"][0])
    assert float(G["a_oracle_vs_ref"][0]) <= 1e-6
    m = PO.PoseModel("yolov8n-pose.yaml")
    P.apply_procedural_weights(m, family="yolov8n-pose")
    st = otr.TrainState(m)
    keys = [str(k) for k in G["a_param_keys"]]
    for step in range(steps):
        x, lab = P.synthetic_images(bs, h=imgsz, w=imgsz, seed=seed + step), PT.pose_labels(bs, seed=seed + step)
        info = {}
        items, norm = PT.train_step(m, st, {"img": x, **lab}, info=info)
        assert int(info["fg_mask"].sum()) > 0 and float(items[1]) > 0 and float(items[2]) > 0
        np.testing.assert_allclose(items.detach().numpy(), G[f"a_loss_items_{step}"], rtol=1e-4)
        np.testing.assert_allclose(norm, float(G[f"a_grad_norm_{step}"][0]), rtol=1e-4)
        named = dict(m.named_parameters())
        l2 = np.array([float(named[k].grad.double().norm()) for k in keys])
        np.testing.assert_allclose(l2, G[f"a_grad_l2_{step}"], rtol=1e-3, atol=1e-6 * float(G[f"a_grad_l2_{step}"].max()))
        # atol = K u of the tensor's largest element, K the f32 terms that torch re-associates by the thread count on the way to an
        # element, u = 2^-24.  cv4.0.2 (the chain's last conv): one sum over n h w = 4 x 20 x 20 = 1600 sign-mixed products: 1e-4.
        # cv4.0.0 (its first): that sum of products whose factor dz has come back through two 3x3 convs (51 x 9 = 459 terms each) and
        # two BatchNorm backward reductions over the 1600 pixels: 1600 + 2 x 459 + 2 x 1600 = 5718 terms: 3.4e-4.
        for k, terms in (("model.22.cv4.0.2.weight", 1600), ("model.22.cv4.0.0.conv.weight", 5718)):
            want = G[f"a_grad[{k}]_{step}"]
            np.testing.assert_allclose(named[k].grad.numpy(), want, rtol=1e-3, atol=terms * 2.0 ** -24 * float(np.abs(want).max()), err_msg=k)
        sd = m.state_dict()
        np.testing.assert_allclose(sd["model.0.conv.weight"].numpy(), G[f"a_w_stem_{step}"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(sd["model.22.cv4.0.0.bn.running_var"].numpy(), G[f"a_bn_rv_{step}"], rtol=0, atol=1e-6)
