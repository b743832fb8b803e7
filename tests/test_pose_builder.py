"""CPU (-m "not gpu"): pose model building.  The product's `PoseModel("yolov{8,11}n-pose.yaml")` reproduces the builder tables captured
from the imported reference (tests/golden/builder_yolov*n-pose.json, tools/gen_golden_pose.py), and the host-side refusals (keypoint
shapes, training, the other validators) hold without a GPU."""

import json

import pytest


@pytest.mark.parametrize("name", ["yolov8n-pose", "yolov11n-pose"])
def test_product_builder_matches_reference(name, golden_dir):
    from ultralytics_pro_amd.nn.tasks import PoseModel
    g = json.loads((golden_dir / f"builder_{name}.json").read_text())
    m = PoseModel(name + ".yaml")
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == g["state_dict"]
    table = [dict(i=l.i, f=l.f, type=l.type.split(".")[-1], np=int(sum(p.numel() for p in l.parameters()))) for l in m.model]
    assert table == g["layers"]
    assert list(m.save) == g["save"]
    assert [float(s) for s in m.stride] == g["stride"]
    assert sum(p.numel() for p in m.parameters()) == g["n_params"]
    head = m.model[-1]
    assert type(head).__name__ == "Pose" and head.nc == g["nc"] and [int(v) for v in head.kpt_shape] == g["kpt_shape"] and head.nk == 51
    assert head.legacy_cls == (name == "yolov8n-pose")
    assert m.kpt_shape == (17, 3)
    # the 51-channel chain: the modules (and so the state_dict) keep the reference's widths, padding exists in the packed weights only
    assert [c.out_channels for c in (head.cv4[0][0].conv, head.cv4[0][1].conv, head.cv4[0][2])] == [51, 51, 51]


def test_pose_yaml_names_resolve_to_the_family_yaml_with_a_scale():
    from ultralytics_pro_amd.nn.tasks import yaml_model_load
    for name, scale in (("yolov8n-pose.yaml", "n"), ("yolov8s-pose.yaml", "s"), ("yolov11n-pose.yaml", "n"), ("yolov11m-pose.yaml", "m")):
        d = yaml_model_load(name)
        assert d["scale"] == scale and d["head"][-1][2] == "Pose" and d["kpt_shape"] == [17, 3], name


def test_data_kpt_shape_overrides_the_yaml():
    from ultralytics_pro_amd.nn.tasks import PoseModel
    m = PoseModel("yolov8n-pose.yaml", data_kpt_shape=(5, 2))
    assert m.kpt_shape == (5, 2) and m.model[-1].nk == 10 and m.model[-1].cv4[0][2].out_channels == 10


@pytest.mark.parametrize("kpt_shape,what", [((17, 4), r"kpt_shape\[1\]"), ((17, 1), r"kpt_shape\[1\]"), ((0, 3), r"kpt_shape\[0\]")])
def test_bad_keypoint_shapes_are_refused_naming_the_layer(kpt_shape, what):
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.nn.tasks import PoseModel
    with pytest.raises(L.UpaError, match=r"layer 22 \(Pose.*" + what):
        PoseModel("yolov8n-pose.yaml", data_kpt_shape=kpt_shape)


def test_pose_model_refuses_a_detection_yaml():
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.nn.tasks import PoseModel
    with pytest.raises(L.UpaError, match="Pose head"):
        PoseModel("yolov8n.yaml")


def test_trainer_and_other_validators_refuse_pose_models():
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer
    from ultralytics_pro_amd.engine.validator import DetectionValidator, PoseValidator, SegmentationValidator
    from ultralytics_pro_amd.nn.tasks import PoseModel
    m = PoseModel("yolov8n-pose.yaml")
    with pytest.raises(L.UpaError, match="pose training"):
        DetectionTrainer(m)
    for cls in (DetectionValidator, SegmentationValidator):
        with pytest.raises(L.UpaError, match="PoseValidator"):
            cls(m)
    v = PoseValidator(m)
    assert v.kpt_shape == (17, 3) and len(v.sigma) == 17
    assert list(PoseValidator(kpt_shape=(5, 2)).sigma) == [0.2] * 5  # ones(nkpt) / nkpt (pose/val.py:116)


def test_train_mode_pose_forward_raises():
    import torch

    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.nn.modules.head import Pose
    head = Pose(1, (17, 3), (16, 32, 64)).train()
    with pytest.raises(L.UpaError, match="pose training"):
        head([torch.zeros(1, 16, 4, 4), torch.zeros(1, 32, 2, 2), torch.zeros(1, 64, 1, 1)])
