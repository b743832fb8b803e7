"""CPU (-m "not gpu"): segmentation model building.  The product's `SegmentationModel("yolov{8,11}n-seg.yaml")` reproduces the builder
tables captured from the imported reference (tests/golden/builder_yolov*n-seg.json, tools/gen_golden_segment.py), and the host-side
refusals (training, validation) hold without a GPU."""

import json

import pytest


@pytest.mark.parametrize("name", ["yolov8n-seg", "yolov11n-seg"])
def test_product_builder_matches_reference(name, golden_dir):
    from ultralytics_pro_amd.nn.tasks import SegmentationModel
    g = json.loads((golden_dir / f"builder_{name}.json").read_text())
    m = SegmentationModel(name + ".yaml")
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == g["state_dict"]
    table = [dict(i=l.i, f=l.f, type=l.type.split(".")[-1], np=int(sum(p.numel() for p in l.parameters()))) for l in m.model]
    assert table == g["layers"]
    assert list(m.save) == g["save"]
    assert [float(s) for s in m.stride] == g["stride"]
    assert sum(p.numel() for p in m.parameters()) == g["n_params"]
    head = m.model[-1]
    assert type(head).__name__ == "Segment" and (head.nm, head.npr) == (32, 64)
    assert head.legacy_cls == (name == "yolov8n-seg")
    if name == "yolov11n-seg":
        assert g["n_params"] == 2876848  # the YAML's summary line


def test_seg_yaml_names_resolve_to_the_family_yaml_with_a_scale():
    from ultralytics_pro_amd.nn.tasks import yaml_model_load
    for name, stem, scale in (("yolov8n-seg.yaml", "yolov8-seg", "n"), ("yolov8t-seg.yaml", "yolov8-seg", "t"),
                              ("yolov11s-seg.yaml", "yolov11-seg", "s"), ("yolov8n.yaml", "yolov8", "n")):
        d = yaml_model_load(name)
        assert d["scale"] == scale and d["head"][-1][2] == ("Segment" if "seg" in stem else "Detect"), name


def test_every_yolo11_seg_scale_builds_with_the_yaml_parameter_counts():
    from ultralytics_pro_amd.nn.tasks import SegmentationModel
    want = {"n": 2876848, "s": 10113248, "m": 22420896}  # the reference YAML's summary lines
    for s, npar in want.items():
        assert sum(p.numel() for p in SegmentationModel(f"yolov11{s}-seg.yaml").parameters()) == npar


def test_segmentation_model_refuses_a_detection_yaml():
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.nn.tasks import SegmentationModel
    with pytest.raises(L.UpaError, match="Segment head"):
        SegmentationModel("yolov8n.yaml")


def test_trainer_and_validator_refuse_segmentation_models():
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer
    from ultralytics_pro_amd.engine.validator import DetectionValidator
    from ultralytics_pro_amd.nn.tasks import SegmentationModel
    m = SegmentationModel("yolov8n-seg.yaml")
    with pytest.raises(L.UpaError, match="segmentation"):
        DetectionTrainer(m)
    with pytest.raises(L.UpaError, match="mask mAP"):
        DetectionValidator(m)
