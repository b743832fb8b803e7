"""CPU (-m "not gpu"): classification model building.  `ClassificationModel("yolov{8,11}n-cls.yaml")` of the product package and of the
CPU oracle tests/classify_oracle.py reproduce the builder tables captured from the imported reference
(tests/golden/builder_yolov*n-cls.json, tools/gen_golden_classify.py), share their state_dict, and the head's host-side guards hold
without a GPU."""

import json

import pytest
import torch

from tests import classify_oracle as C
from ultralytics_pro_amd._lib import UpaError

NAMES = ["yolov8n-cls", "yolov11n-cls"]


def _table(m):
    return [dict(i=l.i, f=l.f, type=l.type.split(".")[-1], np=int(sum(p.numel() for p in l.parameters()))) for l in m.model]


def _check(m, g):
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == g["state_dict"]
    assert _table(m) == g["layers"]
    assert list(m.save) == g["save"]
    assert [float(s) for s in m.stride] == g["stride"] == [1.0]
    assert sum(p.numel() for p in m.parameters()) == g["n_params"]
    assert len(m.names) == g["nc"] and m.names[0] == "0"
    assert sorted({mod.eps for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)}) == g["bn_eps"]  # torch's default: no initialize_weights


@pytest.mark.parametrize("name", NAMES)
def test_product_builder_matches_reference(name, golden_dir):
    from ultralytics_pro_amd.nn.modules import Classify
    from ultralytics_pro_amd.nn.tasks import ClassificationModel
    g = json.loads((golden_dir / f"builder_{name}.json").read_text())
    m = ClassificationModel(name + ".yaml")
    _check(m, g)
    head = m.model[-1]
    assert isinstance(head, Classify) and head.export is False and not m.training
    assert [n for n, _ in head.named_children()] == ["conv", "pool", "drop", "linear"]
    i = len(m.model) - 1
    keys = set(m.state_dict())
    assert {f"model.{i}.conv.conv.weight", f"model.{i}.conv.bn.weight", f"model.{i}.conv.bn.running_var", f"model.{i}.linear.weight",
            f"model.{i}.linear.bias"} <= keys
    assert head.conv.conv.out_channels == 1280 and head.linear.in_features == 1280 and head.linear.out_features == g["nc"]
    assert g["n_params"] == {"yolov8n-cls": 2719288, "yolov11n-cls": 1633584}[name]  # the reference's summary lines


@pytest.mark.parametrize("name", NAMES)
def test_oracle_builder_matches_reference(name, golden_dir):
    g = json.loads((golden_dir / f"builder_{name}.json").read_text())
    _check(C.ClassificationModel(name + ".yaml"), g)


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_loads_both_ways(name):
    from ultralytics_pro_amd.nn.tasks import ClassificationModel
    from ultralytics_pro_amd.utils import procedural as P
    prod, orc = ClassificationModel(name + ".yaml"), C.ClassificationModel(name + ".yaml")
    P.apply_procedural_weights(orc)
    assert P.model_family(orc) == P.model_family(prod) == name
    res = prod.load_state_dict(orc.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    i = len(prod.model) - 1
    assert torch.equal(prod.state_dict()[f"model.{i}.linear.weight"], orc.state_dict()[f"model.{i}.linear.weight"])
    P.apply_procedural_weights(prod, family="smooth:" + name)
    res = orc.load_state_dict(prod.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(prod.state_dict()["model.0.conv.weight"], orc.state_dict()["model.0.conv.weight"])


def test_nc_override_reshape_outputs_and_scales():
    from ultralytics_pro_amd.nn.tasks import ClassificationModel, yaml_model_load
    m = ClassificationModel("yolov8n-cls.yaml", nc=10)
    assert m.model[-1].linear.out_features == 10 and len(m.names) == 10
    ClassificationModel.reshape_outputs(m, 7)
    assert m.model[-1].linear.out_features == 7 and m.model[-1].linear.in_features == 1280 and len(m.names) == 7
    ClassificationModel.reshape_outputs(m, 7)  # already there: untouched
    assert yaml_model_load("yolov11s-cls.yaml")["scale"] == "s" and yaml_model_load("yolov8x-cls.yaml")["scale"] == "x"
    # yolov8x-cls is the scale whose head reads 1280 input channels (upa_classify_pool's deepest K)
    assert ClassificationModel("yolov8x-cls.yaml").model[-1].conv.conv.in_channels == 1280
    assert m.set_compute_dtype(torch.bfloat16).compute_dtype == torch.bfloat16 and m.fuse().is_fused()


def test_head_refuses_what_is_out_of_scope():
    from ultralytics_pro_amd.nn.modules import Classify
    from ultralytics_pro_amd.nn.tasks import ClassificationModel, DetectionModel
    for kw in (dict(k=3), dict(g=2), dict(s=2)):
        with pytest.raises(UpaError):
            Classify(32, 10, **kw)
    h = Classify(32, 10).eval()
    with pytest.raises(UpaError):
        h([torch.zeros(1, 16, 2, 2), torch.zeros(1, 16, 2, 2)])  # list input
    with pytest.raises(UpaError):
        h(torch.zeros(1, 32, 2, 2))  # CPU tensor: no fallback
    with pytest.raises(UpaError):
        Classify(32, 10).train()(torch.zeros(1, 32, 2, 2))  # train mode
    with pytest.raises(UpaError):
        ClassificationModel("yolov8n.yaml")  # a Detect tail
    with pytest.raises(UpaError):
        ClassificationModel.reshape_outputs(DetectionModel("yolov8n.yaml"), 3)
    with pytest.raises(UpaError):
        ClassificationModel("yolov8n-cls.yaml")(torch.zeros(1, 3, 64, 64))


def test_abi_entries_are_bound():
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    assert len(L.PROTOTYPES["upa_classify_pool"][1]) == 15 and len(L.PROTOTYPES["upa_softmax_topk"][1]) == 9
    # host-side refusals need no GPU: nothing is launched
    assert lib.upa_softmax_topk(None, 1, 4, 4, None, 4, 1, None, None) == L.UPA_EINVAL
    assert b"softmax_topk" in lib.upa_last_error()
    assert lib.upa_classify_pool(None, 1, 1, 1, 16, 16, None, None, None, 16, 16, L.ACT_SILU, L.UPA_F32, None, None) == L.UPA_EINVAL
    assert b"classify_pool" in lib.upa_last_error()
