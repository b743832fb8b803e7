"""CPU (-m "not gpu"): YOLO11 model building and the CPU checker.  The product's `DetectionModel("yolov11{n,m}.yaml")` reproduces the
builder tables captured from the imported reference (tests/golden/builder_yolov11*.json, tools/gen_golden_yolo11.py), the CPU oracle
tests/yolo11_oracle.py reproduces the reference's per-op and end-to-end outputs, and the host-side guards that keep YOLO11 off the
C2f / legacy-Detect fused forms hold without a GPU."""

import json

import numpy as np
import pytest
import torch

from tests import yolo11_oracle as Y
from ultralytics_pro_amd.utils import procedural as P


@pytest.mark.parametrize("name", ["yolov11n", "yolov11m"])
def test_product_builder_matches_reference(name, golden_dir):
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    g = json.loads((golden_dir / f"builder_{name}.json").read_text())
    m = DetectionModel(name + ".yaml")
    assert [[k, list(v.shape)] for k, v in m.state_dict().items()] == g["state_dict"]
    table = [dict(i=l.i, f=l.f, type=l.type.split(".")[-1], np=int(sum(p.numel() for p in l.parameters()))) for l in m.model]
    assert table == g["layers"]
    assert list(m.save) == g["save"]
    assert [float(s) for s in m.stride] == g["stride"]
    assert sum(p.numel() for p in m.parameters()) == g["n_params"]
    if name == "yolov11n":
        assert g["n_params"] == 2624080  # the YAML's summary line
    # the m scale forces C3k inner blocks everywhere (tasks.py:2863)
    c3k = [type(b).__name__ for l in m.model if type(l).__name__ == "C3k2" for b in l.m]
    assert set(c3k) == ({"C3k"} if name == "yolov11m" else {"Bottleneck", "C3k"})
    assert not m.model[-1].legacy_cls


def test_every_yolo11_scale_builds_with_the_yaml_parameter_counts():
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    want = {"n": 2624080, "s": 9458752, "m": 20114688, "l": 25372160, "x": 56966176}  # the YAML's summary lines
    for s, npar in want.items():
        assert sum(p.numel() for p in DetectionModel(f"yolov11{s}.yaml").parameters()) == npar


def test_building_yolo11_leaves_the_legacy_head_of_later_models():
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    DetectionModel("yolov11n.yaml")
    m = DetectionModel("yolov8n.yaml")
    assert m.model[-1].legacy_cls and type(m.model[-1].cv3[0][0]).__name__ == "Conv"


@pytest.mark.parametrize("name", [c[0] for c in Y.op_cases()])
def test_oracle_reproduces_reference_ops(name, golden_dir):
    g = np.load(golden_dir / "ops_yolo11.npz")
    _, cls, args, xshape = {c[0]: c for c in Y.op_cases()}[name]
    o = Y.ORACLE_CLASSES[cls](*args)
    for mod in o.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eps, mod.momentum = 1e-3, 0.03
    o.eval()
    P.apply_procedural_weights(o, family="yolov11n")
    with torch.no_grad():
        y = o(P.uniform(f"unit:{name}", xshape, -1.0, 1.0))
    ref = torch.from_numpy(g[name])
    assert y.shape == ref.shape
    assert float((y - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))


def test_oracle_reproduces_reference_nonlegacy_detect(golden_dir):
    g = np.load(golden_dir / "ops_yolo11.npz")
    ch = (64, 128, 256)
    o = Y.Detect(80, ch)
    for mod in o.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eps, mod.momentum = 1e-3, 0.03
    o.eval()
    o.stride = torch.tensor([8.0, 16.0, 32.0])
    o.bias_init()
    P.apply_procedural_weights(o, family="yolov11n")
    xs = [P.uniform(f"unit:detect11:{i}", (2, c, s, s), -1.0, 1.0) for i, (c, s) in enumerate(zip(ch, (16, 8, 4)))]
    with torch.no_grad():
        y = o(xs)[0]
    assert float((y - torch.from_numpy(g["detect11"])).abs().max()) <= 1e-4


@pytest.mark.parametrize("family", ["yolov11n", "smooth:yolov11n"])
def test_oracle_reproduces_reference_e2e(family, golden_dir):
    from oracle import nms as onms
    g = np.load(golden_dir / f"e2e_yolov11n{'_smooth' if family.startswith('smooth') else ''}.npz")
    o = Y.DetectionModel("yolov11n.yaml")
    P.apply_procedural_weights(o, family=family)
    o.fuse()
    with torch.no_grad():
        y = o(P.synthetic_images(2))[0]
    d = np.abs(y[:, :, g["anchor_sel"]].numpy() - g["y_sel"])
    assert d.max() <= 1e-3  # the f32 model sits within 5e-4 px / 3e-6 of its float64 run on this recipe (utils/procedural.py)
    out = onms.non_max_suppression(y, conf_thres=0.25, iou_thres=0.7, max_det=300)
    assert [r.shape[0] for r in out] == list(g["predict_n"])
    assert sum(g["predict_n"]) > 0


def test_attention_softmax_of_the_fixture_is_not_degenerate():
    """The procedural qkv gain (utils/procedural.py PSA_QKV_GAIN2) gives the default family a softmax that is neither one-hot nor flat on
    the golden images: a one-hot or uniform attention would let a kernel that mixes up q / k / v or the scale pass the f32 golden test.
    (The smooth family, whose BatchNorm scale is 1, keeps a near-flat attention - it pins detection agreement in bf16; the bf16 attention
    kernel itself is tested on sharp softmaxes in tests/test_hip_yolo11.py::test_psa_attention_vs_oracle.)"""
    for family in ("yolov11n",):
        o = Y.DetectionModel("yolov11n.yaml")
        P.apply_procedural_weights(o, family=family)
        o.fuse()
        seen = {}
        attn = o.model[10].m[0].attn
        h = attn.register_forward_hook(lambda mod, i, out: seen.__setitem__("x", i[0]))
        with torch.no_grad():
            o(P.synthetic_images(2))
            mx = attn.probs(seen["x"]).max(-1).values
        h.remove()
        assert float(mx.median()) < 0.5 and float((mx > 0.99).float().mean()) < 0.01, family
        assert float(mx.median()) > 4.0 / 400, family  # at least 4x the uniform weight 1/400 (measured ~7x)


def test_recipe_for_yolo11_leaves_other_families_unchanged():
    """The YOLO11-only recipe entries touch no key another config has (attn.qkv exists only in C2PSA)."""
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    m = DetectionModel("yolov8n.yaml")
    assert not any("attn.qkv" in k for k in m.state_dict())
    assert "yolov8n" not in P.PSA_QKV_GAIN2


def test_grouped_conv_other_than_depthwise_raises():
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.nn.modules.conv import Conv
    c = Conv(8, 16, 3, g=2).eval()
    with pytest.raises(L.UpaError):
        c(torch.zeros(1, 8, 4, 4))


def test_c3k2_never_takes_the_c2f_whole_block_kernels():
    """C3k2 blocks with the outer shapes of the C2f whole-block kernels (yolov11n layers 6, 13, 16, 19) must not reach them: those kernels
    hard-code Bottleneck(c, c, e = 1.0)."""
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    m = DetectionModel("yolov11n.yaml")
    for i in (6, 13, 16, 19):
        blk = m.model[i]
        assert type(blk).__name__ == "C3k2"
        assert blk._form64() or blk._form32up()  # the predicates alone would accept them
        x = torch.zeros(1, blk.cv1.conv.in_channels, 8, 8, dtype=torch.bfloat16)
        assert blk._fused(x, None) is None and blk._pair_cv2(x, None) is None and blk.forward_down(x, None) is None


def test_nonlegacy_detect_rejects_the_fused_class_branch_forms():
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    det = DetectionModel("yolov11n.yaml").model[-1]
    t = torch.zeros(1, 80, 4, 4, dtype=torch.bfloat16)
    assert det._branch_tail_args(t, det.cv3[0][1], det.cv3[0][2], 2) is None
    assert det._levels_grouped([0, 1], [t, t], {}) is False
    assert det._level_stream(0, t, {}) is False
