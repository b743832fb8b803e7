"""CPU: what training YOLO11 detection rests on without a GPU.  The oracle (tests/yolo11_oracle.DetectionModel stepped by
oracle.train.train_step) reproduces the imported reference's record of whole yolov11n training steps (tests/golden/train_yolov11n.npz,
tools/gen_golden_detect_train11.py) with the tolerances of tests/test_classify_train11_golden.py; `DetectionTrainer`'s refusals - the
default one and the new ones behind `yolo11=True` - are raised before anything touches a device; the two fused depthwise entries are
declared in include/upa.h and exported by the built library."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import train as otr
from tests import yolo11_oracle as Y
from ultralytics_pro_amd.utils import procedural as P

ROOT = Path(__file__).resolve().parents[1]
DW = ["model.23.cv3.0.0.0", "model.23.cv3.0.1.0"]
RAW_KEYS = ["model.23.cv3.0.2.bias"] + [f"{d}.{p}" for d in DW for p in ("conv.weight", "bn.weight", "bn.bias")]
NEW_SYMBOLS = ["upa_dwconv2d_bn_act_fwd", "upa_dwconv_bn_act_bwd"]


def test_oracle_step_matches_reference_golden_yolov11n(golden_dir):
    G = np.load(golden_dir / "train_yolov11n.npz")
    bs, imgsz, steps = (int(v) for v in G["a_shape"])
    assert (bs, imgsz, steps) == (4, 320, 2) and float(G["a_oracle_vs_ref"][0]) <= 1e-6
    m = Y.DetectionModel("yolov11n.yaml")
    P.apply_procedural_weights(m, family="yolov11n")
    state = otr.TrainState(m)
    keys = [str(k) for k in G["a_param_keys"]]
    named = dict(m.named_parameters())
    assert "model.23.dfl.conv.weight" in named and "model.23.dfl.conv.weight" not in keys  # no gradient in the reference's record ...
    assert set(RAW_KEYS) <= set(keys)
    for step in range(steps):
        x = P.synthetic_images(bs, h=imgsz, w=imgsz, seed=step)
        lab = P.synthetic_labels(bs, seed=step)
        items, norm = otr.train_step(m, state, {"img": x, **lab})
        assert named["model.23.dfl.conv.weight"].grad is None  # ... and none in the oracle
        np.testing.assert_allclose(items.detach().numpy(), G[f"a_loss_items_{step}"], rtol=1e-4)
        np.testing.assert_allclose(norm, float(G[f"a_grad_norm_{step}"][0]), rtol=1e-4)
        l2 = np.array([float(named[k].grad.double().norm()) for k in keys])
        np.testing.assert_allclose(l2, G[f"a_grad_l2_{step}"], rtol=1e-3, atol=1e-6 * float(G[f"a_grad_l2_{step}"].max()))
        for k in RAW_KEYS:
            want = G[f"a_grad[{k}]_{step}"]
            np.testing.assert_allclose(named[k].grad.numpy(), want, rtol=1e-3, atol=1e-5 * float(np.abs(want).max()), err_msg=k)
        sd = m.state_dict()
        np.testing.assert_allclose(sd["model.0.conv.weight"].numpy(), G[f"a_w_stem_{step}"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(sd["model.2.cv1.bn.running_var"].numpy(), G[f"a_bn_rv_{step}"], rtol=1e-4)
        fk = [str(k) for k in G["a_state_keys"]]
        np.testing.assert_allclose(np.array([float(state.ema[k].double().sum()) for k in fk]), G[f"a_ema_sum_{step}"], rtol=1e-4, atol=1e-3)


def _model(nc):
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    return DetectionModel("yolov11n.yaml", nc=nc)


def test_trainer_refuses_a_class_count_the_depthwise_kernels_cannot_take():
    """nc = 81 makes the class branch c3 = max(ch[0], min(nc, 100)) = 81 channels wide: not a multiple of 8.  The refusal names the layer
    and nc, and comes before the model is moved to a device (this test has none)."""
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer
    m = _model(81)
    with pytest.raises(UpaError, match=r"model\.23\.cv3\.0\.1\.0.*multiples of 8.*nc = 81"):
        DetectionTrainer(m, dtype=torch.float32, device="cuda:0", yolo11=True)
    assert all(p.device.type == "cpu" for p in m.parameters())


def test_trainer_refuses_yolo11_detection_unless_asked():
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer
    m = _model(80)
    with pytest.raises(UpaError, match="Detect.*no training path.*yolo11=True"):
        DetectionTrainer(m, dtype=torch.float32, device="cuda:0")
    assert all(p.device.type == "cpu" for p in m.parameters())


@pytest.mark.parametrize("symbol", NEW_SYMBOLS)
def test_fused_depthwise_entries_are_declared_and_exported(symbol):
    from ultralytics_pro_amd import _lib as L
    header = (ROOT / "include" / "upa.h").read_text()
    assert re.search(rf"^int {symbol}\(", header, re.M) and re.search(rf"^size_t {symbol}_workspace_bytes\(", header, re.M)
    assert "head.py:98-110" in header and "conv.py:411-425" in header
    assert symbol in L.PROTOTYPES and symbol + "_workspace_bytes" in L.PROTOTYPES
    handle = ctypes.CDLL(str(L.LIB_PATH))  # (a plain dlopen: no device is touched)
    assert getattr(handle, symbol) is not None and getattr(handle, symbol + "_workspace_bytes") is not None
    q = getattr(handle, symbol + "_workspace_bytes")
    q.restype, q.argtypes = ctypes.c_size_t, [ctypes.c_int] * 4
    rows = 16 * 10  # yolov11n level 0 at bs 16, 640 x 640: 16 images x 10 bands of 8 rows; sized by the shape, not capped at 128
    assert q(16, 80, 80, 80) == rows * 80 * (2 if symbol.endswith("fwd") else 9) * 4 and q(0, 80, 80, 80) == 0
