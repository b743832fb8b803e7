"""CPU (-m "not gpu"): the classification checker tests/classify_oracle.py reproduces the reference's per-op and end-to-end goldens
(tests/golden/ops_classify.npz, e2e_yolov*n-cls*.npz, tools/gen_golden_classify.py); the goldens themselves are decidable (separated
top-6, no saturated row); and the float64 references of tests/classify_ref.py are pinned against loops, an f32 emulation and two
negative controls."""

import numpy as np
import pytest
import torch

from tests import classify_oracle as C
from tests import classify_ref as CF
from tests import conv_ref as CR
from ultralytics_pro_amd.utils import procedural as P

E2E = ["yolov8n-cls", "yolov8n-cls_smooth", "yolov11n-cls", "yolov11n-cls_smooth"]


@pytest.mark.parametrize("case", C.head_cases(), ids=[c[0] for c in C.head_cases()])
def test_oracle_classify_head(case, golden_dir):
    g = np.load(golden_dir / "ops_classify.npz")
    m, x = C.head_case(case)
    assert np.array_equal(x.numpy(), g[f"{case[0]}_x"])
    with torch.no_grad():
        p, z = m(x)
    assert p.shape == (case[4], case[3])
    assert float((z - torch.from_numpy(g[f"{case[0]}_logits"])).abs().max()) <= 1e-5
    assert float((p - torch.from_numpy(g[f"{case[0]}_probs"])).abs().max()) <= 1e-5
    m.export = True
    with torch.no_grad():
        assert torch.equal(m(x), p)


@pytest.mark.parametrize("name", E2E)
def test_oracle_e2e(name, golden_dir):
    g = np.load(golden_dir / f"e2e_{name}.npz")
    base, smooth = name.replace("_smooth", ""), name.endswith("_smooth")
    o = C.ClassificationModel(base + ".yaml")
    P.apply_procedural_weights(o, family=("smooth:" if smooth else "") + base)
    o.fuse()
    with torch.no_grad():
        p, z = o(P.synthetic_images(2, h=224, w=224))
    # 1e-3 as the other end-to-end oracle checks: the CPU's summation order depends on its thread count
    assert float(np.abs(z.numpy() - g["logits"]).max()) <= 1e-3
    assert float(np.abs(p.numpy() - g["probs"]).max()) <= 1e-3
    assert np.array_equal(z.argsort(1, descending=True)[:, :5].numpy(), g["top5"])


@pytest.mark.parametrize("name", E2E)
def test_e2e_goldens_are_decidable(name, golden_dir):
    """On the reference's own outputs: ranks 1-6 of every row pairwise at least 1e-2 apart (a top-5 list is then a property of the
    model, not of the last bits) and no saturated row (a probability comparison would be vacuous)."""
    g = np.load(golden_dir / f"e2e_{name}.npz")
    z = np.sort(g["logits"], axis=1)[:, ::-1][:, :6]
    assert float((z[:, :-1] - z[:, 1:]).min()) >= 1e-2
    assert float(g["probs"].max()) < 0.999
    assert np.array_equal(np.argsort(-g["logits"], axis=1, kind="stable")[:, :5], g["top5"])
    assert np.abs(g["probs"].sum(1) - 1).max() <= 1e-5


def test_classify_metrics_match_reference(golden_dir):
    from ultralytics_pro_amd.utils import metrics as M
    g = np.load(golden_dir / "ops_classify.npz")
    pred, targets = C.metrics_case()
    assert np.array_equal(torch.cat(pred).numpy(), g["metrics_pred"]) and np.array_equal(torch.cat(targets).numpy(), g["metrics_targets"])
    for met in (C.ClassifyMetrics(), M.ClassifyMetrics()):
        met.process(targets, pred)
        assert [met.top1, met.top5, met.fitness] == list(g["metrics_top1_top5_fitness"])
        assert list(met.results_dict) == list(g["metrics_keys"]) == ["metrics/accuracy_top1", "metrics/accuracy_top5", "fitness"]
    assert (met.top1, met.top5) == (np.float32(3 / 7), np.float32(5 / 7))
    assert np.array_equal(M.process_cls_preds(pred, targets, 10), g["metrics_confusion"])
    assert M.ClassifyMetrics().summary() == [{"top1_acc": 0, "top5_acc": 0}]


# ---- tests/classify_ref.py ---------------------------------------------------------------------------------------------------------

def test_pool_ref_equals_loops_on_a_hand_case():
    """2 pixels, 3 channels, 2 outputs: by hand v = b + x . w per pixel, the mean of SiLU(v)."""
    x = torch.tensor([[[[1.0, -2.0]], [[0.5, 0.25]], [[-1.0, 3.0]]]])  # (1, 3, 1, 2)
    w = torch.tensor([[1.0, 2.0, -1.0], [0.5, -0.5, 0.25]])
    b = torch.tensor([0.5, -1.0])
    for act in (CR.ACT_NONE, CR.ACT_SILU):
        ref, bound = CF.pool_ref(x, w, b, act)
        assert float((ref - CF.pool_loop(x, w, b, act)).abs().max()) <= 1e-15
        assert bool((bound > 0).all())
    v = torch.tensor([[3.5, -4.0], [-1.0, -1.375]], dtype=torch.float64)  # [channel][pixel]
    assert torch.equal(CF.pool_ref(x, w, b, CR.ACT_NONE)[0][0], v.mean(1))
    silu = v / (1 + torch.exp(-v))
    assert float((CF.pool_ref(x, w, b, CR.ACT_SILU)[0][0] - silu.mean(1)).abs().max()) <= 1e-15


@pytest.mark.parametrize("act", [CR.ACT_NONE, CR.ACT_SILU])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_pool_bound_holds_f32_orders_and_rejects_padded_row_bugs(act, dtype):
    n, cin, h, w, cout = 2, 64, 7, 7, 24
    x, wt, b, _ = CR.conv_family("uniform", n, cin, h, w, cout, 1, dtype, seed=3)
    wt = wt.reshape(cout, cin)
    ref, bound = CF.pool_ref(x, wt, b, act)
    for order in ("forward", "reverse", "pairwise"):
        y = CF.pool_f32_emulation(x, wt, b, act, order).to(torch.float64)
        assert bool(((y - ref).abs() <= bound).all()), order
    # 15 padded rows (49 of 64) that count with act(bias), or that count in the divisor: both far outside
    bad = CF.pool_f32_emulation(x, wt, b, act, pad_rows=15, pad_mode="act_bias").to(torch.float64)
    assert float(((bad - ref).abs() > bound).float().mean()) > 0.9
    bad = CF.pool_f32_emulation(x, wt, b, act, pad_rows=15, pad_mode="count").to(torch.float64)
    assert float(((bad - ref).abs() > bound).float().mean()) > 0.9


def test_softmax_and_topk_refs():
    z = torch.tensor([[0.0, 1.0, 1.0, -float("inf"), -0.0, 2.0], [3.0, 3.0, 3.0, 3.0, 3.0, 3.0]])
    ref, bound, tol = CF.softmax_ref(z)
    assert float((ref.sum(1) - 1).abs().max()) <= 1e-15 and float(ref[0, 3]) == 0.0
    assert float((ref - torch.softmax(z.double(), 1)).abs().max()) <= 1e-15
    assert float((torch.softmax(z, 1).double() - ref).abs().max()) <= float(bound.max()) and tol == 14 * 2.0 ** -24
    assert CF.topk_ref(z, 5).tolist() == [[5, 1, 2, 0, 4], [0, 1, 2, 3, 4]]  # ties (and -0 == +0) to the lower index
