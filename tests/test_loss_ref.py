"""CPU (-m "not gpu"): the float64 detection-loss reference of tests/loss_ref.py against the oracle run in float64, against
answers known in closed form, and - for every input that tests/test_hip_loss.py hands the kernels - the checks that the input can be
decided by a float32 implementation and still contains what it is there for.  A GPU case that has lost its point fails here."""

import math

import pytest
import torch

from tests import loss_ref as LR

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


def test_loss_ref_equals_the_oracle_in_float64():
    """oracle/loss.py under torch.set_default_dtype(float64) on the base case: items and autograd gradients to 1e-12 relative, the
    assignment exactly (the base case has no zero-metric fill of a top-k, the only part torch.topk leaves open)."""
    i, r = LR.inputs("base"), LR.reference("base")
    items, grads, agt, score = LR.oracle_loss(i.feats, i.gt, i.n_gt, i.strides, i.nc, F64)
    assert items.dtype == F64 and all(g.dtype == F64 for g in grads)
    assert _rel(items, r.items) <= 1e-12
    for g, ref in zip(grads, r.grads):
        assert _rel(g, ref) <= 1e-12
    assert torch.equal(agt, r.assign)
    assert float((score - r.score).abs().max()) <= 1e-12
    for b, c in enumerate(r.claims):  # every single claim is the assignment; every assigned anchor was claimed by some box
        n = c.sum(0)
        assert torch.equal(n > 0, r.assign[b] >= 0)
        one = n == 1
        if c.shape[0]:
            assert torch.equal(c[:, one].long().argmax(0), r.assign[b][one])


@pytest.mark.parametrize("name", ["empty_maxgt1", "empty_maxgt64"])
def test_batch_without_boxes_is_the_plain_bce(name):
    """items = (0, gain_cls * sum softplus(x), 0); class gradient = gain_cls * B * sigmoid(x); box / DFL gradient exactly 0."""
    i, r = LR.inputs(name), LR.reference(name)
    x = torch.cat([f[:, 64:].double().flatten() for f in i.feats])
    want = LR.GAINS[1] * torch.nn.functional.softplus(x).sum()
    assert float(r.items[0]) == 0.0 and float(r.items[2]) == 0.0
    assert abs(float(r.items[1]) - float(want)) <= 1e-12 * float(want)
    for f, g in zip(i.feats, r.grads):
        assert float(g[:, :64].abs().max()) == 0.0
        assert _rel(g[:, 64:], LR.GAINS[1] * i.B * torch.sigmoid(f[:, 64:].double())) <= 1e-12
    assert int((r.assign >= 0).sum()) == 0


def _one_level(boxes, hw=(8, 8), nc=2, key="known"):
    gt, n_gt = LR.pack([boxes], 4)
    return LR.uniform_maps(f"loss:{key}", 1, [hw], nc), gt, n_gt


def test_one_perfectly_predicted_anchor_has_ciou_one():
    """A box around one stride-8 anchor centre, predicted exactly: the one positive has target score = CIoU = 1 within 1e-6."""
    box = (8.0, 8.0, 16.0, 16.0)  # holds the centre (12, 12) only; half a cell to every side
    feats, gt, n_gt = _one_level([[1, *box]])
    LR.set_prediction(feats, (8.0,), 0, 0, 1, 1, box, {1: 6.0})
    r = LR.loss_ref(feats, gt, n_gt, (8.0,), 2)
    assert r.assign[0].tolist().count(0) == 1 and int(r.assign[0, 9]) == 0
    t = float(r.score[0, 9])
    assert abs(t - 1.0) <= 1e-6
    assert abs(float(r.items[0]) / (LR.GAINS[0] * t)) <= 1e-6  # 1 - CIoU of the positive


def test_report_rejects_a_tie_in_the_top_k():
    """Eleven anchors that predict their box exactly and score its class alike: the 10th and 11th metric are equal to rounding."""
    box = (4.0, 4.0, 60.0, 60.0)
    feats, gt, n_gt = _one_level([[0, *box]])
    for n in range(11):
        LR.set_prediction(feats, (8.0,), 0, 0, 1 + n // 4, 1 + n % 4, box, {0: 3.0})
    rep = LR.loss_ref(feats, gt, n_gt, (8.0,), 2).report
    assert rep["topk_gap"] < 1e-9
    assert any("alignment metric" in s for s in LR.undecidable(rep))
    feats[0][0, 64, 1 + 10 // 4, 1 + 10 % 4] = -3.0  # the eleventh now scores the class lower: decided
    assert LR.loss_ref(feats, gt, n_gt, (8.0,), 2).report["topk_gap"] > 0.5


def test_report_rejects_a_target_score_at_the_slide_jump():
    """Two exact anchors of one box; the second one's class logit is chosen so that its target score is 0.4."""
    box = (4.0, 4.0, 28.0, 28.0)
    feats, gt, n_gt = _one_level([[0, *box]], hw=(4, 4))
    s1 = 1.0 / (1.0 + math.exp(-5.0))
    s2 = 0.16 * s1  # target score = sqrt(s2 / s1) * overlap, overlap = 1
    LR.set_prediction(feats, (8.0,), 0, 0, 1, 1, box, {0: 5.0})
    LR.set_prediction(feats, (8.0,), 0, 0, 2, 2, box, {0: math.log(s2 / (1 - s2))})
    rep = LR.loss_ref(feats, gt, n_gt, (8.0,), 2).report
    assert rep["slide_gap"] < 1e-6
    assert any("from 0.4" in s for s in LR.undecidable(rep))


def test_report_rejects_an_undecided_resolve_and_a_coordinate_on_its_target():
    rep = dict(LR.reference("base").report)
    assert LR.undecidable(rep) == []
    for key, word in (("multi_gap", "multiply-claimed"), ("coord_gap", "from its target"), ("dmin", "box edge")):
        assert any(word in s for s in LR.undecidable(dict(rep, **{key: 1e-6})))
    assert any("zero-metric" in s for s in LR.undecidable(dict(rep, zero_fill=1)))


def test_every_gpu_case_names_an_input():
    assert len({c.name for c in LR.CASES}) == len(LR.CASES)
    assert {c.source for c in LR.CASES if c.source} <= set(LR.INPUT_NAMES)
    assert all(c.layout is None or c.layout[1] + 64 + LR.inputs(c.name).nc <= c.layout[0] for c in LR.CASES)


@pytest.mark.parametrize("name", LR.INPUT_NAMES)
def test_gpu_case_input_is_decidable_and_holds_its_point(name):
    case, i, r = LR.CASE[name], LR.inputs(name), LR.reference(name)
    rep = r.report
    assert LR.undecidable(rep) == [], name
    for key in case.contains:
        assert rep[key] >= 1, f"{name} no longer contains {key}: {case.pins}"
    if name == "on_centre":
        assert LR.on_centre_strides(rep, i.hw, i.strides) == [8.0, 16.0, 32.0]
        for b, a in rep["on_centre"]:  # an anchor on a box's edge is outside that box
            px = (LR.anchors(i.hw, i.strides)[0] * LR.anchors(i.hw, i.strides)[1][:, None])[a]
            rows = i.gt[b, :int(i.n_gt[b])].double()
            edge = torch.cat((px - rows[:, 1:3], rows[:, 3:5] - px), 1).amin(1) == 0
            assert bool(edge.any()) and not bool(r.claims[b][edge, a].any())
        # the marked edge anchors are background, and would be their rows' best positives if the edge counted as inside
        a0 = [0, 240, 300]
        marked = [(a0[l] + y * i.hw[l][1] + x, g) for l, y, x, g in LR.ON_EDGE]
        assert all((0, a) in rep["on_centre"] and int(r.assign[0, a]) == -1 for a, _ in marked)
        grown = i.gt.clone()
        grown[0, :3, 1:3] -= 1e-3
        wide = LR.loss_ref(i.feats, grown, i.n_gt, i.strides, i.nc)
        assert all(int(wide.assign[0, a]) == g and float(wide.score[0, a]) > 0.9 for a, g in marked)
    if name.startswith("empty"):
        assert rep["images_with_boxes"] == 0
    if name == "maxgt192_full":
        assert int(i.n_gt.max()) == i.max_gt == 192
    if name == "maxgt1024":
        assert i.max_gt == 1024 and int(i.n_gt.max()) == 3
    if name == "a8400":
        assert r.assign.shape[1] == 8400
    # the float32 oracle takes the float64 decisions
    _, _, agt32, score32 = LR.oracle32(name)
    assert torch.equal(LR.effective(agt32, score32), LR.effective(r.assign, r.score)), name
    assert float((score32.double() - r.score).abs().max()) <= 1e-4


def test_refusals_stand_before_the_first_launch():
    """The anchor-count, LDS-row and workspace checks of upa_detection_loss_scaled come before its first launch."""
    assert LR.refusals_precede_launches()
