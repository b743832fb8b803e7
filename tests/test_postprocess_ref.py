"""CPU: the post-processing reference tests/postprocess_ref.py pinned three ways - against oracle/nms.py on the real-reference goldens
(tests/golden/nms_cases.npz), against the oracle on every built scene, and against the TP matrices of map_yolov8n.npz - with every
scene's decidability assertion run here, before a scene reaches a GPU.

The last part breaks the rules on purpose: a CPU model of the greedy kernel's structure (chunks of 64, the kept list dealt to 16 waves,
the suppression-column fixed point, the `room` cut) equals the reference on every scene, and each single fault in it - or in the tie
order, or in the matching's claim rule - makes the scene built for that structure fail."""

import json

import numpy as np
import pytest
import torch

from oracle import nms as onms
from tests import postprocess_ref as PR

NAMES = [s.name for s in PR.scenes()]


def _same(res, out, keep, what):
    assert len(res) == len(out)
    for b, (rows, k, _, _) in enumerate(res):
        assert rows.shape == tuple(out[b].shape), (what, b, rows.shape, tuple(out[b].shape))
        assert np.array_equal(rows, out[b].numpy()), (what, b)
        assert np.array_equal(k, keep[b].numpy()), (what, b)


def test_nms_ref_equals_reference_goldens(golden_dir):
    g = np.load(golden_dir / "nms_cases.npz")
    names = sorted(k[:-5] for k in g.files if k.endswith("_pred"))
    assert len(names) >= 19
    for name in names:
        kw = json.loads(str(g[name + "_kw"]))
        res = PR.nms_ref(g[name + "_pred"], **kw)
        assert [r[0].shape[0] for r in res] == list(g[name + "_n"]), name
        assert np.array_equal(np.concatenate([r[0] for r in res]), g[name + "_out"]), name
        assert np.array_equal(np.concatenate([r[1] for r in res]), g[name + "_keep"]), name
        out, keep = onms.non_max_suppression(torch.from_numpy(g[name + "_pred"]), return_idxs=True, **kw)
        _same(res, out, keep, name)


@pytest.mark.parametrize("name", NAMES)
def test_scene_is_decidable_and_equals_oracle(name):
    s = PR.scene(name)
    res = s.ref()  # asserts decidability and the count the scene was built for
    out, keep = onms.non_max_suppression(torch.from_numpy(s.pred), return_idxs=True, **s.kw)
    _same(res, out, keep, name)
    rows, counts, k = s.fixed()
    for b in range(len(res)):
        assert not rows[b, counts[b]:].any() and (k[b, counts[b]:] == -1).all()


def test_zero_area_boxes_survive_as_in_the_reference():
    """Three zero-area boxes of one class and an ordinary box: the reference keeps all four (a zero-area kept box intersects nothing, so
    TorchNMS.nms leaves its suppression step early); 0 / 0 = NaN arithmetic without that rule would drop the second point."""
    s = PR.scene("degenerate_three_points-sl")
    assert [r[0].shape[0] for r in s.ref()] == [4]
    assert onms.non_max_suppression(torch.from_numpy(s.pred), **s.kw)[0].shape[0] == 4


def test_match_ref_reproduces_reference_tp(golden_dir):
    G = np.load(golden_dir / "map_yolov8n.npz")
    for i in range(4):
        gt = np.concatenate([G[f"gt_cls{i}"][:, None], G[f"gt_boxes{i}"]], 1)
        tp, i32, i64 = PR.match_ref(G[f"det{i}"], gt)
        assert np.array_equal(tp, G[f"tp{i}"]), i
        assert np.abs(i32 - i64).max() <= 2e-6


@pytest.mark.parametrize("max_det", [300, 600])
def test_match_scenes_are_decidable(max_det):
    for m in (PR.match_scene(max_det), PR.match_scene(max_det, True), PR.match_scene_clamped(max_det)):
        tp = m.ref()
        n0 = min(int(m.counts[0]), max_det)
        assert tp[0, :n0].any() and not tp[0, n0:].any()
    m, u = PR.match_scene(max_det).ref(), PR.match_scene(max_det, True).ref()
    # the contest over label 0: detection 3 holds the low thresholds, 7 (higher IoU) the ones only it reaches, 11 none; the same over 256
    assert m[0, [3, 7, 11]].tolist() == [[1, 1] + [0] * 8, [0, 0, 1, 1, 1, 1, 1, 0, 0, 0], [0] * 10]
    assert m[0, [250, 260]].tolist() == [[1, 1] + [0] * 8, [0, 0] + [1] * 7 + [0]]
    if max_det == 600:
        assert m[0, [510, 515]].tolist() == [[1, 1] + [0] * 8, [0, 0] + [1] * 7 + [0]]
    # IoU on the threshold counts; one ulp below does not
    assert m[0, 40:44].sum(1).tolist() == [1, 4, 10, 5] and u[0, 40:44].sum(1).tolist() == [1, 3, 10, 4]


# ---- the rules, broken on purpose ---------------------------------------------------------------------------------------------------


def greedy_model(ob, thr, max_det, rounds_cap=None, strict=False, no_room=False, skip_wave=None, stage_local=False):
    """The greedy kernel's structure on the class-offset boxes in score order (f32): chunks of 64 in stages of 1024; a chunk is tested
    against the kept list (dealt to 16 waves), then resolved - serial walk below 8 alive candidates, else the fixed point
    kept = alive & ~(some kept j in my column) - and cut to the room left under max_det.  The keyword arguments each break one rule."""
    ob = np.asarray(ob, PR.F32)
    area = (ob[:, 2] - ob[:, 0]) * (ob[:, 3] - ob[:, 1])
    thr = PR.F32(thr)

    def sup(k, i):  # (len(k), len(i)) bool: kept k suppresses candidate i
        w = np.maximum(np.minimum(ob[k, 2][:, None], ob[i, 2][None]) - np.maximum(ob[k, 0][:, None], ob[i, 0][None]), 0)
        h = np.maximum(np.minimum(ob[k, 3][:, None], ob[i, 3][None]) - np.maximum(ob[k, 1][:, None], ob[i, 1][None]), 0)
        inter = w * h
        with np.errstate(invalid="ignore", divide="ignore"):
            iou = inter / (area[k][:, None] + area[i][None] - inter)
        return (inter != 0) & ~((iou < thr) if strict else (iou <= thr))

    kept = []
    for base in range(0, ob.shape[0], 64):
        if len(kept) >= max_det:
            break
        idx = np.arange(base, min(base + 64, ob.shape[0]))
        k = np.array([v for q, v in enumerate(kept) if (skip_wave is None or q % 16 != skip_wave)
                      and (not stage_local or v // 1024 == base // 1024)], np.int64)
        alive = idx[~sup(k, idx).any(0)]
        room = max_det - len(kept)
        if alive.shape[0] >= 8:
            m = np.triu(sup(alive, alive), 1)  # m[j, i]: j < i and j would suppress i
            cur, rounds = np.ones(alive.shape[0], bool), 0
            while True:
                nxt = ~(m & cur[:, None]).any(0)
                rounds += 1
                done = np.array_equal(nxt, cur) or (rounds_cap is not None and rounds >= rounds_cap)
                cur = nxt
                if done:
                    break
            new = alive[cur]
        else:
            new = []
            for i in alive:
                if not new or not sup(np.array(new), np.array([i])).any():
                    new.append(int(i))
        kept += [int(v) for v in (new if no_room else new[:room])]
    return kept


def _model_keep(s, **fault):
    tie_last = fault.pop("tie_last", False)
    out = []
    for cd in PR.candidates(s.pred, tie_last=tie_last, **s.kw):
        out.append(cd["anchor"][greedy_model(cd["ob32"], s.kw.get("iou_thres", 0.45), s.kw.get("max_det", 300), **fault)])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_kernel_structure_model_equals_reference(name):
    s = PR.scene(name)
    for got, (_, keep, _, _) in zip(_model_keep(s), s.ref()):
        assert np.array_equal(got, keep)


@pytest.mark.parametrize("fault,name", [
    (dict(rounds_cap=4), "chain70_period2-sl"), (dict(rounds_cap=4), "chain200_from60-sl"), (dict(rounds_cap=4), "chain200_period3-ml"),
    (dict(rounds_cap=4), "alive9-sl"),
    (dict(strict=True), "iou_eq_thr_third_c0"), (dict(strict=True), "iou_eq_thr_25_175_c2"),
    (dict(no_room=True), "cut_serial_first-sl"), (dict(no_room=True), "cut_cols_first-sl"), (dict(no_room=True), "cut_serial_second-sl"),
    (dict(no_room=True), "cut_cols_second-sl"), (dict(no_room=True), "iso1100_maxdet65"),
    (dict(skip_wave=5), "slices64-sl"), (dict(skip_wave=15), "slices40-sl"), (dict(skip_wave=14), "alive8-sl"),
    (dict(stage_local=True), "stage1025-sl"), (dict(stage_local=True), "stage2049-ml"),
    (dict(tie_last=True), "maxnms_ties-sl"), (dict(tie_last=True), "maxnms_pow2-ml"), (dict(tie_last=True), "tie_anchors-sl"),
])
def test_a_broken_rule_fails_its_scene(fault, name):
    s = PR.scene(name)
    assert any(not np.array_equal(got, keep) for got, (_, keep, _, _) in zip(_model_keep(s, **dict(fault)), s.ref())), \
        f"{name} does not notice {fault}"


def _claim_model(det, gt, iouv, pick=min, tie_low=False):
    """The matching kernel's claim rule: a detection's best same-class label (threshold-independent); per (label, threshold) the
    smallest detection index among the detections whose best label it is and whose IoU reaches the threshold."""
    n = det.shape[0]
    tp = np.zeros((n, len(iouv)), bool)
    if n == 0 or gt.shape[0] == 0:
        return tp
    iou = PR.box_iou_ref(gt[:, 1:], det[:, :4], dtype=PR.F32) * (gt[:, 0][:, None] == det[:, 5][None])
    best = iou.argmax(0)
    for k, t in enumerate(iouv):
        for l in range(gt.shape[0]):
            c = [d for d in range(n) if best[d] == l and iou[l, d] > 0 and iou[l, d] >= t]
            if c:
                tp[pick(c), k] = True
    return tp


@pytest.mark.parametrize("max_det", [300, 600])
def test_claim_rule_and_its_breakage(max_det):
    m = PR.match_scene(max_det)
    ref, n = m.ref(), int(m.counts[0])
    assert np.array_equal(_claim_model(m.det[0, :n], m.gt[0, :int(m.ngt[0])], m.iouv), ref[0, :n].astype(bool))
    wrong = _claim_model(m.det[0, :n], m.gt[0, :int(m.ngt[0])], m.iouv, pick=max)
    rows = [250, 260] + ([510, 515] if max_det == 600 else [])
    assert all((wrong[r] != ref[0, r].astype(bool)).any() for r in rows)
    # rounds of 256 that forget the claims of the rounds before them: the later detection of a split contest takes every threshold it reaches
    assert ref[0, 260, :2].tolist() == [0, 0] and ref[0, 256, :2].tolist() == [0, 0]
