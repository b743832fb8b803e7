"""-m gpu: the trainers' Adam / AdamW / auto optimizer (engine/trainer.py `optimizer=`, upa_adam_ema) on yolov8n-cls at the AdamW
golden's shapes (nc 10, bs 4, 64 x 64: case `a` of tests/classify_train_oracle.GOLDEN_CASES, the smallest the model builds at).

The plumbing check holds every element of P, M (exp_avg), V (exp_avg_sq) and E (EMA) after `optimizer_step` to tests/adam_ref.py
applied, group by group, to the DEVICE's own gradients and prior state, within the kernel test's bound (`adam_ref.adam_bounds` from
a zero carried bound): it pins the group offsets, the lr / weight decay of each group, the step count and the EMA decay, and does not
depend on how a near-zero gradient rounds - which under Adam decides the sign of a first update and is pinned by the gradient tests."""

import functools
import math

import numpy as np
import pytest
import torch

from tests import adam_ref as AR
from tests import classify_train_oracle as T
from tests import kernel_check as KC
from tests import train_ref as TR
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _trainer(nc=10, dtype=F32, **kw):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine.trainer import ClassificationTrainer
    from ultralytics_pro_amd.nn.tasks import ClassificationModel
    m = ClassificationModel("yolov8n-cls.yaml", nc=nc)
    P.apply_procedural_weights(m, family="yolov8n-cls")
    return m, ClassificationTrainer(m, dtype=dtype, device=DEV, **kw)


@functools.lru_cache(maxsize=None)
def _batch(step):
    from tests.hip_utils import DEV
    b = T.golden_batch("a", step)
    return b["img"].to(DEV), {"cls": b["cls"]}


def _state(tr):
    torch.cuda.synchronize()
    return {k: getattr(tr, k).cpu().clone() for k in ("G", "P", "M", "V", "E")}


def _check_optimizer_step(tr, t, what, report, scale=None, lrs=None, weight_decay=None):
    """optimizer_step() from the gradients in the flat buffer; every group against adam_ref from the device's own state.  t: the count
    this step must leave."""
    h = tr.hyp
    s0 = _state(tr)
    tr.optimizer_step(lrs=lrs, weight_decay=weight_decay)
    s1 = _state(tr)
    ss = float(tr.sumsq.cpu()[0])
    assert math.isfinite(ss) and tr.opt_step == t, (ss, tr.opt_step, t)
    d = TR.f32(h["ema_decay"] * (1 - math.exp(-tr.updates / h["ema_tau"])))
    lrs = [h["lr"]] * 3 if lrs is None else lrs
    assert [bool(wd) for _, _, wd in tr.groups] == [False, True, False] and all(n > 0 for _, n, _ in tr.groups)
    for gi, (start, n, wd) in enumerate(tr.groups):
        if wd and weight_decay is not None:
            wd = weight_decay
        sl = slice(start, start + n)
        outs, terms = AR.adam_ref(s0["P"][sl], s0["G"][sl], s0["M"][sl], s0["V"][sl], s0["E"][sl], ss, h["max_norm"], TR.f32(lrs[gi]),
                                  TR.f32(h["momentum"]), TR.f32(h["beta2"]), TR.f32(h["adam_eps"]), TR.f32(wd),
                                  tr.optimizer_name == "AdamW", t, d, 1, scale)
        em, ev, ep, ee = AR.adam_bounds(terms, AR.zeros(n))
        pn, gn, mn, vn, en = outs
        KC.check_bound(s1["M"][sl].double(), mn, em + 1e-300, f"{what} group {gi} exp_avg", report)
        KC.check_bound(s1["V"][sl].double(), vn, ev + 1e-300, f"{what} group {gi} exp_avg_sq", report)
        KC.check_bound(s1["P"][sl].double(), pn, ep + 1e-300, f"{what} group {gi} p", report)
        KC.check_bound(s1["E"][sl].double(), en, ee + 1e-300, f"{what} group {gi} ema", report)
    assert float(s1["G"].abs().max()) == 0.0, what + ": the step zeroes the gradients"
    assert not torch.equal(s1["P"], s0["P"])


@KC.stop_after_fault
def test_adamw_steps_follow_adam_ref_group_by_group(golden_dir):
    """ClassificationTrainer(optimizer="AdamW"), f32: three steps.  Step-0 loss and gradient norm agree with the AdamW golden of the
    imported reference at the tolerances of test_training_step_matches_reference_golden (loss 2e-3, norm 3e-3 relative).
    Measured on MI355X: loss 10.034763 (reference 10.034786), gradient norm 1418.7076 (1418.7062); worst error / bound 0.98 (a
    parameter of the norm-weight group: the half ulp of its final subtraction leads the bound)."""
    G = np.load(golden_dir / "train_yolov8n-cls_adamw.npz")
    lr = float(G["hyp"][0])
    m, tr = _trainer(hyp=dict(lr=lr), optimizer="adamw")
    assert tr.optimizer_name == "AdamW" and tr.opt_step == 0 and tr.V is not None
    st = tr.optimizer_state()
    assert st["exp_avg"] is tr.M and st["exp_avg_sq"] is tr.V and st["step"] == 0
    report = []
    for step in range(3):
        x, lab = _batch(step)
        items = tr.forward_backward(x, lab)
        norm = tr.grad_norm()
        if step == 0:
            ref_loss, ref_norm = G["loss_0"], float(G["grad_norm_0"][0])
            print(f"step 0: loss {float(items[0]):.6f} (ref {float(ref_loss[0]):.6f}) |grad| {norm:.4f} (ref {ref_norm:.4f})")
            np.testing.assert_allclose(items.cpu().numpy(), ref_loss, rtol=2e-3)
            assert abs(norm - ref_norm) <= 3e-3 * ref_norm
        _check_optimizer_step(tr, step + 1, f"AdamW step {step}", report)
    KC.print_report(report, "AdamW trainer", "comparisons")
    assert tr.optimizer_state()["step"] == 3


@KC.stop_after_fault
def test_graph_replay_equals_eager_steps():
    """After one eager step and compile(), three replays of the single graph (forward + backward + step advance + optimizer) are
    bit-identical to three eager steps from the same state, and the device-side count reads 4: every replay saw a new t."""
    runs = []
    for mode in ("eager", "compiled"):
        m, tr = _trainer(dtype=BF16, optimizer="AdamW", hyp=dict(lr=0.000714))
        losses = [tr.step(*_batch(0)).cpu().clone()]
        if mode == "compiled":
            tr.compile(*_batch(0), warm_steps=0)
            assert len(tr._graphs) == 1
            torch.cuda.synchronize()
            assert tr.opt_step == 1, "the capture itself must not advance the count"
        for s in (1, 0, 1):
            losses.append(tr.step(*_batch(s)).cpu().clone())
        torch.cuda.synchronize()
        runs.append((torch.cat(losses), tr.P.cpu().clone(), tr.M.cpu().clone(), tr.V.cpu().clone(), tr.E.cpu().clone()))
        assert tr.opt_step == 4 and tr.updates == 4
    for a, b in zip(*runs):
        assert KC.same_bits(a, b)
    assert bool(torch.isfinite(runs[0][0]).all()) and bool(torch.isfinite(runs[0][1]).all())


@KC.stop_after_fault
def test_amp_overflow_skips_the_step_and_keeps_the_count():
    """amp_scaler=True: with the loss scale set to 2**127 the scaled gradients overflow float32 (their largest unscaled element is
    above 2), so the step is skipped - P, M, V bit-identical, the count not advanced, the EMA still moving, the gradients zeroed.  The
    following step, with the scale set back, matches adam_ref with the un-advanced t."""
    m, tr = _trainer(amp_scaler=True, optimizer="AdamW", hyp=dict(lr=0.000714))
    report = []
    tr.forward_backward(*_batch(0))
    _check_optimizer_step(tr, 1, "scaled step 0", report, scale=65536.0)
    tr.scaler.state.copy_(torch.tensor([2.0 ** 127, 0.0, 0.0, 0.0]))
    tr.forward_backward(*_batch(1))
    s0 = _state(tr)
    assert not bool(torch.isfinite(s0["G"]).all()), "the forced scale did not overflow the gradients"
    tr.optimizer_step()
    s1 = _state(tr)
    assert all(KC.same_bits(s1[k], s0[k]) for k in ("P", "M", "V")) and tr.opt_step == 1
    assert not torch.equal(s1["E"], s0["E"]) and float(s1["G"].abs().max()) == 0.0 and tr.scaler.found_inf()
    tr.scaler.state.copy_(torch.tensor([65536.0, 0.0, 0.0, 0.0]))
    tr.forward_backward(*_batch(1))
    _check_optimizer_step(tr, 2, "the step after the skipped one", report, scale=65536.0)
    KC.print_report(report, "AdamW under the GradScaler", "comparisons")


@KC.stop_after_fault
def test_auto_schedule_dispatch_and_refusals():
    """optimizer="auto": AdamW with the recorded lr for 100 iterations, the SGD path above 10 000; under set_schedule the bias group's lr
    starts from 0 (whatever warmup_bias_lr says) and beta1 stays 0.9 through warm-up, where SGD's momentum starts from 0.8.  Other
    names and auto without iterations are refused; SGD (named or by default) allocates no V."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.engine.trainer import ClassificationTrainer
    from ultralytics_pro_amd.nn.tasks import ClassificationModel
    m, tr = _trainer(optimizer="auto", iterations=100, hyp=dict(lr=0.5, momentum=0.5))
    assert tr.optimizer_name == "AdamW" and tr.hyp["lr"] == AR.auto_rule(10, 100)[1] == 0.000714 and tr.hyp["momentum"] == 0.9
    tr.set_schedule(batches_per_epoch=10, global_batch=4, warmup_bias_lr=0.1)
    nw = 100
    for ni in (0, 1, 50, nw, nw + 1):
        acc, lrs, mom, wd = tr.schedule_at(ni, 4)
        assert mom == 0.9, (ni, mom)
        if ni == 0:
            assert lrs == [0.0, 0.0, 0.0]
        elif ni <= nw:
            assert 0.0 < lrs[0] <= tr.hyp["lr"] and lrs[0] == lrs[1] == lrs[2]  # all three rise from 0: the bias group has no head start
    # one scheduled step runs with those per-group values and the scheduled weight decay
    report = []
    tr.ni = 50
    acc, lrs, mom, wd = tr.schedule_at(50, 4)
    tr.forward_backward(*_batch(0))
    _check_optimizer_step(tr, 1, "auto, warm-up iteration 50", report, lrs=lrs, weight_decay=wd)
    KC.print_report(report, "auto under the schedule", "comparisons")
    m, ts = _trainer(optimizer="auto", iterations=10001, hyp=dict(lr=0.5))
    assert ts.optimizer_name == "SGD" and ts.V is None and ts.opt_step is None and ts.hyp["lr"] == 0.01 and ts.hyp["momentum"] == 0.9
    ts.set_schedule(batches_per_epoch=10, global_batch=4)
    assert ts.schedule_at(0, 4)[1][0] == 0.0 and ts.schedule_at(0, 4)[2] == pytest.approx(0.8)
    ts.step(*_batch(0))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ts.P).all()) and "momentum_buffer" in ts.optimizer_state()
    for kw in (dict(), dict(optimizer="SGD"), dict(optimizer="sgd")):
        m, t0 = _trainer(**kw)
        assert t0.optimizer_name == "SGD" and t0.V is None and t0.opt_step_dev is None
        assert t0.set_schedule(batches_per_epoch=10, global_batch=4).schedule_at(0, 4)[1][0] == pytest.approx(0.1)
    model = ClassificationModel("yolov8n-cls.yaml", nc=10)
    for name in ("RMSProp", "Adamax", "NAdam", "RAdam", "lion"):
        with pytest.raises(UpaError, match="AdamW"):
            ClassificationTrainer(model, device=DEV, optimizer=name)
    with pytest.raises(UpaError, match="iterations"):
        ClassificationTrainer(model, device=DEV, optimizer="auto")


@KC.stop_after_fault
def test_detection_trainer_adamw_plumbing():
    """DetectionTrainer(yolov8n, optimizer="AdamW"), f32, one step at 2 x 128 x 128 (the smallest size of the detection-trainer tests):
    the same group-by-group check."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    m = DetectionModel("yolov8n.yaml")
    P.apply_procedural_weights(m)
    tr = DetectionTrainer(m, dtype=F32, device=DEV, optimizer="AdamW", hyp=dict(lr=0.001))
    report = []
    tr.forward_backward(P.synthetic_images(2, h=128, w=128, seed=0).to(DEV), P.synthetic_labels(2, seed=0))
    _check_optimizer_step(tr, 1, "detection AdamW", report)
    KC.print_report(report, "DetectionTrainer AdamW", "comparisons")
