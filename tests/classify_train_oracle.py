"""ORACLE for one classification training step (test infrastructure, never on the product path).

tests/classify_oracle.ClassificationModel in train mode under torch autograd, v8ClassificationLoss = F.cross_entropy(preds,
batch["cls"], reduction="mean") (utils/loss.py:873-880), `loss * world_size` backward (engine/trainer.py:424-432), then the
optimizer step of oracle/train.py - its parameter groups, clip_grad_norm_(10), SGD with Nesterov momentum and the ModelEMA update
(engine/trainer.py:674-682, :891-950; utils/torch_utils.py:606-650).  oracle/train.py's `train_step` has the detection loss built in,
so the update loop is restated here on `oracle.train.param_groups` / `TrainState` / `HYP`; nothing under oracle/ changes.
tools/gen_golden_classify_train.py pins this step to the imported reference and records the distance in the golden.
"""

from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from oracle import train as otr

HYP = otr.HYP
TrainState = otr.TrainState


def classification_loss(preds, batch):
    """utils/loss.py:873-880: (loss, loss.detach()) of the raw train-mode logits."""
    preds = preds[1] if isinstance(preds, (list, tuple)) else preds
    loss = F.cross_entropy(preds, batch["cls"].long(), reduction="mean")
    return loss, loss.detach()


def train_step(model, state, batch, hyp=HYP, world_size=1, optimize=True):
    """Returns (loss (1,), gradient norm before clipping).  The model is updated in place; gradients stay on `.grad` (clipped)."""
    model.train()
    for p in model.parameters():
        p.grad = None
    loss, item = classification_loss(model(batch["img"]), batch)
    (loss * world_size).backward()
    if not optimize:
        return item.reshape(1), float("nan")
    params = [p for p in model.parameters() if p.grad is not None]
    total_norm = torch.nn.utils.clip_grad_norm_(params, max_norm=hyp["max_norm"])
    g0, g1, g2 = otr.param_groups(model)
    lr, mom = hyp["lr"], hyp["momentum"]
    with torch.no_grad():
        for group, wd in ((g2, 0.0), (g0, hyp["weight_decay"]), (g1, 0.0)):
            for name, p in group:
                if p.grad is None:
                    continue
                g = p.grad
                if wd:
                    g = g.add(p, alpha=wd)
                buf = state.momentum.get(name)
                if buf is None:
                    buf = state.momentum[name] = g.clone()  # torch.optim.SGD: the first step copies the gradient
                else:
                    buf.mul_(mom).add_(g)
                g = g.add(buf, alpha=mom)  # nesterov
                p.add_(g, alpha=-lr)
        state.updates += 1
        d = hyp["ema_decay"] * (1 - math.exp(-state.updates / hyp["ema_tau"]))
        msd = model.state_dict()
        for k, v in state.ema.items():
            if v.dtype.is_floating_point:
                v.mul_(d)
                v.add_((1 - d) * msd[k].detach())  # two roundings, as torch_utils.py:645-646
    return item.reshape(1), float(total_norm)


def procedural_cls(bs, nc, seed=0):
    """(bs,) int64 class ids from the counter hash the procedural weights and images come from; labels 0 and nc - 1 are forced into
    every batch of two or more so both ends of the class range are exercised."""
    from ultralytics_pro_amd.utils import procedural as P
    u = P.uniform(f"labels:cls:{seed}", (bs,), 0.0, 1.0)
    cls = (u * nc).long().clamp_(0, nc - 1)
    if bs >= 2:
        cls[0], cls[-1] = 0, nc - 1
    return cls


GOLDEN_CASES = {"a": dict(nc=10, bs=4, imgsz=64, steps=2), "b": dict(nc=1000, bs=2, imgsz=224, steps=1)}


def golden_batch(case, step):
    """The batch of step `step` of golden case 'a' / 'b' (tests/golden/train_yolov8n-cls.npz)."""
    from ultralytics_pro_amd.utils import procedural as P
    c = GOLDEN_CASES[case]
    return {"img": P.synthetic_images(c["bs"], h=c["imgsz"], w=c["imgsz"], seed=step), "cls": procedural_cls(c["bs"], c["nc"], seed=step)}
