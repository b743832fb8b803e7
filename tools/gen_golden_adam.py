"""Generate tests/golden/ops_adam.npz and tests/golden/train_yolov8n-cls_adamw.npz by running the IMPORTED REFERENCE (via
oracle/ref_shim.py): its `BaseTrainer.build_optimizer` (engine/trainer.py:891-950), called unbound on a namespace that carries the two
things it reads (`args`, `data`), and the torch optimizers it builds.  Data only.

Run on a machine that has the reference checkout:   python -m tools.gen_golden_adam

ops_adam.npz - a tiny Conv + BatchNorm + Linear model (its parameters fall into all three groups):
  table_nc, table_iterations, table_name, table_lr, table_momentum, table_warmup_bias_lr, table_groups
      the optimizer=auto table over nc {1, 10, 80, 1000} x iterations {10000, 10001}; table_groups = parameter counts of the three
      param groups in the optimizer's order (biases, decayed weights, norm weights);
  for run in (Adam, AdamW, auto): four steps from recorded gradients through clip_grad_norm_(10) and opt.step(), the three groups' lr set
  before each step as warm-up does:
      <run>_hyp = (beta1, beta2, eps, weight_decay of the decayed group), <run>_name, <run>_lrs (4, 3), names, groups (group of each
      tensor), and per step s and tensor k: grad_<s>[k] (before clipping), <run>_norm_<s> (what clip_grad_norm_ returned),
      <run>_p_<s>[k], <run>_m_<s>[k], <run>_v_<s>[k] after the step, <run>_step_<s>; p_init[k].
  Gradients: log-uniform magnitudes with random signs, in 1e-6 .. 1e2 at step 1, whose norm passes 10 (clipping bites), and in
  1e-6 .. 1 at the other steps, whose norm stays below 10;
  the linear bias's gradient holds exact zeros in every step.
train_yolov8n-cls_adamw.npz - case `a` of tests/classify_train_oracle.GOLDEN_CASES (nc 10, bs 4, 64 x 64), three steps of the reference
  model under build_optimizer(name="AdamW") and ModelEMA: hyp, per step loss_<s>, grad_norm_<s> (before clipping), cls_<s>, and for the
  four head tensors HEAD_KEYS in full: grad[k]_<s> (clipped), p[k]_<s>, ema[k]_<s>; p_init[k].
"""

from __future__ import annotations

import sys
from pathlib import Path
from types import SimpleNamespace as NS

import numpy as np
import torch
import torch.nn as nn

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
GOLD = ROOT / "tests" / "golden"

from oracle import train as otr  # noqa: E402
from oracle.ref_shim import import_reference  # noqa: E402
from tests import classify_train_oracle as T  # noqa: E402
from tools.gen_golden_classify import _ref_model  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

HEAD_KEYS = ["model.9.linear.weight", "model.9.linear.bias", "model.9.conv.bn.weight", "model.9.conv.bn.bias"]
DECAY = 5e-4
STEPS = 4
# (biases, decayed weights, norm weights) learning-rate factors of the four steps: the bias group falls, the others rise
LR_FACTORS = [(1.0, 0.0, 0.0), (0.8, 0.25, 0.25), (0.6, 0.5, 0.5), (0.5, 1.0, 1.0)]


def tiny(nc=5):
    m = nn.Sequential()
    m.add_module("conv", nn.Conv2d(3, 8, 3, bias=False))
    m.add_module("bn", nn.BatchNorm2d(8))
    m.add_module("linear", nn.Linear(8, nc))
    for k, p in m.named_parameters():
        p.data = P.uniform(f"adam:p:{k}", tuple(p.shape), -1.0, 1.0)
    return m


def build(trainer_cls, model, name, nc=10, iterations=100, lr=0.001, momentum=0.9):
    self = NS(args=NS(lr0=lr, momentum=momentum, warmup_bias_lr=0.1), data={"nc": nc})
    opt = trainer_cls.build_optimizer(self, model, name=name, lr=lr, momentum=momentum, decay=DECAY, iterations=iterations)
    return opt, self


def gradient(key, shape, step):
    mag = 10.0 ** P.uniform(f"adam:gmag:{key}:{step}", shape, -6.0, 2.0 if step == 1 else 0.0)
    sign = torch.where(P.uniform(f"adam:gsign:{key}:{step}", shape, -1.0, 1.0) < 0, -1.0, 1.0)
    g = (mag * sign).float()
    if key == "linear.bias":
        g[::2] = 0.0
    return g


def ops_golden(trainer_cls):
    G = {}
    rows = []
    for nc in (1, 10, 80, 1000):
        for it in (10000, 10001):
            opt, self = build(trainer_cls, tiny(nc), "auto", nc=nc, iterations=it)
            pg = opt.param_groups
            mom = pg[0]["momentum"] if "momentum" in pg[0] else pg[0]["betas"][0]
            rows.append((nc, it, type(opt).__name__, pg[0]["lr"], mom, self.args.warmup_bias_lr,
                         [sum(p.numel() for p in g["params"]) for g in pg]))
    G["table_nc"] = np.array([r[0] for r in rows])
    G["table_iterations"] = np.array([r[1] for r in rows])
    G["table_name"] = np.array([r[2] for r in rows])
    G["table_lr"] = np.array([r[3] for r in rows], dtype=np.float64)
    G["table_momentum"] = np.array([r[4] for r in rows], dtype=np.float64)
    G["table_warmup_bias_lr"] = np.array([r[5] for r in rows], dtype=np.float64)
    G["table_groups"] = np.array([r[6] for r in rows])
    names = [k for k, _ in tiny().named_parameters()]
    G["names"] = np.array(names)
    grads = {(k, s): gradient(k, tuple(p.shape), s) for k, p in tiny().named_parameters() for s in range(STEPS)}
    n1 = float(torch.sqrt(sum((grads[(k, 1)].double() ** 2).sum() for k in names)))
    assert n1 > 10.0, n1
    for s in range(STEPS):
        ns = float(torch.sqrt(sum((grads[(k, s)].double() ** 2).sum() for k in names)))
        print(f"ops_adam step {s}: |grad| = {ns:.4f}")
        assert (ns > 10.0) == (s == 1), "step 1, and only step 1, clips"
        for k in names:
            G[f"grad_{s}[{k}]"] = grads[(k, s)].numpy()
    for k, p in tiny().named_parameters():
        G[f"p_init[{k}]"] = p.detach().numpy().copy()
    for run in ("Adam", "AdamW", "auto"):
        model = tiny()
        opt, _ = build(trainer_cls, model, run, nc=10, iterations=100)
        named = dict(model.named_parameters())
        group_of = {id(p): j for j, g in enumerate(opt.param_groups) for p in g["params"]}
        G["groups"] = np.array([group_of[id(named[k])] for k in names])
        pg = opt.param_groups
        G[f"{run}_name"] = np.array([type(opt).__name__])
        G[f"{run}_hyp"] = np.array([pg[0]["betas"][0], pg[0]["betas"][1], pg[0]["eps"], pg[1]["weight_decay"]], dtype=np.float64)
        assert pg[0]["weight_decay"] == 0.0 and pg[2]["weight_decay"] == 0.0 and not pg[0]["amsgrad"]
        lr0 = pg[0]["lr"]
        lrs = np.array([[lr0 * f for f in row] for row in LR_FACTORS], dtype=np.float64)
        G[f"{run}_lrs"] = lrs
        for s in range(STEPS):
            for j, g in enumerate(pg):
                g["lr"] = float(lrs[s, j])
            for k in names:
                named[k].grad = grads[(k, s)].clone()
            norm = torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=10.0)
            opt.step()
            G[f"{run}_norm_{s}"] = np.array([float(norm)], dtype=np.float32)
            steps = {float(opt.state[named[k]]["step"]) for k in names}
            assert steps == {float(s + 1)}
            G[f"{run}_step_{s}"] = np.array([s + 1])
            for k in names:
                st = opt.state[named[k]]
                G[f"{run}_p_{s}[{k}]"] = named[k].detach().numpy().copy()
                G[f"{run}_m_{s}[{k}]"] = st["exp_avg"].numpy().copy()
                G[f"{run}_v_{s}[{k}]"] = st["exp_avg_sq"].numpy().copy()
    out = GOLD / "ops_adam.npz"
    np.savez_compressed(out, **G)
    print(f"{out.name}: {out.stat().st_size} bytes")
    assert out.stat().st_size < (1 << 20)


def cls_golden(rt, trainer_cls):
    from ultralytics.utils.torch_utils import ModelEMA
    name, hyp, case = "yolov8n-cls", otr.HYP, "a"
    c = T.GOLDEN_CASES[case]
    steps = 3
    ref = _ref_model(rt, name)
    rt.ClassificationModel.reshape_outputs(ref, c["nc"])
    P.apply_procedural_weights(ref, family=name)
    lr = round(0.002 * 5 / (4 + c["nc"]), 6)  # what optimizer=auto gives this model
    opt, _ = build(trainer_cls, ref, "AdamW", nc=c["nc"], lr=lr, momentum=0.9)
    ema = ModelEMA(ref, decay=hyp["ema_decay"], tau=hyp["ema_tau"])
    pg = opt.param_groups
    G = {"shape": np.array([c["nc"], c["bs"], c["imgsz"], steps]),
         "hyp": np.array([lr, pg[0]["betas"][0], pg[0]["betas"][1], pg[0]["eps"], pg[1]["weight_decay"], hyp["max_norm"], hyp["ema_decay"],
                          hyp["ema_tau"]], dtype=np.float64),
         "head_keys": np.array(HEAD_KEYS)}
    named = dict(ref.named_parameters())
    for k in HEAD_KEYS:
        G[f"p_init[{k}]"] = named[k].detach().numpy().copy()
    for step in range(steps):
        batch = T.golden_batch(case, step)
        ref.train()
        loss, item = ref(dict(batch))
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=hyp["max_norm"])
        gr = {k: named[k].grad.detach().clone() for k in HEAD_KEYS}
        opt.step()
        opt.zero_grad()
        ema.update(ref)
        esd = ema.ema.state_dict()
        print(f"train {name} AdamW step {step}: loss {float(item):.6f} |grad| {float(norm):.4f}")
        G[f"loss_{step}"] = np.array([float(item)], dtype=np.float32)
        G[f"grad_norm_{step}"] = np.array([float(norm)])
        G[f"cls_{step}"] = batch["cls"].numpy().astype(np.int64)
        for k in HEAD_KEYS:
            G[f"grad[{k}]_{step}"] = gr[k].numpy()
            G[f"p[{k}]_{step}"] = named[k].detach().numpy().copy()
            G[f"ema[{k}]_{step}"] = esd[k].numpy().copy()
    out = GOLD / "train_yolov8n-cls_adamw.npz"
    np.savez_compressed(out, **G)
    print(f"{out.name}: {out.stat().st_size} bytes")
    assert out.stat().st_size < (1 << 20)


def main():
    torch.manual_seed(0)
    rt = import_reference()
    from ultralytics.engine.trainer import BaseTrainer
    ops_golden(BaseTrainer)
    cls_golden(rt, BaseTrainer)


if __name__ == "__main__":
    main()
