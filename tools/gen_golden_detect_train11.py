"""Generate tests/golden/train_yolov11n.npz: whole detection training steps of yolov11n by the IMPORTED REFERENCE (via oracle/ref_shim.py)
on the CPU - train-mode forward, v8DetectionLoss, backward, clip_grad_norm_(10), SGD-Nesterov on the three parameter groups, ModelEMA -
on procedural weights (family "yolov11n"), images and labels, as oracle/gen_golden.py:train_golden does for yolov8n and
tools/gen_golden_classify_train11.py for yolov11n-cls; and assert that the CPU oracle (tests/yolo11_oracle.DetectionModel stepped by
oracle.train.train_step) follows it, recording the measured distance.

Run on a machine that has the reference checkout:   python -m tools.gen_golden_detect_train11
Case a: bs 4, 320 x 320, two steps (100 tokens in C2PSA, Detect levels 40 / 20 / 10).  Per step (keys prefixed `a_`, suffixed `_<step>`):
loss_items, grad_norm (before clipping), grad_l2 / grad_sum per parameter (after clipping), state_sum / state_l2 / ema_sum per floating
state_dict entry, and raw: the class-bias gradient, the two depthwise weights of Detect level 0 with their BN weight / bias gradients,
the stem weight after the step and one BatchNorm's running statistics.  `a_oracle_vs_ref` = max |oracle - reference| over (loss items,
gradients, parameters, EMA) of every step.  Data only.
"""

from __future__ import annotations

import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
GOLD = ROOT / "tests" / "golden"

from oracle import train as otr  # noqa: E402
from oracle.ref_shim import import_reference  # noqa: E402
from tests import yolo11_oracle as Y  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

NAME, FAMILY, REF_CFG = "yolov11n", "yolov11n", "cfg/models/v11/Detect/yolov11n.yaml"
CASES = {"a": dict(bs=4, imgsz=320, steps=2)}
DW = ["model.23.cv3.0.0.0", "model.23.cv3.0.1.0"]
RAW_KEYS = ["model.23.cv3.0.2.bias"] + [f"{d}.{p}" for d in DW for p in ("conv.weight", "bn.weight", "bn.bias")]
NO_GRAD = "model.23.dfl.conv.weight"


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


def main():
    torch.manual_seed(0)
    rt = import_reference()
    from ultralytics.utils.torch_utils import ModelEMA
    hyp = otr.HYP
    G = {}
    for case, c in CASES.items():
        ref = rt.DetectionModel(REF_CFG, ch=3, nc=80, verbose=False)
        P.apply_procedural_weights(ref, family=FAMILY)
        ref.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5)
        mine = Y.DetectionModel(NAME + ".yaml")
        P.apply_procedural_weights(mine, family=FAMILY)
        assert all(torch.equal(a, b) for a, b in zip(ref.state_dict().values(), mine.state_dict().values()))
        g0, g1, g2 = otr.param_groups(ref)
        opt = torch.optim.SGD([p for _, p in g2], lr=hyp["lr"], momentum=hyp["momentum"], nesterov=True)
        opt.add_param_group({"params": [p for _, p in g0], "weight_decay": hyp["weight_decay"]})
        opt.add_param_group({"params": [p for _, p in g1], "weight_decay": 0.0})
        ema = ModelEMA(ref, decay=hyp["ema_decay"], tau=hyp["ema_tau"])
        state = otr.TrainState(mine)
        worst = 0.0
        G[f"{case}_shape"] = np.array([c["bs"], c["imgsz"], c["steps"]])
        for step in range(c["steps"]):
            x = P.synthetic_images(c["bs"], h=c["imgsz"], w=c["imgsz"], seed=step)
            lab = P.synthetic_labels(c["bs"], seed=step)
            ref.train()
            loss, items_r = ref({"img": x, **lab})                # tasks.py: forward(dict) -> self.loss(batch)
            loss.sum().backward()                                 # trainer.py:424-432 (world_size 1, no scaler)
            norm_r = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=hyp["max_norm"])  # trainer.py:677
            gr = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
            opt.step()
            opt.zero_grad()
            ema.update(ref)
            items_o, norm_o = otr.train_step(mine, state, {"img": x.clone(), **lab}, hyp)
            go = {k: p.grad.detach().clone() for k, p in mine.named_parameters() if p.grad is not None}
            assert set(gr) == set(go) and NO_GRAD not in gr and NO_GRAD in dict(ref.named_parameters())
            dl = maxdiff(items_r, items_o)
            dg = max(maxdiff(gr[k], go[k]) for k in gr)
            dp = max(maxdiff(a, b) for a, b in zip(ref.state_dict().values(), mine.state_dict().values()))
            de = max(maxdiff(ema.ema.state_dict()[k], state.ema[k]) for k in state.ema)
            dn = abs(float(norm_r) - norm_o)
            print(f"train {NAME} case {case} step {step}: loss items {items_r.tolist()} |grad| {float(norm_r):.5f}  oracle-vs-ref: loss {dl:.2e} "
                  f"grad {dg:.2e} norm {dn:.2e} params {dp:.2e} ema {de:.2e}")
            assert max(dl, dg, dp, de) <= 1e-6 and dn <= 1e-6 * float(norm_r), "the CPU oracle does not follow the reference"
            worst = max(worst, dl, dg, dp, de)
            keys = list(gr.keys())
            sd = ref.state_dict()
            fk = [k for k, v in sd.items() if v.dtype.is_floating_point]
            esd = ema.ema.state_dict()
            G[f"{case}_loss_items_{step}"] = items_r.numpy().copy()
            G[f"{case}_grad_norm_{step}"] = np.array([float(norm_r)])
            G[f"{case}_grad_l2_{step}"] = np.array([float(gr[k].double().norm()) for k in keys])   # after clipping
            G[f"{case}_grad_sum_{step}"] = np.array([float(gr[k].double().sum()) for k in keys])
            G[f"{case}_state_sum_{step}"] = np.array([float(sd[k].double().sum()) for k in fk])
            G[f"{case}_state_l2_{step}"] = np.array([float(sd[k].double().norm()) for k in fk])
            G[f"{case}_ema_sum_{step}"] = np.array([float(esd[k].double().sum()) for k in fk])
            for k in RAW_KEYS:
                G[f"{case}_grad[{k}]_{step}"] = gr[k].numpy()
            G[f"{case}_w_stem_{step}"] = sd["model.0.conv.weight"].numpy().copy()
            G[f"{case}_bn_rm_{step}"] = sd["model.2.cv1.bn.running_mean"].numpy().copy()
            G[f"{case}_bn_rv_{step}"] = sd["model.2.cv1.bn.running_var"].numpy().copy()
        G[f"{case}_param_keys"] = np.array(keys)
        G[f"{case}_state_keys"] = np.array(fk)
        G[f"{case}_oracle_vs_ref"] = np.array([worst])
    out = GOLD / f"train_{NAME}.npz"
    np.savez_compressed(out, **G)
    print(f"{out.name}: {out.stat().st_size} bytes")
    assert out.stat().st_size < 1000000


if __name__ == "__main__":
    main()
