"""Generate tests/golden/train_yolov11n-cls.npz (the yolov11n-cls counterpart of tools/gen_golden_classify_train.py) by running the IMPORTED REFERENCE (via oracle/ref_shim.py) for whole classification
training steps on the CPU - train-mode forward, v8ClassificationLoss, backward, clip_grad_norm_(10), SGD-Nesterov on the three
parameter groups, ModelEMA - on procedural weights, images and labels, as oracle/gen_golden.py:train_golden does for detection; and
assert that the CPU oracle tests/classify_train_oracle.py follows it, recording the measured distance.

Run on a machine that has the reference checkout:   python -m tools.gen_golden_classify_train11
Cases (tests/classify_train_oracle.GOLDEN_CASES):  a = nc 10, bs 4, 64 x 64, two steps;  b = nc 1000, bs 2, 224 x 224, one step.
Per case and step (keys prefixed `<case>_`, suffixed `_<step>`): loss, grad_norm (before clipping), grad_l2 / grad_sum per parameter
(after clipping), state_sum / state_l2 / ema_sum per floating state_dict entry, a few raw slices (stem weight and its gradient, one BN's
running statistics) and, for case a, the head's gradients: linear weight / bias and head BN weight / bias in full, the head conv's
first 16 filters (the whole 1280 x 256 tensor would pass the size limit of a committed file; its norm is in grad_l2), and the
gradients of layer 9's attention that only the new kernels produce: pe's depthwise weight, pe's BN weight / bias, qkv's BN weight.
`<case>_oracle_vs_ref` = max |oracle - reference| over (loss, gradients, parameters, EMA) of every step.  Data only.
"""

from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
GOLD = ROOT / "tests" / "golden"

from oracle import train as otr  # noqa: E402
from oracle.ref_shim import import_reference  # noqa: E402
from tests import classify_oracle as C  # noqa: E402
from tests import classify_train_oracle as T  # noqa: E402
from tools.gen_golden_classify import _ref_model, maxdiff  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

HEAD_KEYS = ["model.10.linear.weight", "model.10.linear.bias", "model.10.conv.bn.weight", "model.10.conv.bn.bias"]
ATTN_KEYS = ["model.9.m.0.attn.pe.conv.weight", "model.9.m.0.attn.pe.bn.weight", "model.9.m.0.attn.pe.bn.bias", "model.9.m.0.attn.qkv.bn.weight"]
HEAD_CONV, HEAD_CONV_ROWS = "model.10.conv.conv.weight", 16  # 1.3 MB per step in full: its first 16 filters (its norm is in grad_l2)


def main():
    torch.manual_seed(0)
    rt = import_reference()
    from ultralytics.utils.torch_utils import ModelEMA
    name, hyp = "yolov11n-cls", otr.HYP
    G = {}
    for case, c in T.GOLDEN_CASES.items():
        ref = _ref_model(rt, name)
        rt.ClassificationModel.reshape_outputs(ref, c["nc"])
        P.apply_procedural_weights(ref, family=name)
        mine = C.ClassificationModel(name + ".yaml", nc=c["nc"])
        P.apply_procedural_weights(mine, family=name)
        assert all(torch.equal(a, b) for a, b in zip(ref.state_dict().values(), mine.state_dict().values()))
        g0, g1, g2 = otr.param_groups(ref)
        opt = torch.optim.SGD([p for _, p in g2], lr=hyp["lr"], momentum=hyp["momentum"], nesterov=True)
        opt.add_param_group({"params": [p for _, p in g0], "weight_decay": hyp["weight_decay"]})
        opt.add_param_group({"params": [p for _, p in g1], "weight_decay": 0.0})
        ema = ModelEMA(ref, decay=hyp["ema_decay"], tau=hyp["ema_tau"])
        state = T.TrainState(mine)
        worst = 0.0
        G[f"{case}_shape"] = np.array([c["nc"], c["bs"], c["imgsz"], c["steps"]])
        for step in range(c["steps"]):
            batch = T.golden_batch(case, step)
            ref.train()
            loss, item_r = ref(dict(batch))                      # tasks.py: forward(dict) -> self.loss(batch)
            loss.backward()                                       # trainer.py:424-432 (world_size 1, no scaler)
            norm_r = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=hyp["max_norm"])  # trainer.py:677
            gr = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
            opt.step()
            opt.zero_grad()
            ema.update(ref)
            item_o, norm_o = T.train_step(mine, state, {"img": batch["img"].clone(), "cls": batch["cls"]}, hyp)
            go = {k: p.grad.detach().clone() for k, p in mine.named_parameters() if p.grad is not None}
            assert set(gr) == set(go) == set(dict(ref.named_parameters())), "a parameter without gradient"
            dl = abs(float(item_r) - float(item_o))
            dg = max(maxdiff(gr[k], go[k]) for k in gr)
            dp = max(maxdiff(a, b) for a, b in zip(ref.state_dict().values(), mine.state_dict().values()))
            de = max(maxdiff(ema.ema.state_dict()[k], state.ema[k]) for k in state.ema)
            dn = abs(float(norm_r) - norm_o)
            print(f"train {name} case {case} step {step}: loss {float(item_r):.6f} |grad| {float(norm_r):.4f}  oracle-vs-ref: loss {dl:.2e} "
                  f"grad {dg:.2e} norm {dn:.2e} params {dp:.2e} ema {de:.2e}")
            assert max(dl, dg, dp, de) <= 1e-6 and dn <= 1e-6 * float(norm_r), "the CPU oracle does not follow the reference"
            worst = max(worst, dl, dg, dp, de)
            keys = list(gr.keys())
            sd = ref.state_dict()
            fk = [k for k, v in sd.items() if v.dtype.is_floating_point]
            esd = ema.ema.state_dict()
            G[f"{case}_loss_{step}"] = np.array([float(item_r)], dtype=np.float32)
            G[f"{case}_grad_norm_{step}"] = np.array([float(norm_r)])
            G[f"{case}_grad_l2_{step}"] = np.array([float(gr[k].double().norm()) for k in keys])   # after clipping
            G[f"{case}_grad_sum_{step}"] = np.array([float(gr[k].double().sum()) for k in keys])
            G[f"{case}_state_sum_{step}"] = np.array([float(sd[k].double().sum()) for k in fk])
            G[f"{case}_state_l2_{step}"] = np.array([float(sd[k].double().norm()) for k in fk])
            G[f"{case}_ema_sum_{step}"] = np.array([float(esd[k].double().sum()) for k in fk])
            G[f"{case}_grad_stem_w_{step}"] = gr["model.0.conv.weight"].numpy()
            G[f"{case}_w_stem_{step}"] = sd["model.0.conv.weight"].numpy().copy()
            G[f"{case}_bn_rm_{step}"] = sd["model.2.cv1.bn.running_mean"].numpy().copy()
            G[f"{case}_bn_rv_{step}"] = sd["model.2.cv1.bn.running_var"].numpy().copy()
            G[f"{case}_cls_{step}"] = batch["cls"].numpy().astype(np.int64)
            if case == "a":
                for k in HEAD_KEYS + ATTN_KEYS:
                    G[f"{case}_grad[{k}]_{step}"] = gr[k].numpy()
                G[f"{case}_grad[{HEAD_CONV}]_{step}"] = gr[HEAD_CONV][:HEAD_CONV_ROWS].numpy().copy()
            G[f"{case}_linear_b_{step}"] = sd["model.10.linear.bias"].numpy().copy()
        G[f"{case}_param_keys"] = np.array(keys)
        G[f"{case}_state_keys"] = np.array(fk)
        G[f"{case}_oracle_vs_ref"] = np.array([worst])
    out = GOLD / "train_yolov11n-cls.npz"
    np.savez_compressed(out, **G)
    print(f"{out.name}: {out.stat().st_size} bytes")
    assert out.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
