"""Generate tests/golden/train_yolov8n-seg.npz: whole segmentation training steps of yolov8n-seg by the IMPORTED REFERENCE (via
oracle/ref_shim.py) on the CPU - train-mode forward, v8SegmentationLoss (box 7.5, cls 0.5, dfl 1.5, overlap_mask True), backward,
clip_grad_norm_(10), SGD-Nesterov on the three parameter groups, ModelEMA - on procedural weights (family "yolov8n-seg"), images, labels
and overlap masks (tests/segment_train_oracle.overlap_masks, at prototype resolution), as tools/gen_golden_detect_train11.py does for
yolov11n; and assert that the CPU oracle (tests/segment_train_oracle.train_step on tests/segment_oracle.SegmentationModel) follows it,
recording the measured distance.

On the CPU the reference's crop_mask slices by rounded integers whenever it sees fewer than 50 boxes (utils/ops.py:498-509); a GPU run
takes the comparison branch (:510-513), the one the HIP kernel and the oracle restate.  The name `crop_mask` that ultralytics.utils.loss
calls is therefore wrapped: every call is padded to 50 rows and sliced back, so the reference itself evaluates the comparison branch; the
wrapper counts the calls and the generator asserts that every one went that way and that the branch really is the comparison form
(against tests/segment_train_oracle.crop_mask_compare on the call's own arguments).

Run on a machine that has the reference checkout:   python -m tools.gen_golden_segment_train
Case a: bs 4, 160 x 160 (Detect levels 20 / 10 / 5, prototypes 40 x 40), two steps.  Per step (keys prefixed `a_`, suffixed `_<step>`):
loss_items (box, seg, cls, dfl), grad_norm (before clipping), grad_l2 / grad_sum per parameter (after clipping), state_sum / state_l2 /
ema_sum per floating state_dict entry, and raw: the ConvTranspose weight and bias gradients, cv4.0.2's weight gradient, the stem weight
after the step and one BatchNorm's running statistics.  `a_oracle_vs_ref` = max |oracle - reference| over (loss items, gradients,
parameters, EMA) of every step.  Data only.
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
from tests import segment_oracle as S  # noqa: E402
from tests import segment_train_oracle as ST  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

NAME, FAMILY = "yolov8n-seg", "yolov8n-seg"
REF_YAML = "/root/reference/ultralytics/cfg/models/v8/Segment/yolov8-seg.yaml"
CASES = {"a": dict(bs=4, imgsz=160, steps=2)}
RAW_KEYS = ["model.22.proto.upsample.weight", "model.22.proto.upsample.bias", "model.22.cv4.0.2.weight"]
NO_GRAD = "model.22.dfl.conv.weight"
PAD_ROWS = 50  # utils/ops.py:498: `if n < 50 and not masks.is_cuda` takes the slicing branch


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


def force_comparison_branch():
    """Wrap ultralytics.utils.loss.crop_mask: pad to PAD_ROWS rows, call the reference, slice back.  Returns the call log."""
    import ultralytics.utils.loss as RL
    real = RL.crop_mask
    log = dict(calls=0, padded=0, native=0, worst=0.0)

    def wrapped(masks, boxes):
        n = masks.shape[0]
        log["calls"] += 1
        if n < PAD_ROWS and not masks.is_cuda:
            log["padded"] += 1
            pm = torch.cat([masks, masks.new_zeros(PAD_ROWS - n, *masks.shape[1:])], 0)
            pb = torch.cat([boxes, boxes.new_zeros(PAD_ROWS - n, 4)], 0)
            out = real(pm, pb)[:n]
        else:  # 50 rows or more: the reference takes the comparison branch by itself
            log["native"] += 1
            out = real(masks, boxes)
        log["worst"] = max(log["worst"], maxdiff(out.detach(), ST.crop_mask_compare(masks.detach(), boxes.detach())))
        return out

    RL.crop_mask = wrapped
    return log


def main():
    torch.manual_seed(0)
    rt = import_reference()
    import yaml
    from ultralytics.utils.torch_utils import ModelEMA
    log = force_comparison_branch()
    hyp = otr.HYP
    G = {}
    for case, c in CASES.items():
        d = yaml.safe_load(Path(REF_YAML).read_text())
        d["scale"] = "n"
        ref = rt.SegmentationModel(d, ch=3, nc=80, verbose=False)
        P.apply_procedural_weights(ref, family=FAMILY)
        ref.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, overlap_mask=True)
        mine = S.SegmentationModel(NAME + ".yaml")
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
        mres = c["imgsz"] // 4
        for step in range(c["steps"]):
            x = P.synthetic_images(c["bs"], h=c["imgsz"], w=c["imgsz"], seed=step)
            lab = P.synthetic_labels(c["bs"], seed=step)
            lab["masks"] = ST.overlap_masks(lab, c["bs"], mres, mres)
            assert int(lab["masks"].max()) >= 2, "the overlap masks hold more than one instance"
            ref.train()
            before = log["calls"]
            loss, items_r = ref({"img": x, **lab})
            assert log["calls"] > before, "the reference did not reach crop_mask"
            loss.sum().backward()
            norm_r = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=hyp["max_norm"])
            gr = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
            opt.step()
            opt.zero_grad()
            ema.update(ref)
            items_o, norm_o = ST.train_step(mine, state, {"img": x.clone(), **lab}, hyp)
            go = {k: p.grad.detach().clone() for k, p in mine.named_parameters() if p.grad is not None}
            assert set(gr) == set(go) and NO_GRAD not in gr and NO_GRAD in dict(ref.named_parameters())
            for k in RAW_KEYS:
                assert float(gr[k].abs().max()) > 0, f"{k}: zero gradient in the reference"
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
    # every crop_mask call of the reference went through the comparison branch, and that branch is the comparison form
    assert log["calls"] > 0 and log["padded"] + log["native"] == log["calls"] and log["padded"] > 0 and log["worst"] == 0.0, log
    G["crop_mask_calls"] = np.array([log["calls"], log["padded"], log["native"]])
    out = GOLD / f"train_{NAME}.npz"
    np.savez_compressed(out, **G)
    print(f"{out.name}: {out.stat().st_size} bytes; crop_mask calls {log}")
    assert out.stat().st_size < 1000000


if __name__ == "__main__":
    main()
