"""Generate tests/golden/train_yolov8n-pose.npz: whole pose training steps of yolov8n-pose by the IMPORTED REFERENCE (via
oracle/ref_shim.py) on the CPU - train-mode forward, v8PoseLoss (box 7.5, cls 0.5, dfl 1.5, pose 12, kobj 1), backward,
clip_grad_norm_(10), SGD-Nesterov on the three parameter groups, ModelEMA - on procedural weights (family "yolov8n-pose"), images and
keypoint labels (tests/pose_train_oracle.pose_labels), as tools/gen_golden_segment_train.py does for yolov8n-seg; and assert that the CPU
oracle (tests/pose_train_oracle.train_step on tests/pose_oracle.PoseModel) follows it, recording the measured distance.

Asserted on the CPU, per step: the batch has foreground anchors; both keypoint items are > 0; at least one ASSIGNED label has an
invisible keypoint and the label whose keypoints are all invisible is assigned; the oracle follows the reference (1e-6); no assignment
tie decides the step - the oracle's assignment in float64 (weights, activations and assigner) is the float32 one, anchor by anchor.  The
label seed is tried from 0 upwards until a step sequence passes the tie check; the one used is recorded (`a_label_seed`).

Run on a machine that has the reference checkout:   python -m tools.gen_golden_pose_train
Case a: bs 4, 160 x 160 (Detect levels 20 / 10 / 5), two steps.  Per step (keys prefixed `a_`, suffixed `_<step>`): loss_items (box, pose,
kobj, cls, dfl), grad_norm (before clipping), grad_l2 / grad_sum per parameter (after clipping), state_sum / state_l2 / ema_sum per
floating state_dict entry, and raw: the gradients of cv4.0.2's weight and cv4.0.0's conv weight, the stem weight after the step and the
running statistics of one cv4 BatchNorm.  `a_oracle_vs_ref` = max |oracle - reference| over (loss items, gradients, parameters, EMA) of
every step.  Data only.
"""

from __future__ import annotations

import copy
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
from tests import pose_oracle as PO  # noqa: E402
from tests import pose_train_oracle as PT  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

NAME, FAMILY = "yolov8n-pose", "yolov8n-pose"
REF_YAML = "/root/reference/ultralytics/cfg/models/v8/Pose/yolov8-pose.yaml"
CASES = {"a": dict(bs=4, imgsz=160, steps=2)}
RAW_KEYS = ["model.22.cv4.0.2.weight", "model.22.cv4.0.0.conv.weight"]
BN = "model.22.cv4.0.0.bn"
NO_GRAD = "model.22.dfl.conv.weight"
SEEDS = range(8)


class Tie(Exception):
    pass


def maxdiff(a, b):
    return float((a.double() - b.double()).abs().max()) if a.numel() else 0.0


def run_case(rt, case, c, seed0):
    """The steps of one case with label / image seeds seed0, seed0 + 1, ...; raises Tie if float64 assigns another anchor."""
    import yaml
    from ultralytics.utils.torch_utils import ModelEMA
    hyp = otr.HYP
    G = {}
    d = yaml.safe_load(Path(REF_YAML).read_text())
    d["scale"] = "n"
    ref = rt.PoseModel(d, ch=3, nc=None, verbose=False)
    P.apply_procedural_weights(ref, family=FAMILY)
    ref.args = SimpleNamespace(box=7.5, cls=0.5, dfl=1.5, pose=12.0, kobj=1.0)
    mine = PO.PoseModel(NAME + ".yaml")
    P.apply_procedural_weights(mine, family=FAMILY)
    assert all(torch.equal(a, b) for a, b in zip(ref.state_dict().values(), mine.state_dict().values()))
    kpt_shape = tuple(mine.model[-1].kpt_shape)
    g0, g1, g2 = otr.param_groups(ref)
    opt = torch.optim.SGD([p for _, p in g2], lr=hyp["lr"], momentum=hyp["momentum"], nesterov=True)
    opt.add_param_group({"params": [p for _, p in g0], "weight_decay": hyp["weight_decay"]})
    opt.add_param_group({"params": [p for _, p in g1], "weight_decay": 0.0})
    ema = ModelEMA(ref, decay=hyp["ema_decay"], tau=hyp["ema_tau"])
    state = otr.TrainState(mine)
    worst = 0.0
    G[f"{case}_shape"] = np.array([c["bs"], c["imgsz"], c["steps"]])
    G[f"{case}_label_seed"] = np.array([seed0])
    for step in range(c["steps"]):
        x = P.synthetic_images(c["bs"], h=c["imgsz"], w=c["imgsz"], seed=seed0 + step)
        lab = PT.pose_labels(c["bs"], seed=seed0 + step, kpt_shape=kpt_shape)
        # the tie check first, on the weights this step starts from: the assignment in float64
        m64 = copy.deepcopy(mine).double().train()
        i64 = dict(assign_only=True)
        with torch.no_grad():
            PT.v8_pose_loss(m64(x.double()), lab, m64.stride, kpt_shape, nc=m64.model[-1].nc, info=i64)
        ref.train()
        loss, items_r = ref({"img": x, **lab})
        loss.sum().backward()
        norm_r = torch.nn.utils.clip_grad_norm_(ref.parameters(), max_norm=hyp["max_norm"])
        gr = {k: p.grad.detach().clone() for k, p in ref.named_parameters() if p.grad is not None}
        opt.step()
        opt.zero_grad()
        ema.update(ref)
        info = {}
        items_o, norm_o = PT.train_step(mine, state, {"img": x.clone(), **lab}, hyp, info=info)
        fg, idx = info["fg_mask"], info["target_gt_idx"]
        if not (torch.equal(fg, i64["fg_mask"]) and torch.equal(idx[fg], i64["target_gt_idx"][fg])):
            raise Tie(f"seed {seed0} step {step}: float64 assigns {int((fg != i64['fg_mask']).sum())} anchors differently")
        # what the batch is there for
        assert int(fg.sum()) > 0, "no foreground anchor"
        assert float(items_r[1]) > 0 and float(items_r[2]) > 0, items_r
        bi = lab["batch_idx"].long()
        vis = lab["keypoints"][..., 2]
        assigned = set()
        for i in range(c["bs"]):
            rows = (bi == i).nonzero().view(-1)
            assigned |= {int(rows[g]) for g in idx[i][fg[i]].unique().tolist()}
        assert any(bool((vis[j] == 0).any()) for j in assigned), "no assigned label has an invisible keypoint"
        blind = [j for j in range(vis.shape[0]) if bool((vis[j] == 0).all())]
        assert blind and any(j in assigned for j in blind), f"the label without a visible keypoint ({blind}) is not assigned"
        go = {k: p.grad.detach().clone() for k, p in mine.named_parameters() if p.grad is not None}
        assert set(gr) == set(go) and NO_GRAD not in gr and NO_GRAD in dict(ref.named_parameters())
        for k in RAW_KEYS:
            assert float(gr[k].abs().max()) > 0, f"{k}: zero gradient in the reference"
        dl = maxdiff(items_r, items_o)
        dg = max(maxdiff(gr[k], go[k]) for k in gr)
        dp = max(maxdiff(a, b) for a, b in zip(ref.state_dict().values(), mine.state_dict().values()))
        de = max(maxdiff(ema.ema.state_dict()[k], state.ema[k]) for k in state.ema)
        dn = abs(float(norm_r) - norm_o)
        print(f"train {NAME} case {case} seed {seed0} step {step}: loss items {items_r.tolist()} |grad| {float(norm_r):.5f} fg {int(fg.sum())} "
              f"oracle-vs-ref: loss {dl:.2e} grad {dg:.2e} norm {dn:.2e} params {dp:.2e} ema {de:.2e}")
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
        G[f"{case}_bn_rm_{step}"] = sd[BN + ".running_mean"].numpy().copy()
        G[f"{case}_bn_rv_{step}"] = sd[BN + ".running_var"].numpy().copy()
    G[f"{case}_param_keys"] = np.array(keys)
    G[f"{case}_state_keys"] = np.array(fk)
    G[f"{case}_oracle_vs_ref"] = np.array([worst])
    return G


def main():
    torch.manual_seed(0)
    rt = import_reference()
    G = {}
    for case, c in CASES.items():
        for seed in SEEDS:
            try:
                G.update(run_case(rt, case, c, seed))
                break
            except Tie as t:
                print(f"tie: {t}; next seed")
        else:
            raise SystemExit("no tie-free label seed")
    out = GOLD / f"train_{NAME}.npz"
    np.savez_compressed(out, **G)
    print(f"{out.name}: {out.stat().st_size} bytes")
    assert out.stat().st_size < 1000000


if __name__ == "__main__":
    main()
