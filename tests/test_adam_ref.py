"""CPU: tests/adam_ref.py against what the imported reference recorded (tools/gen_golden_adam.py).

`adam_ref` (float64, one step from float32 state) is fed the golden's own gradients and must reproduce torch's Adam / AdamW - parameters,
both moments, the step count - within `adam_bounds`: the bound is derived for a float32 evaluation in torch's operation order, which is
what torch itself ran, plus the float32 rounding of each stored value.  `auto_rule`, and the trainer's `resolve_optimizer`, equal the
recorded optimizer=auto table exactly."""

import math

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import adam_ref as AR
from tests import train_ref as TR

F64 = torch.float64
U24 = AR.U24


@pytest.fixture(scope="module")
def ops(golden_dir):
    return np.load(golden_dir / "ops_adam.npz")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _held(got, ref, bound, what, worst):
    err = (got.double() - ref).abs()
    ok = bool((err <= bound).all())
    share = float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())
    worst.append((share, what))
    assert ok, f"{what}: worst error / bound = {share:.3f}"


@pytest.mark.parametrize("run", ["Adam", "AdamW", "auto"])
def test_adam_ref_reproduces_the_reference_optimizer(ops, run):
    """Four steps of every tensor of the tiny model, each in its group (lr of the step and group, weight decay of the group).  The
    squared norm fed to the clip is the square of the float32 norm clip_grad_norm_ returned, so the coefficient is formed from the very
    number torch used; that number is within 1e-6 of the exact norm of the recorded gradients."""
    names = [str(k) for k in ops["names"]]
    groups = [int(j) for j in ops["groups"]]
    b1, b2, eps, decay = (float(x) for x in ops[f"{run}_hyp"])
    opt = str(ops[f"{run}_name"][0])
    assert opt == ("Adam" if run == "Adam" else "AdamW")
    lrs = ops[f"{run}_lrs"]
    state = {k: (_t(ops[f"p_init[{k}]"]).reshape(-1), None, None) for k in names}
    prev = {k: AR.zeros(state[k][0].numel()) for k in names}
    worst = []
    for s in range(4):
        norm = float(ops[f"{run}_norm_{s}"][0])
        exact = math.sqrt(sum(TR.sumsq_ref(_t(ops[f"grad_{s}[{k}]"]).reshape(-1)) for k in names))
        assert abs(norm - exact) <= 1e-6 * exact
        assert (norm > 10.0) == (s == 1)
        assert int(ops[f"{run}_step_{s}"][0]) == s + 1
        for k, j in zip(names, groups):
            p, m, v = state[k]
            g = _t(ops[f"grad_{s}[{k}]"]).reshape(-1)
            if k == "linear.bias":
                assert bool((g[::2] == 0).all())
            m = torch.zeros_like(p) if m is None else m
            v = torch.zeros_like(p) if v is None else v
            outs, T = AR.adam_ref(p, g, m, v, None, norm * norm, 10.0, float(lrs[s, j]), b1, b2, eps, decay if j == 1 else 0.0,
                                  opt == "AdamW", s + 1, 0.0, 0)
            em, ev, ep, _ = prev[k] = AR.adam_bounds(T, prev[k])
            pn, _, mn, vn, _ = outs
            what = f"{run} step {s} {k}"
            for tag, got, ref, e in (("p", ops[f"{run}_p_{s}[{k}]"], pn, ep), ("m", ops[f"{run}_m_{s}[{k}]"], mn, em),
                                     ("v", ops[f"{run}_v_{s}[{k}]"], vn, ev)):
                got = _t(got).reshape(-1)
                assert bool(torch.isfinite(got).all())
                _held(got, ref, e + U24 * ref.abs() + 1e-300, f"{what} {tag}", worst)
            state[k] = (pn.float(), mn.float(), vn.float())
            prev[k] = AR.carry(prev[k], outs, has_ema=False)
    print(f"{run}: {len(worst)} comparisons, worst error / bound = {max(worst)[0]:.3f} ({max(worst)[1]})")


def test_adam_ref_reproduces_the_adamw_classification_golden(golden_dir):
    """Three AdamW + ModelEMA steps of the four head tensors of yolov8n-cls (all three groups): the clipped gradients the golden stores
    go in with a zero squared norm (coefficient exactly 1).  Each tensor is put into its group by the reference's rule - the name
    contains `bias`, else the owning module is a norm layer, else decayed."""
    from tests import classify_oracle as C
    G = np.load(golden_dir / "train_yolov8n-cls_adamw.npz")
    lr, b1, b2, eps, decay, max_norm, ema_decay, ema_tau = (float(x) for x in G["hyp"])
    nc, bs, imgsz, steps = (int(v) for v in G["shape"])
    assert steps == 3 and lr == AR.auto_rule(nc, 100)[1]
    model = C.ClassificationModel("yolov8n-cls.yaml", nc=nc)
    norm = tuple(v for k, v in nn.__dict__.items() if "Norm" in k)
    owner = {f"{mn}.{pn}" if mn else pn: mod for mn, mod in model.named_modules() for pn, _ in mod.named_parameters(recurse=False)}
    keys = [str(k) for k in G["head_keys"]]
    wds = {k: 0.0 if "bias" in k else 0.0 if isinstance(owner[k], norm) else decay for k in keys}
    assert sorted(wds.values()) == [0.0, 0.0, 0.0, decay] and wds["model.9.linear.weight"] == decay
    worst = []
    for k in keys:
        p = _t(G[f"p_init[{k}]"]).reshape(-1)
        m, v, e = torch.zeros_like(p), torch.zeros_like(p), p.clone()
        prev = AR.zeros(p.numel())
        for s in range(steps):
            g = _t(G[f"grad[{k}]_{s}"]).reshape(-1)
            d = ema_decay * (1 - math.exp(-(s + 1) / ema_tau))
            outs, T = AR.adam_ref(p, g, m, v, e, 0.0, max_norm, lr, b1, b2, eps, wds[k], True, s + 1, d, 0)
            prev = AR.adam_bounds(T, prev)
            pn, _, mn, vn, en = outs
            _held(_t(G[f"p[{k}]_{s}"]).reshape(-1), pn, prev[2] + U24 * pn.abs() + 1e-300, f"step {s} {k} p", worst)
            _held(_t(G[f"ema[{k}]_{s}"]).reshape(-1), en, prev[3] + U24 * en.abs() + 1e-300, f"step {s} {k} ema", worst)
            p, m, v, e = pn.float(), mn.float(), vn.float(), en.float()
            prev = AR.carry(prev, outs)
    print(f"AdamW golden: {len(worst)} comparisons, worst error / bound = {max(worst)[0]:.3f} ({max(worst)[1]})")


def _tiny(nc):
    m = nn.Sequential()
    m.add_module("conv", nn.Conv2d(3, 8, 3, bias=False))
    m.add_module("bn", nn.BatchNorm2d(8))
    m.add_module("linear", nn.Linear(8, nc))
    return m


def test_auto_rule_equals_the_recorded_table(ops):
    """Name, lr, momentum and warmup_bias_lr of optimizer=auto for nc {1, 10, 80, 1000} x iterations {10000, 10001}, exactly - from
    `auto_rule` and from the trainer's `resolve_optimizer`; the three group sizes are those of the trainer's flat parameter layout."""
    from ultralytics_pro_amd.engine.trainer import resolve_optimizer
    from ultralytics_pro_amd.parallel import flat_parameter_layout
    assert len(ops["table_nc"]) == 8
    for i, (nc, it) in enumerate(zip(ops["table_nc"], ops["table_iterations"])):
        want = (str(ops["table_name"][i]), float(ops["table_lr"][i]), float(ops["table_momentum"][i]), float(ops["table_warmup_bias_lr"][i]))
        assert AR.auto_rule(int(nc), int(it)) == want
        name, hyp, auto = resolve_optimizer("AUTO", int(it), int(nc))
        assert (name, hyp["lr"], hyp["momentum"], auto) == (want[0], want[1], want[2], True) and want[3] == 0.0
        layout, _ = flat_parameter_layout(_tiny(int(nc)))
        assert [n for _, n, _ in layout] == [int(v) for v in ops["table_groups"][i]]
        assert [bool(wd) for _, _, wd in layout] == [False, True, False]
    assert {(int(n), int(t)): str(a) for n, t, a in zip(ops["table_nc"], ops["table_iterations"], ops["table_name"])}[(10, 10000)] == "AdamW"
