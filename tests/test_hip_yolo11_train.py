"""-m gpu: YOLO11 detection training (`DetectionTrainer(..., yolo11=True)`).  The non-legacy Detect head alone against float64 autograd of
the oracle head, with the fused depthwise entries (upa_dwconv2d_bn_act_fwd / upa_dwconv_bn_act_bwd) and with the composed form
(`DWConvT.fused = False`); whole steps of yolov11n against the live CPU oracle (oracle.train.train_step on
tests/yolo11_oracle.DetectionModel) and against the imported reference's record (tests/golden/train_yolov11n.npz)."""

import numpy as np
import pytest
import torch

from tests import kernel_check as KC
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
NAME = "yolov11n"
DW_KEYS = [f"model.23.cv3.0.{j}.0.{p}" for j in (0, 1) for p in ("conv.weight", "bn.weight")]  # level 0's four depthwise gradients


@pytest.fixture
def composed_or_fused(request):
    from ultralytics_pro_amd.engine import trainer as TR
    old = TR.DWConvT.fused
    TR.DWConvT.fused = request.param
    yield request.param
    TR.DWConvT.fused = old


# ---- 1. the head alone --------------------------------------------------------------------------------------------------------------
HEAD_LEVELS = [(2, 64, 8, 8), (2, 128, 4, 4), (2, 256, 2, 2)]


def _heads(nc):
    from tests import yolo11_oracle as Y
    from ultralytics_pro_amd.nn.modules import head as H
    ch = tuple(s[1] for s in HEAD_LEVELS)
    old = H.Detect.legacy
    H.Detect.legacy = False
    try:
        hip = H.Detect(nc, ch)
    finally:
        H.Detect.legacy = old
    ora = Y.Detect(nc, ch)
    sd = {}
    for k, v in ora.state_dict().items():
        tag = f"head11:{nc}:{k}"
        if not v.dtype.is_floating_point:
            sd[k] = v
        elif k.endswith("running_var") or k.endswith("bn.weight"):
            sd[k] = P.uniform(tag, tuple(v.shape), 0.5, 1.5)
        else:
            fan = max(1, int(np.prod(v.shape[1:])))
            sd[k] = P.uniform(tag, tuple(v.shape), -1.0, 1.0) * (fan ** -0.5 if v.dim() == 4 else 0.5)
    ora.load_state_dict(sd)
    hip.load_state_dict(sd)
    assert not hip.legacy_cls
    return hip, ora


@pytest.mark.parametrize("composed_or_fused", [True, False], ids=["fused", "composed"], indirect=True)
@pytest.mark.parametrize("nc", [80, 12])  # (c3 = 80 and 64.  12, not 10: the raw map's 64 + nc channels must be a multiple of the f32 vector of 4)
@KC.stop_after_fault
def test_head_forward_and_gradients_match_float64_autograd(nc, composed_or_fused):
    """`DetectT` of a non-legacy head on three small levels, f32, under a fixed upstream gradient: the raw maps, the gradient of every
    level's input and every parameter gradient against float64 autograd of the oracle head in train mode.  Gates as the YOLO11-cls
    composites (tests/test_hip_psa_train.py): 2e-2 on each gradient's norm and 2e-2 as a relative l2 distance (parameters whose norm
    is above 1e-3 of the largest)."""
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.engine import trainer as TR
    DEV = KC.env()[0]
    hip, ora = _heads(nc)
    xs = [P.uniform(f"head11:x:{s}", s, -1.0, 1.0) for s in HEAD_LEVELS]
    ora = ora.double().train()
    xo = [x.double().requires_grad_(True) for x in xs]
    yo = ora(xo)
    dys = [P.uniform(f"head11:dy:{nc}:{i}", tuple(y.shape), -1.0, 1.0) for i, y in enumerate(yo)]
    sum((y * d.double()).sum() for y, d in zip(yo, dys)).backward()
    hip = hip.to(DEV).train()
    for p_ in hip.parameters():
        p_.grad = torch.zeros_like(p_)
    ctx = TR._Ctx(DEV, F32, 1)
    op = TR.DetectT(ctx, hip, "model.23", None)
    kinds = [type(o).__name__ for o in op.br[0][1]]
    assert kinds == ["DWConvT", "ConvT", "DWConvT", "ConvT", "ConvT"] and [type(o).__name__ for o in op.br[0][0]] == ["ConvT"] * 3
    nb = 4 * hip.reg_max
    pool = R.BufferPool()
    with R.static_buffers(pool):
        for cv in op.convs():
            cv.pack()
        xd = [R.to_nhwc(x.to(DEV), F32, key=("test", "x", i)) for i, x in enumerate(xs)]
        raw = op.forward(xd)
        dxs = []
        for i, s in enumerate(HEAD_LEVELS):
            dyd = R.to_nhwc(dys[i].to(DEV), F32, key=("test", "dy", i))
            dx = R.alloc_nhwc(*s, F32, DEV, key=("test", "dx", i))
            for k, (seq, g) in enumerate(zip(op.br[i], (dyd[:, :nb], dyd[:, nb:]))):
                for j in range(len(seq) - 1, 0, -1):
                    vt = R.view_of(seq[j].x)
                    d = R.alloc_nhwc(vt.n, vt.c, vt.h, vt.w, F32, DEV, key=("test", "d", i, k, j))
                    seq[j].backward(g, d, False)
                    g = d
                seq[0].backward(g, dx, k > 0)
            dxs.append(dx)
        for side in ctx.wgrad_streams:
            torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()

    def dist(a, b):
        return float((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-300))
    for i in range(len(xs)):
        d_y, d_x = dist(raw[i], yo[i].detach()), dist(dxs[i], xo[i].grad)
        print(f"head nc {nc} fused {composed_or_fused} level {i}: forward {d_y:.2e}, dx {d_x:.2e}")
        assert d_y <= 2e-2 and d_x <= 2e-2
    named, ref = dict(hip.named_parameters()), {k: v for k, v in ora.named_parameters() if v.grad is not None}
    top = max(float(v.grad.norm()) for v in ref.values())
    worst = 0.0
    for k, v in ref.items():
        rn = float(v.grad.norm())
        if rn <= 1e-3 * top:
            continue
        gn = float(named[k].grad.double().norm())
        assert abs(gn - rn) <= 2e-2 * rn, (k, gn, rn)
        d = dist(named[k].grad, v.grad)
        worst = max(worst, d)
        assert d <= 2e-2, (k, d)
    print(f"   worst parameter-gradient distance {worst:.2e}")


# ---- 2. whole steps ---------------------------------------------------------------------------------------------------------------------
def _pair(dtype, oracle=True, **kw):
    from tests import yolo11_oracle as Y
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    ref = None
    if oracle:
        ref = Y.DetectionModel(NAME + ".yaml")
        P.apply_procedural_weights(ref, family=NAME)
    m = DetectionModel(NAME + ".yaml")
    P.apply_procedural_weights(m, family=NAME)
    return ref, m, DetectionTrainer(m, dtype=dtype, device=DEV, yolo11=True, **kw)


def _run_steps(sz, dtype, steps=2, bs=2):
    """Training steps of yolov11n on the HIP trainer and on the live oracle, as tests/test_hip_bot3_train.py::_run_steps; one dict of
    figures per step, nothing asserted."""
    from oracle import train as otr
    from tests.hip_utils import DEV
    ref, m, tr = _pair(dtype)
    st = otr.TrainState(ref)
    named, rnamed = dict(m.named_parameters()), dict(ref.named_parameters())
    out = []
    for step in range(steps):
        x = P.synthetic_images(bs, h=sz, w=sz, seed=step)
        lab = P.synthetic_labels(bs, seed=step)
        ref_items, ref_norm = otr.train_step(ref, st, {"img": x, **lab})
        ref_items = ref_items.detach().numpy()
        coef = min(1.0, 10.0 / (ref_norm + 1e-6))  # the oracle's .grad are what clip_grad_norm_ left
        items = tr.forward_backward(x.to(DEV), lab)
        norm = tr.grad_norm()
        torch.cuda.synchronize()
        f = dict(step=step, items=items.cpu().numpy(), ref_items=ref_items, norm=norm, ref_norm=ref_norm)
        keys = [k for k, p in rnamed.items() if p.grad is not None]
        l2 = np.array([float(named[k].grad.double().norm()) * coef for k in keys])
        ref_l2 = np.array([float(rnamed[k].grad.double().norm()) for k in keys])
        big = ref_l2 > 1e-3 * ref_l2.max()
        f["l2"], f["ref_l2"] = l2[big], ref_l2[big]
        f["l2_rel"] = np.abs(l2[big] - ref_l2[big]) / ref_l2[big]
        f["dw"] = {k: float((named[k].grad.cpu() * coef - rnamed[k].grad).abs().max() / rnamed[k].grad.abs().max()) for k in DW_KEYS}
        tr.optimizer_step()
        torch.cuda.synchronize()
        sd, rsd = m.state_dict(), ref.state_dict()
        f["w_stem"] = float((sd["model.0.conv.weight"].cpu() - rsd["model.0.conv.weight"]).abs().max())
        rv, rrv = sd["model.2.cv1.bn.running_var"].cpu(), rsd["model.2.cv1.bn.running_var"]
        f["bn_rv_rel"] = float(((rv - rrv).abs() / rrv.abs()).max())
        ema = tr.ema_state_dict()
        fk = [k for k, v in st.ema.items() if v.dtype.is_floating_point]
        f["ema_sum"] = np.array([float(ema[k].double().sum()) for k in fk])
        f["ref_ema_sum"] = np.array([float(st.ema[k].double().sum()) for k in fk])
        items_rel = np.abs(f["items"] - ref_items) / np.abs(ref_items)
        print(f"yolov11n {sz} {dtype} step {step}: items {f['items']} vs {ref_items} (rel {items_rel.max():.3e}), norm {norm:.5f} vs "
              f"{ref_norm:.5f} (rel {abs(norm - ref_norm) / ref_norm:.3e}), per-parameter norm error max {f['l2_rel'].max():.3e} median "
              f"{np.median(f['l2_rel']):.3e}, stem weights {f['w_stem']:.3e}, running_var rel {f['bn_rv_rel']:.3e}, depthwise elementwise "
              f"max {max(f['dw'].values()):.3e}")
        out.append(f)
    return out


@pytest.mark.parametrize("sz", [128, 160])
@KC.stop_after_fault
def test_two_training_steps_follow_the_oracle_f32(sz):
    """f32, bs 2: the yolov8n gates unchanged (tests/test_hip_train.py) - loss items 2e-3, gradient norm 3e-3, large-parameter norms 2e-2,
    stem weight 2e-5, running_var 2e-3, EMA sums 1e-3 / 1e-2 - and the four depthwise gradients of level 0 element by element to 5e-3 of
    the tensor's largest element."""
    for f in _run_steps(sz, F32):
        np.testing.assert_allclose(f["items"], f["ref_items"], rtol=2e-3)
        assert abs(f["norm"] - f["ref_norm"]) <= 3e-3 * f["ref_norm"]
        np.testing.assert_allclose(f["l2"], f["ref_l2"], rtol=2e-2)
        assert f["w_stem"] <= 2e-5 and f["bn_rv_rel"] <= 2e-3
        np.testing.assert_allclose(f["ema_sum"], f["ref_ema_sum"], rtol=1e-3, atol=1e-2)
        assert max(f["dw"].values()) <= 5e-3, f["dw"]


def _golden_step(golden_dir, dtype):
    """One step at bs 4, 320 x 320 (Detect levels 40 / 20 / 10, 100 tokens in C2PSA) on the HIP trainer beside the imported reference's
    record; a dict of figures, nothing asserted."""
    from tests.hip_utils import DEV
    G = np.load(golden_dir / "train_yolov11n.npz")
    bs, imgsz, _ = (int(v) for v in G["a_shape"])
    _, m, tr = _pair(dtype, oracle=False)
    keys = [str(k) for k in G["a_param_keys"]]
    named = dict(m.named_parameters())
    assert set(keys) == set(named) - {"model.23.dfl.conv.weight"}
    x, lab = P.synthetic_images(bs, h=imgsz, w=imgsz, seed=0), P.synthetic_labels(bs, seed=0)
    items = tr.forward_backward(x.to(DEV), lab)
    norm = tr.grad_norm()
    torch.cuda.synchronize()
    f = dict(items=items.cpu().numpy(), ref_items=G["a_loss_items_0"], norm=norm, ref_norm=float(G["a_grad_norm_0"][0]))
    coef = min(1.0, 10.0 / (f["ref_norm"] + 1e-6))
    l2 = np.array([float(named[k].grad.double().norm()) * coef for k in keys])
    ref_l2 = G["a_grad_l2_0"]
    big = ref_l2 > 1e-3 * ref_l2.max()
    f["l2"], f["ref_l2"] = l2[big], ref_l2[big]
    f["l2_rel"] = np.abs(l2[big] - ref_l2[big]) / ref_l2[big]
    f["raw"] = {}
    for k in DW_KEYS + ["model.23.cv3.0.2.bias"]:
        want = G[f"a_grad[{k}]_0"]
        f["raw"][k] = float(np.abs(named[k].grad.cpu().numpy() * coef - want).max() / np.abs(want).max())
    dfl = named["model.23.dfl.conv.weight"].grad
    f["dfl_has_grad"] = dfl is not None and bool(dfl.abs().max() > 0)
    tr.optimizer_step()
    torch.cuda.synchronize()
    sd = m.state_dict()
    f["w_stem"], f["ref_w_stem"] = sd["model.0.conv.weight"].cpu().numpy(), G["a_w_stem_0"]
    f["bn_rv"], f["ref_bn_rv"] = sd["model.2.cv1.bn.running_var"].cpu().numpy(), G["a_bn_rv_0"]
    fk = [str(k) for k in G["a_state_keys"]]
    ema = tr.ema_state_dict()
    f["ema_sum"], f["ref_ema_sum"] = np.array([float(ema[k].double().sum()) for k in fk]), G["a_ema_sum_0"]
    items_rel = np.abs(f["items"] - f["ref_items"]) / np.abs(f["ref_items"])
    print(f"golden a {dtype}: items {f['items']} vs {f['ref_items']} (rel {items_rel.max():.3e}), norm {norm:.5f} vs {f['ref_norm']:.5f} "
          f"(rel {abs(norm - f['ref_norm']) / f['ref_norm']:.3e}), per-parameter norm error max {f['l2_rel'].max():.3e} median "
          f"{np.median(f['l2_rel']):.3e}, raw gradients elementwise max {max(f['raw'].values()):.3e}")
    return f


@KC.stop_after_fault
def test_training_step_matches_reference_golden_f32(golden_dir):
    """One step at bs 4, 320 x 320 against the imported reference's record, f32, the same gates."""
    f = _golden_step(golden_dir, F32)
    np.testing.assert_allclose(f["items"], f["ref_items"], rtol=2e-3)
    assert abs(f["norm"] - f["ref_norm"]) <= 3e-3 * f["ref_norm"]
    np.testing.assert_allclose(f["l2"], f["ref_l2"], rtol=2e-2)
    assert max(f["raw"].values()) <= 5e-3, f["raw"]
    assert not f["dfl_has_grad"]  # no gradient on either side
    np.testing.assert_allclose(f["w_stem"], f["ref_w_stem"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(f["bn_rv"], f["ref_bn_rv"], rtol=2e-3)
    np.testing.assert_allclose(f["ema_sum"], f["ref_ema_sum"], rtol=1e-3, atol=1e-2)


# bf16 whole steps.  Measured on one MI355X against the reference's record (fused entries; worst over the steps of each run), in this
# suite's session and - second figure, where it differs - from a plain script, whose library defaults dispatch some convs otherwise:
#                     loss items            gradient norm         median per-parameter norm error
#   live oracle 128   1.173e-2 | 1.152e-2   3.262e-1 | 1.903e-1   3.723e-1 | 1.655e-1     (step 1 is the worst of the session's run)
#   live oracle 160   6.860e-3              2.589e-1              1.238e-1
#   golden bs 4, 320  4.313e-3 | 4.947e-3   1.046e-1 | 1.179e-1   5.669e-2 | 6.354e-2
# The gates are twice the worst of each kind of record - the margin of every bf16 whole-step gate in this project (pool boxes and
# summation-order changes move these figures by tens of percent; between the two dispatches above step 1 at 128 pixels moved by more).
# bs 2 at 128 / 160 pixels (Detect levels down to 4 x 4, BatchNorm over 32 values) with the procedural weight family is the noisy end:
# single parameters are off by more than their norm, which is why the gate is on the median.  The golden's step, bs 4 at 320, is the
# tighter record.
BF16_LIVE = dict(items=2.35e-2, norm=6.5e-1, median=7.4e-1)
BF16_GOLDEN = dict(items=9.9e-3, norm=2.36e-1, median=1.27e-1)


def _bf16_gate(f, gate):
    items_rel = np.abs(f["items"] - f["ref_items"]) / np.abs(f["ref_items"])
    assert items_rel.max() <= gate["items"], items_rel
    assert abs(f["norm"] - f["ref_norm"]) <= gate["norm"] * f["ref_norm"], (f["norm"], f["ref_norm"])
    assert np.median(f["l2_rel"]) <= gate["median"], np.median(f["l2_rel"])


@pytest.mark.parametrize("sz", [128, 160])
@KC.stop_after_fault
def test_two_training_steps_follow_the_oracle_bf16(sz):
    for f in _run_steps(sz, BF16):
        _bf16_gate(f, BF16_LIVE)


@KC.stop_after_fault
def test_training_step_matches_reference_golden_bf16(golden_dir):
    f = _golden_step(golden_dir, BF16)
    _bf16_gate(f, BF16_GOLDEN)
    assert not f["dfl_has_grad"]


def _grads(dtype=F32, fork=True, fused=True, **kw):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine import trainer as TR
    old = TR.DetectT.fork_levels, TR.DWConvT.fused
    TR.DetectT.fork_levels, TR.DWConvT.fused = fork, fused
    try:
        _, m, tr = _pair(dtype, oracle=False, **kw)
        x, lab = P.synthetic_images(2, h=128, w=128, seed=0), P.synthetic_labels(2, seed=0)
        items = tr.forward_backward(x.to(DEV), lab)
        torch.cuda.synchronize()
        return items.cpu().clone(), tr.G.cpu().clone()
    finally:
        TR.DetectT.fork_levels, TR.DWConvT.fused = old


@KC.stop_after_fault
def test_f32_gradients_do_not_depend_on_the_stream_layout():
    """The same bits with the small Detect levels on the level stream or on the main stream and with the weight gradients on 0, 1 or 2
    side streams: every workspace of `DWConvT` is per stream selection, every sum has one order."""
    base = _grads()
    assert bool(torch.isfinite(base[1]).all())
    for kw in (dict(fork=False), dict(wgrad_streams=0), dict(wgrad_streams=2), dict(fork=False, wgrad_streams=0)):
        other = _grads(**kw)
        assert KC.same_bits(other[0], base[0]) and KC.same_bits(other[1], base[1]), kw


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_compiled_step_equals_eager(dtype):
    """The hipGraph replay follows the eager step bit for bit in the loss items and in the flat gradient buffer."""
    from tests.hip_utils import DEV
    runs = []
    x, lab = P.synthetic_images(2, h=128, w=128, seed=0).to(DEV), P.synthetic_labels(2, seed=0)
    for mode in ("eager", "compiled"):
        _, m, tr = _pair(dtype, oracle=False)
        tr.step(x, lab)
        if mode == "compiled":
            tr.compile(x, lab, warm_steps=0)
        items = tr.step(x, lab).cpu().clone()
        torch.cuda.synchronize()
        runs.append((items, tr.G.cpu().clone(), tr.P.cpu().clone()))
    assert bool(torch.isfinite(runs[0][0]).all())
    assert all(KC.same_bits(a, b) for a, b in zip(runs[0], runs[1]))


@pytest.mark.parametrize("optimizer", ["SGD", "AdamW"])
@KC.stop_after_fault
def test_one_step_moves_every_live_parameter(optimizer):
    """Live: a gradient norm above 1e-3 of the largest, the parameters every whole-step gate looks at (at 128 x 128 the box branches of
    the 8 x 8 and 4 x 4 levels may see no positive anchor and, having no weight decay on their norms and biases, rightly stay)."""
    from tests.hip_utils import DEV
    _, m, tr = _pair(BF16, oracle=False, optimizer=optimizer)
    before = {k: v.detach().cpu().clone() for k, v in m.named_parameters()}
    tr.forward_backward(P.synthetic_images(2, h=128, w=128, seed=0).to(DEV), P.synthetic_labels(2, seed=0))
    torch.cuda.synchronize()
    norms = {k: float(v.grad.double().norm()) for k, v in m.named_parameters() if v.grad is not None}
    live = [k for k, v in norms.items() if v > 1e-3 * max(norms.values())]
    assert len(live) > 100 and set(DW_KEYS) <= set(live)
    tr.optimizer_step()
    torch.cuda.synchronize()
    named = dict(m.named_parameters())
    still = [k for k in live if torch.equal(named[k].detach().cpu(), before[k])]
    assert not still, still
