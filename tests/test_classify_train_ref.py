"""CPU (-m "not gpu"): classification training without a device.
  1. the float64 restatements of tests/classify_train_ref.py against float64 torch autograd (avg_pool, cross_entropy, linear);
  2. the CPU oracle step (tests/classify_train_oracle.py) against what the imported reference recorded
     (tests/golden/train_yolov8n-cls.npz), and its loss over eight steps on one batch;
  3. the host-side refusals of the new C-ABI entries (argument checks run before any launch, so they need no GPU);
  4. `ClassificationTrainer`'s constructor refusals that need no device;
  5. the flat parameter layout / gradient buckets of yolov8n-cls."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import classify_oracle as C
from tests import classify_train_oracle as T
from tests import classify_train_ref as CR
from ultralytics_pro_amd.utils import procedural as P

F64 = torch.float64


def _close(a, b, tol=1e-12):
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max()))


@pytest.mark.parametrize("shape", [(1, 16, 1, 1), (2, 40, 5, 3), (2, 8, 20, 20)])
def test_avg_pool_ref_matches_autograd(shape):
    x = P.uniform(f"ref:pool:{shape}", shape, -1.0, 1.0).to(F64).requires_grad_()
    y = torch.nn.AdaptiveAvgPool2d(1)(x).flatten(1)
    ref, mag, ops = CR.avg_pool_ref(x.detach())
    _close(ref, y.detach())
    assert bool((mag >= ref.abs() - 1e-15).all()) and ops == -(-shape[2] * shape[3] // 8) + 8
    dp = P.uniform(f"ref:dpool:{shape}", shape[:2], -1.0, 1.0).to(F64)
    (y * dp).sum().backward()
    d, dmag, dops = CR.avg_pool_bwd_ref(dp, shape[2], shape[3])
    _close(d, x.grad)
    prev = torch.ones(shape, dtype=F64)
    d2, m2, o2 = CR.avg_pool_bwd_ref(dp, shape[2], shape[3], prev)
    _close(d2, x.grad + 1.0)
    assert (dops, o2) == (1, 2) and bool((m2 >= d2.abs() - 1e-15).all())


@pytest.mark.parametrize("rows,nc,amp", [(1, 1, 1.0), (4, 10, 1.0), (3, 1000, 80.0), (65, 5, 80.0)])
def test_cross_entropy_ref_matches_autograd(rows, nc, amp):
    z = P.uniform(f"ref:z:{rows}:{nc}", (rows, nc), -amp, amp).to(F64).requires_grad_()
    t = (P.uniform(f"ref:t:{rows}:{nc}", (rows,), 0.0, 1.0) * nc).long().clamp_(0, nc - 1)
    loss = F.cross_entropy(z, t, reduction="mean")
    (loss * 1024.0).backward()
    rl, dz, mag, ops, mag_l, ops_l = CR.cross_entropy_ref(z.detach(), t, scale=1024.0)
    _close(rl, loss.detach())
    _close(dz, z.grad)
    assert bool((mag >= dz.abs() - 1e-12).all()) and float(mag_l) >= abs(float(rl)) and bool((ops >= 16).all()) and ops_l >= 75


@pytest.mark.parametrize("m,k,n", [(1, 64, 3), (5, 64, 3), (33, 96, 17)])
def test_linear_bwd_ref_matches_autograd(m, k, n):
    x = P.uniform(f"ref:lx:{m}", (m, k), -1.0, 1.0).to(F64).requires_grad_()
    lin = torch.nn.Linear(k, n).to(F64)
    dy = P.uniform(f"ref:ldy:{m}", (m, n), -1.0, 1.0).to(F64)
    (lin(x) * dy).sum().backward()
    dw, db, dx, mw, mb, mx, ow, ox = CR.linear_bwd_ref(x.detach(), dy, lin.weight.detach())
    _close(dw, lin.weight.grad)
    _close(db, lin.bias.grad)
    _close(dx, x.grad)
    assert (ow, ox) == (m, n) and bool((mw >= dw.abs() - 1e-12).all()) and bool((mx >= dx.abs() - 1e-12).all())
    dw2, db2, *_rest, ow2, _ = CR.linear_bwd_ref(x.detach(), dy, lin.weight.detach(), torch.ones(n, k), torch.ones(n))
    _close(dw2, lin.weight.grad + 1.0)
    _close(db2, lin.bias.grad + 1.0)
    assert ow2 == m + 1


def test_oracle_step_matches_reference_golden(golden_dir):
    """Case a (nc 10, bs 4, 64 x 64, two steps) of the golden: the CPU oracle reproduces the reference's record.  The generator measured
    the two bit-identical on its machine (`a_oracle_vs_ref` = 0); another CPU's kernels may round differently, hence 1e-4 relative."""
    G = np.load(golden_dir / "train_yolov8n-cls.npz")
    nc, bs, imgsz, steps = (int(v) for v in G["a_shape"])
    assert (nc, bs, imgsz, steps) == (10, 4, 64, 2) and float(G["a_oracle_vs_ref"][0]) <= 1e-6 and float(G["b_oracle_vs_ref"][0]) <= 1e-6
    assert tuple(int(v) for v in G["b_shape"]) == (1000, 2, 224, 1)
    m = C.ClassificationModel("yolov8n-cls.yaml", nc=nc)
    P.apply_procedural_weights(m, family="yolov8n-cls")
    state = T.TrainState(m)
    keys = [str(k) for k in G["a_param_keys"]]
    for step in range(steps):
        batch = T.golden_batch("a", step)
        assert np.array_equal(batch["cls"].numpy(), G[f"a_cls_{step}"]) and {0, nc - 1} <= set(batch["cls"].tolist())
        item, norm = T.train_step(m, state, batch)
        np.testing.assert_allclose(item.numpy(), G[f"a_loss_{step}"], rtol=1e-4)
        np.testing.assert_allclose(norm, float(G[f"a_grad_norm_{step}"][0]), rtol=1e-4)
        named = dict(m.named_parameters())
        l2 = np.array([float(named[k].grad.double().norm()) for k in keys])
        np.testing.assert_allclose(l2, G[f"a_grad_l2_{step}"], rtol=1e-3, atol=1e-6 * float(G[f"a_grad_l2_{step}"].max()))
        want = G[f"a_grad[model.9.linear.weight]_{step}"]
        np.testing.assert_allclose(named["model.9.linear.weight"].grad.numpy(), want, rtol=1e-3, atol=1e-5 * float(np.abs(want).max()))
        sd = m.state_dict()
        np.testing.assert_allclose(sd["model.0.conv.weight"].numpy(), G[f"a_w_stem_{step}"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(sd["model.2.cv1.bn.running_var"].numpy(), G[f"a_bn_rv_{step}"], rtol=1e-4)
        fk = [str(k) for k in G["a_state_keys"]]
        np.testing.assert_allclose(np.array([float(state.ema[k].double().sum()) for k in fk]), G[f"a_ema_sum_{step}"], rtol=1e-4, atol=1e-3)


def test_oracle_loss_falls_on_one_batch():
    """Eight oracle steps on golden (a)'s first batch with the reference's hyper-parameters (lr 0.01, Nesterov momentum 0.9, clip 10).
    Momentum makes the descent NON-monotone on this batch (10.03, 4.51, 4.00, 0.013, 3.30, 0.55, 0.00, 0.00 on the CPU: step 5 rises
    again), so the property asserted here - and of the HIP trainer in tests/test_hip_classify_train.py - is "last < first"; that the
    monotone form really is false is pinned too, so the weaker assertion is not chosen by feel."""
    m = C.ClassificationModel("yolov8n-cls.yaml", nc=10)
    P.apply_procedural_weights(m, family="yolov8n-cls")
    state = T.TrainState(m)
    batch = T.golden_batch("a", 0)
    losses = [float(T.train_step(m, state, batch)[0]) for _ in range(8)]
    print("oracle losses:", [f"{v:.4f}" for v in losses])
    assert losses[-1] < losses[0] and losses[-1] < 0.1 * losses[0], losses
    assert not all(b < a for a, b in zip(losses[1:], losses[2:])), "monotone after all: assert that form on the GPU too"


def test_new_entries_refuse_bad_arguments_on_the_host():
    """Argument checks run before any launch: a refused call needs no GPU and leaves its buffers alone."""
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    buf = torch.full((2048,), -7.0)
    tg = torch.zeros(8, dtype=torch.int32)
    p, t = buf.data_ptr(), tg.data_ptr()
    o = p + 4096
    assert lib.upa_cross_entropy_workspace_bytes(5) >= 20 and lib.upa_cross_entropy_workspace_bytes(0) == 0
    E, U = L.UPA_EINVAL, L.UPA_EUNSUPPORTED
    calls = [
        (E, lib.upa_global_avgpool_fwd(None, 2, 2, 2, 8, 8, o, 8, 0, None)),
        (E, lib.upa_global_avgpool_fwd(p, 2, 2, 2, 8, 7, o, 8, 0, None)),
        (E, lib.upa_global_avgpool_fwd(p, 2, 2, 2, 8, 8, o, 7, 0, None)),
        (E, lib.upa_global_avgpool_fwd(p, 2, 0, 2, 8, 8, o, 8, 0, None)),
        (U, lib.upa_global_avgpool_fwd(p, 2, 2, 2, 8, 8, o, 8, 2, None)),
        (E, lib.upa_global_avgpool_bwd(p, 8, 2, 2, 2, 8, None, 8, 0, 0, None)),
        (E, lib.upa_global_avgpool_bwd(p, 8, 2, 2, 2, 8, o, 7, 0, 0, None)),
        (U, lib.upa_global_avgpool_bwd(p, 8, 2, 2, 2, 8, o, 8, 0, 5, None)),
        (E, lib.upa_cross_entropy_fwd_bwd(None, 4, 10, 12, t, None, o, o + 64, 12, o + 1024, 16, None)),
        (E, lib.upa_cross_entropy_fwd_bwd(p, 4, 10, 12, None, None, o, o + 64, 12, o + 1024, 16, None)),
        (E, lib.upa_cross_entropy_fwd_bwd(p, 4, 0, 12, t, None, o, o + 64, 12, o + 1024, 16, None)),
        (E, lib.upa_cross_entropy_fwd_bwd(p, 0, 10, 12, t, None, o, o + 64, 12, o + 1024, 16, None)),
        (E, lib.upa_cross_entropy_fwd_bwd(p, 4, 10, 9, t, None, o, o + 64, 12, o + 1024, 16, None)),
        (E, lib.upa_cross_entropy_fwd_bwd(p, 4, 10, 12, t, None, o, o + 64, 9, o + 1024, 16, None)),
        (E, lib.upa_cross_entropy_fwd_bwd(p, 4, 10, 12, t, None, o, o + 64, 12, o + 1024, 12, None)),
        (E, lib.upa_linear_bwd(None, 2, 16, 16, p + 512, 3, 3, p + 1024, o, o + 1024, None, 0, 0, None)),
        (E, lib.upa_linear_bwd(p, 2, 16, 16, p + 512, 3, 3, p + 1024, None, o + 1024, None, 0, 0, None)),
        (E, lib.upa_linear_bwd(p, 2, 16, 12, p + 512, 3, 3, p + 1024, o, o + 1024, None, 0, 0, None)),
        (E, lib.upa_linear_bwd(p, 2, 16, 16, p + 512, 0, 3, p + 1024, o, o + 1024, None, 0, 0, None)),
        (U, lib.upa_linear_bwd(p, 2, 18, 20, p + 512, 3, 3, p + 1024, o, o + 1024, None, 0, 0, None)),
        (U, lib.upa_linear_bwd(p, 2, 1281, 1284, p + 512, 3, 3, p + 1024, o, o + 1024, None, 0, 0, None)),
    ]
    assert [c[1] for c in calls] == [c[0] for c in calls], calls
    assert b"linear_bwd" in lib.upa_last_error() and b"multiples of 4" in lib.upa_last_error()
    assert bool((buf == -7.0).all())


def test_trainer_refusals_without_a_device():
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.engine.trainer import ClassificationTrainer, pack_cls_targets
    from ultralytics_pro_amd.nn.tasks import ClassificationModel, DetectionModel
    with pytest.raises(UpaError, match="C3k2"):
        ClassificationTrainer(ClassificationModel("yolov11n-cls.yaml"))
    with pytest.raises(UpaError, match="Classify"):
        ClassificationTrainer(DetectionModel("yolov8n.yaml"))
    m = ClassificationModel("yolov8n-cls.yaml", nc=10)
    m.model[-1].drop.p = 0.1
    with pytest.raises(UpaError, match="Dropout"):
        ClassificationTrainer(m)
    assert pack_cls_targets({"cls": torch.tensor([0, 9, 3])}, 3, 10).dtype == torch.int32
    for bad in (torch.tensor([0, 10, 3]), torch.tensor([0, -1, 3]), torch.tensor([0, 1]), torch.tensor([0.0, 1.0, 2.0])):
        with pytest.raises(UpaError):
            pack_cls_targets({"cls": bad}, 3, 10)


def test_flat_layout_and_buckets_of_yolov8n_cls():
    from ultralytics_pro_amd.nn.tasks import ClassificationModel
    from ultralytics_pro_amd.parallel import flat_parameter_layout, gradient_bucket_table
    m = ClassificationModel("yolov8n-cls.yaml", nc=10)
    groups, meta = flat_parameter_layout(m)
    total = sum(n for _, n, _ in groups)
    assert total == sum(p.numel() for p in m.parameters()) and [wd for _, _, wd in groups] == [False, True, False]
    where = {name: (off, n) for name, off, n, _ in meta}
    (b0, bn), (w0, wn) = where["model.9.linear.bias"], where["model.9.linear.weight"]
    assert groups[0][0] <= b0 and b0 + bn <= groups[0][0] + groups[0][1] and bn == 10        # a bias: group 0, no decay
    assert groups[1][0] <= w0 and w0 + wn <= groups[1][0] + groups[1][1] and wn == 10 * 1280  # a decayed weight
    table = gradient_bucket_table([(n, o, k) for n, o, k, _ in meta], groups, target_bytes=1 << 20)
    assert table[0][0] <= 9 and sum(b - a for _, rs in table for a, b in rs) == total
    first_span = table[0][1]
    for off, n in (where["model.9.linear.bias"], where["model.9.linear.weight"], where["model.9.conv.conv.weight"]):
        assert any(a <= off and off + n <= b for a, b in first_span), "model.9.* must lie in the span that holds layer 9"
    # with a tiny target every layer is its own span: layer 9's holds exactly the head's parameters
    per_layer = gradient_bucket_table([(n, o, k) for n, o, k, _ in meta], groups, target_bytes=1)
    assert per_layer[0][0] == 9
    head = sum(p.numel() for p in m.model[-1].parameters())
    assert sum(b - a for a, b in per_layer[0][1]) == head
