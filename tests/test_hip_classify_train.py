"""-m gpu: classification training - the four kernels of csrc/classify_train.hip at the C ABI against the float64 restatements of
tests/classify_train_ref.py, and the whole `ClassificationTrainer` step against what the imported reference recorded
(tests/golden/train_yolov8n-cls.npz, tools/gen_golden_classify_train.py) and against the CPU oracle tests/classify_train_oracle.py.

Kernel cases: every call runs twice into NaN-filled outputs, the two must agree bit for bit, everything outside the payload must still
be NaN (pad columns of `dlogits` excepted: they are written as zero), and every element is held to
    |kernel - reference| <= (ops + SLACK) * 2**-24 * magnitude  (+ half a bf16 ulp where the output is bf16)
with `ops` the rounded float32 operations on the kernel's path and `magnitude` the sum of |terms|, both returned by the reference next
to the value (derivations: tests/classify_train_ref.py).  The inputs are float32 / bf16 values, exact in float64, so the reference's own
error (float64) is 2**-29 of the bound.  The `print`s give the worst error / bound per case (pytest -s)."""

import functools

import numpy as np
import pytest
import torch

from tests import classify_oracle as C
from tests import classify_train_oracle as T
from tests import classify_train_ref as CR
from tests import kernel_check as KC
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
UPA_EINVAL, UPA_EUNSUPPORTED = -1, -2


def _held(got, ref, bound, what):
    print(f"{what}: worst error / bound = {KC.check_bound(got, ref, bound, what):.3f}")


def _code(dtype):
    return 1 if dtype == BF16 else 0


# ---- 1. global average pool ---------------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 1, 1, 16, 16), (4, 2, 2, 1280, 1280), (2, 7, 7, 1280, 1280), (3, 5, 3, 40, 64), (2, 20, 20, 64, 64), (2, 3, 3, 10, 13)]
# (the last: channels and pitch off the 16-byte rule - the element-wise path)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", POOL_CASES, ids=["x".join(map(str, c)) for c in POOL_CASES])
@KC.stop_after_fault
def test_global_avgpool_fwd_bwd(case, dtype):
    """Forward: a slice chain of ceil(hw / 8) additions, 7 joining additions, one divide: ops = ceil(hw / 8) + 8, magnitude
    sum |x| / hw.  Backward: one divide (+ one addition under accumulate) of magnitude |dpooled| / hw (+ |stored|), rounded to the
    view's dtype once (bf16: + half a bf16 ulp)."""
    DEV, L, lib, st = KC.env()
    n, h, w, c, ld = case
    x = P.uniform(f"clstrain:pool:{case}", (n, c, h, w), -1.0, 1.0).to(dtype).float()
    xb = torch.full((n, h, w, ld), 7.0, dtype=dtype)
    xb[..., :c] = x.permute(0, 2, 3, 1).to(dtype)
    xd = xb.to(DEV)
    ldp = c + 4
    outs = [torch.full((n + 1, ldp), NAN, dtype=F32, device=DEV) for _ in range(2)]
    for o in outs:
        assert lib.upa_global_avgpool_fwd(xd.data_ptr(), n, h, w, c, ld, o.data_ptr(), ldp, _code(dtype), st) == 0, lib.upa_last_error()
    torch.cuda.synchronize()
    assert KC.same_bits(outs[0], outs[1]), "two runs differ"
    got = outs[0].cpu()
    assert bool(torch.isnan(got[:, c:]).all()) and bool(torch.isnan(got[n:]).all()), "wrote outside the pooled rows"
    ref, mag, ops = CR.avg_pool_ref(x)
    _held(got[:n, :c], ref, CR.bound(ops, mag), f"avgpool_fwd {case} {dtype}")
    # backward, plain and accumulating
    dp = P.uniform(f"clstrain:dpool:{case}", (n, c), -1.0, 1.0)
    dpb = torch.full((n, ldp), NAN, dtype=F32)
    dpb[:, :c] = dp
    dpd = dpb.to(DEV)
    prev = P.uniform(f"clstrain:prev:{case}", (n, c, h, w), -1.0, 1.0).to(dtype).float()
    for acc in (0, 1):
        outs = []
        for _ in range(2):
            b = torch.full((n, h, w, ld), NAN, dtype=dtype)
            if acc:
                b[..., :c] = prev.permute(0, 2, 3, 1).to(dtype)
            b = b.to(DEV)
            assert lib.upa_global_avgpool_bwd(dpd.data_ptr(), ldp, n, h, w, c, b.data_ptr(), ld, acc, _code(dtype), st) == 0, lib.upa_last_error()
            outs.append(b)
        torch.cuda.synchronize()
        assert KC.same_bits(outs[0], outs[1]), "two runs differ"
        got = outs[0].cpu().float()
        assert bool(torch.isnan(got[..., c:]).all()), "wrote outside its channel slice"
        ref, mag, ops = CR.avg_pool_bwd_ref(dp, h, w, prev if acc else None)
        _held(got[..., :c].permute(0, 3, 1, 2), ref, CR.bound(ops, mag, ref, dtype == BF16), f"avgpool_bwd {case} {dtype} acc={acc}")


# ---- 2. cross-entropy ---------------------------------------------------------------------------------------------------------------
CE_CASES = [(1, 1, 4), (4, 10, 12), (3, 1000, 1000), (2, 1001, 1004), (65, 5, 8), (256, 80, 80)]


def _ce_call(z, t, ld, scale=None):
    DEV, L, lib, st = KC.env()
    rows, nc = z.shape
    zb = torch.full((rows, ld), NAN, dtype=F32)  # a pad column read as a logit would poison the row
    zb[:, :nc] = z
    zd, td = zb.to(DEV), t.to(torch.int32).to(DEV)
    sd = None if scale is None else torch.tensor([scale], dtype=F32, device=DEV)
    nws = lib.upa_cross_entropy_workspace_bytes(rows)
    assert nws >= 4 * rows
    outs = []
    for _ in range(2):
        dz = torch.full((rows + 1, ld), NAN, dtype=F32, device=DEV)
        loss = torch.full((3,), NAN, dtype=F32, device=DEV)
        ws = torch.full((nws // 4,), NAN, dtype=F32, device=DEV)
        rc = lib.upa_cross_entropy_fwd_bwd(zd.data_ptr(), rows, nc, ld, td.data_ptr(), None if sd is None else sd.data_ptr(),
                                           loss.data_ptr() + 4, dz.data_ptr(), ld, ws.data_ptr(), nws, st)
        assert rc == 0, lib.upa_last_error()
        outs.append((dz, loss))
    torch.cuda.synchronize()
    assert KC.same_bits(outs[0][0], outs[1][0]) and KC.same_bits(outs[0][1], outs[1][1]), "two runs differ"
    dz, loss = outs[0][0].cpu(), outs[0][1].cpu()
    assert bool(torch.isnan(dz[rows:]).all()) and bool(torch.isnan(loss[[0, 2]]).all()), "wrote outside its outputs"
    assert bool((dz[:rows, nc:] == 0).all()), "pad columns of dlogits are not zero"
    return dz[:rows, :nc], loss[1]


def _targets(rows, nc, key):
    t = (P.uniform(f"clstrain:t:{key}", (rows,), 0.0, 1.0) * nc).long().clamp_(0, nc - 1)
    t[0] = 0
    t[-1] = nc - 1
    return t


@pytest.mark.parametrize("amp", [1.0, 80.0], ids=["pm1", "pm80"])
@pytest.mark.parametrize("case", CE_CASES, ids=["x".join(map(str, c)) for c in CE_CASES])
@KC.stop_after_fault
def test_cross_entropy_fwd_bwd(case, amp):
    """Bounds as derived in classify_train_ref.cross_entropy_ref: with D = max |z - max z| of a row and depth = ceil(nc / 256) + 9,
    gradient ops = 2 (D + 2) + depth + 3 on the magnitude (softmax + onehot) scale / rows; loss ops = D + depth + 6 + ceil(rows / 64)
    + 64 on mean(|max| + |log s| + |z_t| + 1).  The gradient bound also carries the absolute floor 2**-126 (the smallest normal
    float32): exp(z - max) of a far-off class underflows in float32 and not in float64, which no relative bound covers.  The +-80 family overflows exp without the max subtraction.  loss_scale = 1024 (a power
    of two) must give 1024 x the unscaled gradient bit for bit and the same loss."""
    rows, nc, ld = case
    z = P.uniform(f"clstrain:z:{case}:{amp}", (rows, nc), -amp, amp)
    t = _targets(rows, nc, case)
    dz, loss = _ce_call(z, t, ld)
    rl, rdz, mag_dz, ops_dz, mag_l, ops_l = CR.cross_entropy_ref(z, t)
    _held(dz, rdz, CR.bound(ops_dz[:, None], mag_dz) + CR.UNDERFLOW, f"cross_entropy dz {case} +-{amp:g}")
    _held(loss.reshape(1), rl.reshape(1), CR.bound(ops_l, mag_l).reshape(1), f"cross_entropy loss {case} +-{amp:g}")
    if nc == 1:
        assert float(loss) == 0.0 and bool((dz == 0).all())
    dz2, loss2 = _ce_call(z, t, ld, scale=1024.0)
    assert KC.same_bits(dz2, dz * 1024.0) and KC.same_bits(loss2.reshape(1), loss.reshape(1))


@KC.stop_after_fault
def test_cross_entropy_target_outside_the_classes_is_nan_and_in_bounds():
    rows, nc, ld = 3, 10, 12
    z = P.uniform("clstrain:z:bad", (rows, nc), -1.0, 1.0)
    for bad in (nc, -1, 2 ** 31 - 1):
        t = torch.tensor([1, bad, 2])
        DEV, L, lib, st = KC.env()
        zd, td = torch.nn.functional.pad(z, (0, ld - nc)).to(DEV), t.to(torch.int32).to(DEV)
        dz = torch.full((rows + 1, ld), 5.0, dtype=F32, device=DEV)
        loss = torch.full((3,), 5.0, dtype=F32, device=DEV)
        nws = lib.upa_cross_entropy_workspace_bytes(rows)
        ws = torch.zeros(nws // 4 + 2, dtype=F32, device=DEV)
        assert lib.upa_cross_entropy_fwd_bwd(zd.data_ptr(), rows, nc, ld, td.data_ptr(), None, loss.data_ptr() + 4, dz.data_ptr(), ld,
                                             ws.data_ptr(), nws, st) == 0
        torch.cuda.synchronize()
        dz, loss = dz.cpu(), loss.cpu()
        assert bool(torch.isnan(dz[1, :nc]).all()) and bool(torch.isfinite(dz[[0, 2], :nc]).all()) and bool(torch.isnan(loss[1]))
        assert bool((dz[:rows, nc:] == 0).all()) and bool((dz[rows] == 5.0).all()) and loss[0] == 5.0 and loss[2] == 5.0


# ---- 3. nn.Linear backward ----------------------------------------------------------------------------------------------------------
LIN_CASES = [(1, 1280, 10), (4, 1280, 10), (2, 1280, 1000), (5, 64, 3), (33, 96, 17)]


@pytest.mark.parametrize("case", LIN_CASES, ids=["x".join(map(str, c)) for c in LIN_CASES])
@KC.stop_after_fault
def test_linear_bwd(case):
    """FMA chains in index order: dW and db take m roundings (+ 1 for the accumulate addition) of sum |dy x| resp. sum |dy| (+ |stored|),
    dx takes n roundings of sum |dy W|."""
    DEV, L, lib, st = KC.env()
    m, k, n = case
    x = P.uniform(f"clstrain:lx:{case}", (m, k), -1.0, 1.0)
    dy = P.uniform(f"clstrain:ldy:{case}", (m, n), -1.0, 1.0)
    w = P.uniform(f"clstrain:lw:{case}", (n, k), -1.0, 1.0)
    dw0, db0 = P.uniform(f"clstrain:dw0:{case}", (n, k), -1.0, 1.0), P.uniform(f"clstrain:db0:{case}", (n,), -1.0, 1.0)
    ldx, lddy, lddx = k + 4, n + 3, k + 8
    xb = torch.full((m, ldx), NAN, dtype=F32)
    xb[:, :k] = x
    dyb = torch.full((m, lddy), NAN, dtype=F32)
    dyb[:, :n] = dy
    xd, dyd = xb.to(DEV), dyb.to(DEV)
    wbuf = torch.cat([torch.full((1,), NAN), w.flatten()]).to(DEV)  # w and dw one float off a 16-byte boundary: views of a flat buffer
    wd = wbuf[1:]
    for acc, with_dx in ((0, True), (1, True), (0, False)):
        outs = []
        for _ in range(2):
            dw = torch.full((n + 1, k), NAN, dtype=F32)
            db = torch.full((n + 4,), NAN, dtype=F32)
            if acc:
                dw[:n], db[:n] = dw0, db0
            dwbuf = torch.cat([torch.full((1,), NAN), dw.flatten()]).to(DEV)
            dw, db = dwbuf[1:].view(n + 1, k), db.to(DEV)
            assert dw.data_ptr() % 16 == 4 and wd.data_ptr() % 16 == 4
            dx = torch.full((m + 1, lddx), NAN, dtype=F32, device=DEV)
            rc = lib.upa_linear_bwd(xd.data_ptr(), m, k, ldx, dyd.data_ptr(), n, lddy, wd.data_ptr(), dw.data_ptr(), db.data_ptr(),
                                    dx.data_ptr() if with_dx else None, lddx, acc, st)
            assert rc == 0, lib.upa_last_error()
            outs.append((dw, db, dx))
        torch.cuda.synchronize()
        for a, b in zip(*outs):
            assert KC.same_bits(a, b), "two runs differ"
        assert bool(torch.isnan(dwbuf[0])), "wrote in front of dw"
        dw, db, dx = (t.cpu() for t in outs[0])
        assert bool(torch.isnan(dw[n:]).all()) and bool(torch.isnan(db[n:]).all()) and bool(torch.isnan(dx[m:]).all())
        assert bool(torch.isnan(dx[:, k:]).all())
        rdw, rdb, rdx, mw, mb, mx, ops_w, ops_x = CR.linear_bwd_ref(x, dy, w, dw0 if acc else None, db0 if acc else None)
        what = f"linear_bwd {case} acc={acc}"
        _held(dw[:n], rdw, CR.bound(ops_w, mw), what + " dW")
        _held(db[:n], rdb, CR.bound(ops_w, mb), what + " db")
        if with_dx:
            _held(dx[:m, :k], rdx, CR.bound(ops_x, mx), what + " dx")
        else:
            assert bool(torch.isnan(dx).all()), "dx = NULL but dx was written"


@KC.stop_after_fault
def test_refusals_launch_nothing():
    DEV, L, lib, st = KC.env()
    buf = torch.full((4096,), -7.0, dtype=F32, device=DEV)
    tg = torch.zeros(8, dtype=torch.int32, device=DEV)
    p, t = buf.data_ptr(), tg.data_ptr()
    o = p + 8192  # outputs in the second half
    pool_f = lambda x=p, n=2, h=2, w=2, c=8, ld=8, out=o, ldp=8, dt=0: lib.upa_global_avgpool_fwd(x, n, h, w, c, ld, out, ldp, dt, st)  # noqa: E731
    pool_b = lambda d=p, ldp=8, n=2, h=2, w=2, c=8, dy=o, ld=8, dt=0: lib.upa_global_avgpool_bwd(d, ldp, n, h, w, c, dy, ld, 0, dt, st)  # noqa: E731
    ce = lambda z=p, rows=4, nc=10, ldl=12, tt=t, loss=o, dz=o + 64, ldd=12, ws=o + 1024, nws=16: lib.upa_cross_entropy_fwd_bwd(  # noqa: E731
        z, rows, nc, ldl, tt, None, loss, dz, ldd, ws, nws, st)
    lin = lambda x=p, m=2, k=16, ldx=16, dy=p + 512, n=3, lddy=3, w=p + 1024, dw=o, db=o + 1024, dx=o + 2048, lddx=16: lib.upa_linear_bwd(  # noqa: E731
        x, m, k, ldx, dy, n, lddy, w, dw, db, dx, lddx, 0, st)
    einval = [pool_f(x=None), pool_f(out=None), pool_f(ld=7), pool_f(ldp=7), pool_f(n=0), pool_f(c=0), pool_b(d=None), pool_b(dy=None),
              pool_b(ld=7), pool_b(h=0), ce(z=None), ce(tt=None), ce(loss=None), ce(dz=None), ce(ws=None), ce(nc=0), ce(rows=0),
              ce(ldl=9), ce(ldd=9), ce(nws=12), lin(x=None), lin(dy=None), lin(w=None), lin(dw=None), lin(m=0), lin(n=0), lin(ldx=12),
              lin(lddy=2), lin(lddx=12)]
    assert einval == [UPA_EINVAL] * len(einval), einval
    unsupported = [pool_f(dt=2), pool_b(dt=2), lin(k=18, ldx=20, lddx=20), lin(k=1281, ldx=1284, lddx=1284), lin(ldx=18), lin(lddx=18)]
    assert unsupported == [UPA_EUNSUPPORTED] * len(unsupported), unsupported
    assert b"linear_bwd" in lib.upa_last_error()
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all()), "a refused call wrote its output"
    assert pool_f() == 0 and pool_b() == 0 and ce() == 0 and lin() == 0  # the unmodified calls are accepted
    torch.cuda.synchronize()


# ---- 4. the whole step --------------------------------------------------------------------------------------------------------------
def _trainer(nc, dtype=F32, **kw):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine.trainer import ClassificationTrainer
    from ultralytics_pro_amd.nn.tasks import ClassificationModel
    m = ClassificationModel("yolov8n-cls.yaml", nc=nc)
    P.apply_procedural_weights(m, family="yolov8n-cls")
    return m, ClassificationTrainer(m, dtype=dtype, device=DEV, **kw)


@functools.lru_cache(maxsize=None)
def _batch(case, step):
    from tests.hip_utils import DEV
    b = T.golden_batch(case, step)
    return b["img"].to(DEV), {"cls": b["cls"]}


GOLDEN_RUNS = [("a", F32), ("b", F32), ("a", BF16)]


@pytest.mark.parametrize("case,dtype", GOLDEN_RUNS, ids=["a-f32", "b-f32", "a-bf16"])
@KC.stop_after_fault
def test_training_step_matches_reference_golden(case, dtype, golden_dir):
    """Whole steps of yolov8n-cls on the HIP path against the imported reference's record, with the tolerances
    test_training_step_yolov8n_matches_reference_golden uses for the same quantities (f32: loss 2e-3, gradient norm 3e-3, per-parameter
    gradient norms 2e-2, head gradients 5e-3 + 1e-5 max, stem weight 2e-5 abs, running variance 2e-3, EMA sums 1e-3 + 1e-2; bf16: the
    AMP-like bound, loss 8 % / norm 12 % at step 0, 20 % at step 1, median per-parameter norm error 15 %).  The CPU oracle's distance to
    the reference, recorded in the golden as `<case>_oracle_vs_ref`, is 0 for both cases (bit-identical on the CPU), so the whole
    tolerance is the GPU's.  Measured on an MI355X: f32 loss within 3e-6 relative, gradient norm within 1e-6, per-parameter gradient norms
    within 9e-6 (cases a and b); bf16 loss 1.6 % / 2.9 % and norm 0.9 % / 2.2 % off at steps 0 / 1, median per-parameter norm error
    1.5 % / 2.3 %."""
    G = np.load(golden_dir / "train_yolov8n-cls.npz")
    nc, bs, imgsz, steps = (int(v) for v in G[f"{case}_shape"])
    assert float(G[f"{case}_oracle_vs_ref"][0]) <= 1e-6
    m, tr = _trainer(nc, dtype)
    keys = [str(k) for k in G[f"{case}_param_keys"]]
    named = dict(m.named_parameters())
    assert set(keys) == set(named)
    f32 = dtype == F32
    for step in range(steps):
        x, lab = _batch(case, step)
        assert np.array_equal(lab["cls"].numpy(), G[f"{case}_cls_{step}"])
        items = tr.forward_backward(x, lab)
        norm = tr.grad_norm()
        torch.cuda.synchronize()
        ref_loss, ref_norm = G[f"{case}_loss_{step}"], float(G[f"{case}_grad_norm_{step}"][0])
        print(f"case {case} {dtype} step {step}: loss {float(items[0]):.6f} (ref {float(ref_loss[0]):.6f}) |grad| {norm:.4f} (ref {ref_norm:.4f})")
        rt_items, rt_norm = (2e-3, 3e-3) if f32 else ((0.08, 0.12) if step == 0 else (0.2, 0.2))
        assert items.shape == (1,)
        np.testing.assert_allclose(items.cpu().numpy(), ref_loss, rtol=rt_items)
        assert abs(norm - ref_norm) <= rt_norm * ref_norm
        coef = min(1.0, 10.0 / (ref_norm + 1e-6))
        l2 = np.array([float(named[k].grad.double().norm()) * coef for k in keys])
        ref_l2 = G[f"{case}_grad_l2_{step}"]
        big = ref_l2 > 1e-3 * ref_l2.max()
        rel = np.abs(l2[big] - ref_l2[big]) / ref_l2[big]
        print(f"   per-parameter gradient norms: worst {rel.max():.3e}, median {np.median(rel):.3e}")
        if f32:
            np.testing.assert_allclose(l2[big], ref_l2[big], rtol=2e-2)
            if case == "a":
                for k in ["model.9.linear.weight", "model.9.linear.bias", "model.9.conv.bn.weight", "model.9.conv.bn.bias", "model.9.conv.conv.weight"]:
                    want = G[f"a_grad[{k}]_{step}"]
                    got = named[k].grad.cpu().numpy()[:want.shape[0]] * coef
                    np.testing.assert_allclose(got, want, rtol=5e-3, atol=1e-5 * float(np.abs(want).max()), err_msg=k)
        else:
            assert float(np.median(rel)) <= 0.15
        tr.optimizer_step()
        torch.cuda.synchronize()
        sd = m.state_dict()
        np.testing.assert_allclose(sd["model.0.conv.weight"].cpu().numpy(), G[f"{case}_w_stem_{step}"], rtol=0, atol=2e-5 if f32 else 1.5e-2)
        np.testing.assert_allclose(sd["model.2.cv1.bn.running_var"].cpu().numpy(), G[f"{case}_bn_rv_{step}"], rtol=2e-3 if f32 else 0.1)
        if f32:
            np.testing.assert_allclose(sd["model.2.cv1.bn.running_mean"].cpu().numpy(), G[f"{case}_bn_rm_{step}"], rtol=2e-3, atol=1e-6)
            np.testing.assert_allclose(sd["model.9.linear.bias"].cpu().numpy(), G[f"{case}_linear_b_{step}"], rtol=0, atol=2e-5)
            fk = [str(k) for k in G[f"{case}_state_keys"]]
            ema = tr.ema_state_dict()
            got = np.array([float(ema[k].double().sum()) for k in fk])
            np.testing.assert_allclose(got, G[f"{case}_ema_sum_{step}"], rtol=1e-3, atol=1e-2)
            got = np.array([float(sd[k].double().norm()) for k in fk])
            np.testing.assert_allclose(got, G[f"{case}_state_l2_{step}"], rtol=1e-3, atol=1e-4)


@KC.stop_after_fault
def test_compiled_step_equals_eager_and_two_trainers_agree():
    """compile(): the hipGraph replay follows the eager step bit for bit - loss and the flat parameter buffer over three steps - and so
    do two eager trainers from the same start (every sum of the step has a fixed order)."""
    runs = []
    for mode in ("eager", "eager", "compiled"):
        m, tr = _trainer(10, BF16)
        losses = [tr.step(*_batch("a", 0)).cpu().clone()]
        if mode == "compiled":
            tr.compile(*_batch("a", 0), warm_steps=0)
            assert len(tr._graphs) == 1
        for s in (1, 0, 1):
            losses.append(tr.step(*_batch("a", s)).cpu().clone())
        torch.cuda.synchronize()
        runs.append((torch.cat(losses), tr.P.cpu().clone(), tr.E.cpu().clone(), tr.updates))
    for other in runs[1:]:
        assert other[3] == runs[0][3] == 4
        assert KC.same_bits(other[0], runs[0][0]) and KC.same_bits(other[1], runs[0][1]) and KC.same_bits(other[2], runs[0][2])
    assert bool(torch.isfinite(runs[0][0]).all())


@KC.stop_after_fault
def test_eight_steps_on_one_batch_lower_the_loss():
    """Eight f32 steps on golden (a)'s first batch.  With the reference's hyper-parameters (lr 0.01, Nesterov momentum 0.9, clip 10)
    momentum makes the CPU oracle's loss non-monotone on this batch (tests/test_classify_train_ref.py pins that: 10.03, 4.51, 4.00,
    0.013, 3.30, 0.55, 0.00, 0.00), so "last < first" is asserted instead of a monotone descent."""
    m, tr = _trainer(10, F32)
    x, lab = _batch("a", 0)
    losses = [float(tr.step(x, lab).cpu()[0]) for _ in range(8)]
    print("losses:", [f"{v:.4f}" for v in losses])
    assert losses[-1] < losses[0], losses


@KC.stop_after_fault
def test_grad_scaler_leaves_the_unscaled_norm():
    """amp_scaler=True: the loss kernel multiplies its gradient by 2**16 (exact), the reported norm and loss are the unscaled ones
    (the existing scaler test's tolerance: 1e-3 relative on the norm, 1e-6 on the loss)."""
    (m0, t0), (m1, t1) = _trainer(10, F32), _trainer(10, F32, amp_scaler=True)
    x, lab = _batch("a", 0)
    i0, i1 = t0.forward_backward(x, lab).cpu(), t1.forward_backward(x, lab).cpu()
    n0, n1 = t0.grad_norm(), t1.grad_norm()
    torch.cuda.synchronize()
    np.testing.assert_allclose(i1.numpy(), i0.numpy(), rtol=1e-6)
    assert abs(n1 - n0) <= 1e-3 * n0, (n0, n1)
    assert abs(float(t1.G.double().norm()) / 65536.0 - n0) <= 1e-3 * n0
    t0.optimizer_step(); t1.optimizer_step()
    torch.cuda.synchronize()
    np.testing.assert_allclose(t1.P.cpu().numpy(), t0.P.cpu().numpy(), rtol=1e-5, atol=1e-6)


@KC.stop_after_fault
def test_eval_after_training_sees_the_new_weights():
    """After two steps `model.eval()` logits equal the CPU oracle's eval logits computed from the trainer's current weights within the
    f32 e2e tolerance of test_hip_classify.py (1e-3): the packed caches of Conv and of Classify's linear must follow the optimizer's
    raw-pointer writes.  A forward BEFORE training fills the caches, so a stale one would show."""
    from tests.hip_utils import DEV
    m, tr = _trainer(10, F32)
    x, lab = _batch("a", 0)
    with torch.no_grad():
        m.eval()
        z0 = m(x)[1].cpu().clone()
    for s in (0, 1):
        tr.step(*_batch("a", s))
    torch.cuda.synchronize()
    o = C.ClassificationModel("yolov8n-cls.yaml", nc=10)
    o.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    o.eval()
    with torch.no_grad():
        zo = o(x.cpu())[1]
        m.eval()
        p, z = m(x)
        torch.cuda.synchronize()
        z = z.cpu()
    d, moved = float((z - zo).abs().max()), float((z - z0).abs().max())
    print(f"eval after two steps: max|logit d| vs oracle {d:.3e}; the steps moved the logits by {moved:.3e}")
    assert d <= 1e-3 and moved > 10 * 1e-3


@KC.stop_after_fault
def test_refusals():
    from tests.hip_utils import DEV
    from ultralytics_pro_amd._lib import UpaError
    from ultralytics_pro_amd.engine.trainer import ClassificationTrainer, DetectionTrainer
    from ultralytics_pro_amd.nn.tasks import ClassificationModel, DetectionModel
    with pytest.raises(UpaError, match="C3k2"):
        ClassificationTrainer(ClassificationModel("yolov11n-cls.yaml"), device=DEV)
    with pytest.raises(UpaError, match="Classify"):
        ClassificationTrainer(DetectionModel("yolov8n.yaml"), device=DEV)
    m = ClassificationModel("yolov8n-cls.yaml", nc=10)
    m.model[-1].drop.p = 0.1
    with pytest.raises(UpaError, match="Dropout"):
        ClassificationTrainer(m, device=DEV)
    with pytest.raises(UpaError, match="Classify"):
        DetectionTrainer(ClassificationModel("yolov8n-cls.yaml", nc=10), device=DEV)
    m, tr = _trainer(10, F32)
    x, _ = _batch("a", 0)
    p0 = tr.P.clone()
    for bad in (10, -1):
        with pytest.raises(UpaError, match="outside"):
            tr.step(x, {"cls": torch.tensor([0, 1, bad, 3])})
    with pytest.raises(UpaError):
        tr.step(x, {"cls": torch.tensor([0, 1, 2])})  # three labels for four images
    torch.cuda.synchronize()
    assert torch.equal(tr.P, p0), "a refused batch changed the weights"
