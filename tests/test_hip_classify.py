"""-m gpu: image classification on the HIP path.  `upa_classify_pool` and `upa_softmax_topk` through the C ABI against the float64
references and derived bounds of tests/classify_ref.py; their refusals; the `Classify` module against the reference's per-op
goldens; the whole yolov8n-cls / yolov11n-cls models against the e2e goldens and the CPU checker tests/classify_oracle.py (f32 parity,
bf16 smooth family under three dispatches, graph replay, batch invariance); `ClassificationValidator` on targets built from the
checker's own ranking."""

import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import classify_oracle as C
from tests import classify_ref as CF
from tests import conv_ref as CR
from tests import kernel_check as KC
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu
TOL = 1e-3
THROUGHPUT = dict(c2f=4, conv_ws3=1, c2f_stream_rows=-1, detect_stream=2, conv_big=2)  # engine/pipeline.py PipelinedRunner.throughput_opts
DEV = torch.device("cuda:0")
# bf16 smooth family: max |logit - checker's f32 logit| over 2 images, measured on an MI355X per dispatch:
#   yolov8n-cls  (logit std 4.22): session 0.0812, serial 0.0812, throughput 0.0825;  max |prob d| 0.0022
#   yolov11n-cls (logit std 3.24): session 0.0327, serial 0.0327, throughput 0.0327;  max |prob d| 0.0026
# BF16_LOGIT_MEASURED is the worst of the three per model; the gate is twice that worst (box-to-box and dispatch variation
# of this path has not been measured otherwise).
BF16_LOGIT_MEASURED = {"yolov8n-cls": 0.0825, "yolov11n-cls": 0.0327}


def _dispatch(which):
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    if which == "session":
        return contextlib.nullcontext()
    if which == "serial":
        return R.use_opts(L.Opts())
    return R.use_opts(**THROUGHPUT)


def _stream():
    from ultralytics_pro_amd import _lib as L
    return L.current_stream(DEV)


# ---- 1. upa_classify_pool ---------------------------------------------------------------------------------------------------------------
# (h, w, cin, cout, n, dtype, act, family).  Every value of every axis - HW 1 / 49 (masked rows) / 64 (exact chunk) / 65 (chunk + 1) / 400,
# cin 16 (below one bf16 MFMA depth) / 32 / 256 / 1280, cout 16 / 48 (not a multiple of the 64-channel slice) / 1280, n 1 / 3, both dtypes,
# SiLU / none, uniform / positive / impulse - and the pairs (HW 49 | 65) x (cin 16 | 1280) x both dtypes.
F32, BF16 = torch.float32, torch.bfloat16
SILU, NONE = CR.ACT_SILU, CR.ACT_NONE
POOL_CASES = [
    (7, 7, 16, 48, 3, F32, SILU, "uniform"), (7, 7, 16, 48, 3, BF16, SILU, "uniform"),
    (7, 7, 1280, 16, 1, F32, SILU, "uniform"), (7, 7, 1280, 48, 3, BF16, SILU, "uniform"),
    (5, 13, 16, 16, 1, F32, NONE, "uniform"), (5, 13, 16, 48, 3, BF16, SILU, "positive"),
    (5, 13, 1280, 48, 1, F32, SILU, "positive"), (5, 13, 1280, 16, 3, BF16, NONE, "uniform"),
    (1, 1, 16, 16, 1, F32, SILU, "uniform"), (1, 1, 32, 48, 3, BF16, SILU, "uniform"), (1, 1, 256, 1280, 1, BF16, NONE, "positive"),
    (1, 1, 1280, 48, 3, F32, NONE, "uniform"),
    (8, 8, 16, 48, 1, BF16, SILU, "uniform"), (8, 8, 32, 16, 3, F32, SILU, "positive"), (8, 8, 256, 48, 3, BF16, SILU, "uniform"),
    (8, 8, 256, 48, 1, F32, NONE, "uniform"), (8, 8, 32, 1280, 1, F32, SILU, "uniform"),
    (20, 20, 16, 16, 1, BF16, SILU, "uniform"), (20, 20, 32, 48, 3, F32, SILU, "uniform"), (20, 20, 256, 48, 1, BF16, SILU, "positive"),
    (20, 20, 256, 16, 1, F32, NONE, "positive"), (20, 20, 32, 1280, 1, BF16, SILU, "uniform"),
    (7, 7, 32, 1280, 3, BF16, SILU, "uniform"), (7, 7, 256, 1280, 1, F32, SILU, "uniform"), (7, 7, 256, 48, 3, F32, NONE, "positive"),
    (7, 7, 32, 16, 1, BF16, NONE, "positive"), (5, 13, 32, 48, 3, F32, SILU, "uniform"), (5, 13, 256, 1280, 1, BF16, SILU, "uniform"),
    (7, 7, 16, 48, 3, F32, SILU, "impulse"), (7, 7, 1280, 16, 3, BF16, SILU, "impulse"), (5, 13, 16, 48, 3, BF16, NONE, "impulse"),
    (5, 13, 256, 48, 3, F32, SILU, "impulse"), (8, 8, 32, 48, 3, BF16, SILU, "impulse"), (20, 20, 32, 48, 3, F32, NONE, "impulse"),
    (1, 1, 32, 16, 3, F32, SILU, "impulse"), (20, 20, 256, 48, 3, BF16, SILU, "impulse"),
    (7, 7, 32, 48, 3, F32, SILU, "bias"), (7, 7, 32, 48, 3, BF16, SILU, "bias"), (7, 7, 16, 1280, 1, F32, SILU, "bias"),
    (7, 7, 256, 16, 1, BF16, NONE, "bias"),
]


def _pool_id(c):
    h, w, cin, cout, n, dt, act, fam = c
    return f"{h}x{w}-cin{cin}-cout{cout}-n{n}-{'bf16' if dt == BF16 else 'f32'}-{'silu' if act == SILU else 'none'}-{fam}"


def _pool_inputs(case, idx):
    """(x NCHW, w (cout, cin), bias) as CPU float32 holding values the dtype stores exactly.
      uniform   everything in [-1, 1];            positive  inputs and weights in [0, 1]: no cancellation, |sum| = S;
      impulse   one lit pixel per image, at flat positions first / last / 16th / 17th (a wave's last row and the next wave's first) in
                turn, starting at a position that depends on the case - a dropped or doubled row moves a whole pixel's activation;
      bias      x = 0, bias in [-8, 8]: every pixel's activation is act(bias) and so is the mean - a padded row that counts, or a
                divisor that counts it, shows at once."""
    h, w, cin, cout, n, dt, act, fam = case
    base = "impulse" if fam == "impulse" else "uniform"
    x, wt, b, _ = CR.conv_family(base, n, cin, h, w, cout, 1, dt, seed=100 + idx)
    if fam == "positive":
        x, wt = CR.stored(x.abs(), dt), CR.stored(wt.abs(), dt)
    elif fam == "impulse":
        hw = h * w
        pos = [0, hw - 1, 15 % hw, 16 % hw]
        lit = x.flatten(2).abs().sum(1).argmax(1)  # where conv_family put each image's pixel
        x2 = torch.zeros_like(x).flatten(2)
        for i in range(n):
            x2[i, :, pos[(i + idx) % 4]] = x.flatten(2)[i, :, lit[i]]
        x = x2.view_as(x)
    elif fam == "bias":
        x = torch.zeros_like(x)
        b = b * 8.0
    return x, wt.reshape(cout, cin), b


def _pack(wt, dt):
    from ultralytics_pro_amd import _lib as L
    cout, cin = wt.shape
    code = L.dtype_code(dt)
    host = torch.empty(L.lib().upa_conv_packed_weight_bytes(cout, cin, 1, code), dtype=torch.uint8)
    wc = wt.contiguous()
    L.check(L.lib().upa_pack_conv_weight(wc.data_ptr(), cout, cin, 1, code, host.data_ptr()), "pack")
    return host.to(DEV)


def _run_pool(x, wt, b, act, dt, runs=1):
    """x through a channel slice of a wider NaN-filled NHWC buffer (ldx > cin), pooled into a column slice of a NaN-filled buffer with a
    spare row behind (ldp > cout).  Returns (list of `runs` results on the CPU, everything outside the slice still NaN)."""
    from ultralytics_pro_amd import _lib as L
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    E = 16 // (2 if dt == BF16 else 4)
    ldx = cin + 2 * E
    xb = torch.full((n, h, w, ldx), float("nan"), dtype=dt, device=DEV)
    xb[..., E:E + cin] = x.permute(0, 2, 3, 1).to(DEV).to(dt)
    wp, bd = _pack(wt, dt), b.to(DEV)
    ldp, c0 = cout + 5, 3
    outs, clean = [], True
    for _ in range(runs):
        pb = torch.full((n + 1, ldp), float("nan"), dtype=torch.float32, device=DEV)
        L.check(L.lib().upa_classify_pool(xb.data_ptr() + E * xb.element_size(), n, h, w, cin, ldx, wp.data_ptr(), bd.data_ptr(),
                                          pb.data_ptr() + 4 * c0, cout, ldp, act, L.dtype_code(dt), None, _stream()), "classify_pool")
        torch.cuda.synchronize()
        pc = pb.cpu()
        outs.append(pc[:n, c0:c0 + cout].clone())
        pc[:n, c0:c0 + cout] = float("nan")
        clean = clean and bool(torch.isnan(pc).all())
    return outs, clean


@pytest.mark.parametrize("idx", range(len(POOL_CASES)), ids=[_pool_id(c) for c in POOL_CASES])
@KC.stop_after_fault
def test_classify_pool_vs_float64(idx):
    case = POOL_CASES[idx]
    h, w, cin, cout, n, dt, act, fam = case
    x, wt, b = _pool_inputs(case, idx)
    ref, bound = CF.pool_ref(x, wt, b, act)
    (y1, y2), clean = _run_pool(x, wt, b, act, dt, runs=2)
    assert clean, "wrote outside the (n, cout) slice of pooled"
    assert not bool(torch.isnan(y1).any()), "NaN in the output: read outside the channel slice of x, or left an element unwritten"
    err = (y1.double() - ref).abs()
    ratio = float((err / bound).max())
    print(f"classify_pool {_pool_id(case)}: max|err| {float(err.max()):.3e}, worst err / bound {ratio:.3f}")
    assert bool((err <= bound).all()), f"{int((err > bound).sum())} of {err.numel()} outside the bound, worst ratio {ratio:.2f}"
    assert torch.equal(y1, y2), "two runs differ"
    if fam == "bias":  # the reference is exactly act(bias) per channel
        want = CR.act_ref(b.double(), act).expand(n, -1)
        assert float((ref - want).abs().max()) <= 1e-15 * float(want.abs().max())


# ---- 2. upa_softmax_topk ----------------------------------------------------------------------------------------------------------------
def _softmax_input(family, rows, nc, k):
    g = torch.Generator().manual_seed(rows * 7919 + nc)
    z = torch.rand(rows, nc, generator=g) * 8 - 4
    if family == "wide":  # +-80: exp(z - max) underflows to 0 for most entries, nothing is NaN
        z = z * 20
    elif family == "equal":
        z = torch.full((rows, nc), 1.25)
    elif family == "ties":  # duplicated logits straddling rank k: the k-th and (k + 1)-th largest are the same number
        for r in range(rows):
            order = z[r].argsort(descending=True)
            if nc > k:
                z[r, order[k]] = z[r, order[k - 1]]
            if k >= 2:
                z[r, order[0]] = z[r, order[1]]
        z[:, nc // 2] = -0.0
        if nc > 2:
            z[:, nc // 2 + 1] = 0.0
    elif family == "inf":
        z[:, ::3] = -float("inf")
        z[:, min(1, nc - 1)] = 0.5  # a finite maximum in every row
    return z


SOFTMAX_CASES = ([(fam, rows, nc, min(nc, 5)) for fam, rows, nc in
                  [("uniform", 1, 1), ("uniform", 3, 2), ("uniform", 33, 5), ("uniform", 3, 63), ("uniform", 1, 64), ("uniform", 33, 65),
                   ("uniform", 3, 1000), ("uniform", 3, 4099), ("wide", 3, 5), ("wide", 33, 64), ("wide", 3, 1000), ("wide", 1, 4099),
                   ("equal", 3, 2), ("equal", 1, 65), ("equal", 3, 1000), ("ties", 33, 5), ("ties", 3, 63), ("ties", 3, 65), ("ties", 3, 1000),
                   ("ties", 1, 4099), ("inf", 3, 5), ("inf", 33, 64), ("inf", 3, 1000), ("inf", 3, 4099)]]
                 + [("uniform", 3, 1000, 16), ("ties", 33, 1000, 16), ("equal", 1, 1000, 16), ("inf", 3, 1000, 16), ("wide", 3, 1000, 16)])


@pytest.mark.parametrize("family,rows,nc,k", SOFTMAX_CASES, ids=[f"{f}-r{r}-nc{n}-k{k}" for f, r, n, k in SOFTMAX_CASES])
@KC.stop_after_fault
def test_softmax_topk_vs_float64(family, rows, nc, k):
    from ultralytics_pro_amd import _lib as L
    z = _softmax_input(family, rows, nc, k)
    ref, bound, sum_tol = CF.softmax_ref(z)
    ldl, ldpr, g0 = nc + 3, nc + 6, 2
    zb = torch.full((rows + 1, ldl), float("nan"), dtype=torch.float32)
    zb[:rows, g0:g0 + nc] = z
    zb = zb.to(DEV)
    pb = torch.full((rows + 1, ldpr), float("nan"), dtype=torch.float32, device=DEV)
    tk = torch.full((rows + 1, k), -7, dtype=torch.int32, device=DEV)
    L.check(L.lib().upa_softmax_topk(zb.data_ptr() + 4 * g0, rows, nc, ldl, pb.data_ptr() + 4 * g0, ldpr, k, tk.data_ptr(), _stream()),
            "softmax_topk")
    pb2 = torch.full((rows + 1, ldpr), float("nan"), dtype=torch.float32, device=DEV)
    L.check(L.lib().upa_softmax_topk(zb.data_ptr() + 4 * g0, rows, nc, ldl, pb2.data_ptr() + 4 * g0, ldpr, k, None, _stream()),
            "softmax_topk without top-k")
    torch.cuda.synchronize()
    pc, tc = pb.cpu(), tk.cpu()
    p = pc[:rows, g0:g0 + nc].clone()
    assert torch.equal(p, pb2.cpu()[:rows, g0:g0 + nc]), "topk_idx = NULL changed the probabilities"
    pc[:rows, g0:g0 + nc] = float("nan")
    assert bool(torch.isnan(pc).all()), "wrote outside the rows' nc columns"
    assert bool((tc[rows] == -7).all()), "wrote past the last top-k row"
    assert not bool(torch.isnan(p).any())
    err = (p.double() - ref).abs()
    print(f"softmax {family} rows {rows} nc {nc}: worst err / bound {float((err / bound).max()):.3f}, "
          f"worst |sum - 1| / tol {float((p.double().sum(1) - 1).abs().max()) / sum_tol:.3f}")
    assert bool((err <= bound).all())
    assert float((p.double().sum(1) - 1).abs().max()) <= sum_tol
    if family == "inf":
        assert bool((p[torch.isinf(z)] == 0).all())
    want = CF.topk_ref(z, k)
    assert torch.equal(tc[:rows], want), f"top-{k} differs from the stable descending sort in {int((tc[:rows] != want).any(1).sum())} rows"
    if family == "equal":
        assert tc[:rows].tolist() == [list(range(k))] * rows


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------------
@KC.stop_after_fault
def test_refusals_launch_nothing():
    from ultralytics_pro_amd import _lib as L
    lib, st = L.lib(), _stream()
    n, h, w, cin, cout = 2, 3, 3, 32, 16
    x = torch.zeros((n, h, w, cin), dtype=torch.float32, device=DEV)
    wp = _pack(torch.zeros(cout, cin), F32)
    b = torch.zeros(cout, device=DEV)
    out = torch.full((n, cout), -7.0, device=DEV)
    X, W, B, O = x.data_ptr(), wp.data_ptr(), b.data_ptr(), out.data_ptr()
    good = [X, n, h, w, cin, cin, W, B, O, cout, cout, L.ACT_SILU, L.UPA_F32, None, st]

    def pool(**kw):
        names = ["x", "n", "h", "w", "cin", "ldx", "wp", "bias", "pooled", "cout", "ldp", "act", "dtype", "opts", "stream"]
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return lib.upa_classify_pool(*a)

    einval = [dict(x=None), dict(wp=None), dict(bias=None), dict(pooled=None), dict(n=0), dict(h=0), dict(w=-1), dict(cin=0), dict(cout=0),
              dict(ldx=cin - 4), dict(ldp=cout - 1), dict(cin=30, ldx=32), dict(ldx=34), dict(x=X + 4), dict(dtype=L.UPA_BF16, cin=20, ldx=24)]
    for kw in einval:
        assert pool(**kw) == L.UPA_EINVAL, kw
        assert b"classify_pool" in lib.upa_last_error(), kw
    for kw in (dict(act=L.ACT_RELU), dict(act=7), dict(dtype=L.UPA_U8_BGR_HWC), dict(dtype=9)):
        assert pool(**kw) == L.UPA_EUNSUPPORTED, kw
        assert b"classify_pool" in lib.upa_last_error(), kw
    rows, nc = 2, 8
    z = torch.zeros((rows, nc), device=DEV)
    pr = torch.full((rows, nc), -7.0, device=DEV)
    tk = torch.full((rows, 16), -7, dtype=torch.int32, device=DEV)
    Z, P_, T = z.data_ptr(), pr.data_ptr(), tk.data_ptr()
    for args in ((None, rows, nc, nc, P_, nc, 1, T), (Z, rows, nc, nc, None, nc, 1, T), (Z, rows, nc, nc - 1, P_, nc, 1, T),
                 (Z, rows, nc, nc, P_, nc - 1, 1, T), (Z, 0, nc, nc, P_, nc, 1, T), (Z, rows, 0, nc, P_, nc, 1, T)):
        assert lib.upa_softmax_topk(*args, st) == L.UPA_EINVAL, args
        assert b"softmax_topk" in lib.upa_last_error()
    for args in ((Z, rows, nc, nc, P_, nc, 0, T), (Z, rows, nc, nc, P_, nc, nc + 1, T), (Z, rows, nc, nc, P_, nc, 17, T),
                 (Z, rows, 65537, 65537, P_, 65537, 1, T), (Z, rows, 3, nc, P_, nc, 4, T)):
        assert lib.upa_softmax_topk(*args, st) == L.UPA_EUNSUPPORTED, args
        assert b"softmax_topk" in lib.upa_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((pr == -7).all()) and bool((tk == -7).all()), "a refused call wrote its output"
    assert pool() == 0 and lib.upa_softmax_topk(Z, rows, nc, nc, P_, nc, 5, T, st) == 0  # the unmodified calls are accepted
    torch.cuda.synchronize()
    assert bool((pr == 0.125).all()) and tk.flatten()[:5 * rows].view(rows, 5).tolist() == [[0, 1, 2, 3, 4]] * rows  # (rows, k) rows


# ---- 4. the Classify module ---------------------------------------------------------------------------------------------------------------
def _rules(p, z, top, p_ref, z_ref, what):
    """The three f32 rules: |logits - ref| <= 1e-3, |probs - ref| <= 1e-3, top-5 equal to the reference's."""
    dz, dp = float((z - z_ref).abs().max()), float((p - p_ref).abs().max())
    print(f"{what}: max|logit d| {dz:.3e}, max|prob d| {dp:.3e}")
    assert dz <= TOL and dp <= TOL, (what, dz, dp)
    k = min(z_ref.shape[1], 5)
    want = z_ref.argsort(1, descending=True)[:, :k].to(torch.int32)
    assert torch.equal(top, want), (what, top.tolist(), want.tolist())


@pytest.mark.parametrize("case", C.head_cases(), ids=[c[0] for c in C.head_cases()])
@KC.stop_after_fault
def test_classify_module_f32(case, golden_dir):
    from ultralytics_pro_amd.nn.modules import Classify
    g = np.load(golden_dir / "ops_classify.npz")
    o, x = C.head_case(case)
    m, _ = C.head_case(case, Classify)
    m = m.to(DEV)
    with torch.no_grad():
        po, zo = o(x)
        p, z = m(x.to(DEV))
        torch.cuda.synchronize()
        top = m.top5.cpu()
        assert p.shape == po.shape and z.shape == zo.shape and p.dtype == z.dtype == torch.float32
        _rules(p.cpu(), z.cpu(), top, torch.from_numpy(g[f"{case[0]}_probs"]), torch.from_numpy(g[f"{case[0]}_logits"]), f"{case[0]} vs golden")
        _rules(p.cpu(), z.cpu(), top, po, zo, f"{case[0]} vs oracle")
        m.export = True
        assert torch.equal(m(x.to(DEV)).cpu(), p.cpu())


# ---- 5. whole models ------------------------------------------------------------------------------------------------------------------------
MODELS = ["yolov8n-cls", "yolov11n-cls"]


@functools.lru_cache(maxsize=None)
def _images(n):
    return P.synthetic_images(n, h=224, w=224)


@functools.lru_cache(maxsize=None)
def _oracle(name, smooth, n):
    """(probs, logits) of the CPU checker on the first n synthetic images: computed once, shared, never modified."""
    o = C.ClassificationModel(name + ".yaml")
    P.apply_procedural_weights(o, family=("smooth:" if smooth else "") + name)
    o.fuse()
    with torch.no_grad():
        p, z = o(_images(n))
    return p, z


def _product(name, smooth, dtype=torch.float32):
    from ultralytics_pro_amd.nn.tasks import ClassificationModel
    m = ClassificationModel(name + ".yaml")
    P.apply_procedural_weights(m, family=("smooth:" if smooth else "") + name)
    m = m.to(DEV).fuse()
    if dtype != torch.float32:
        m.set_compute_dtype(dtype)
    return m


@pytest.mark.parametrize("name", MODELS)
@KC.stop_after_fault
def test_model_f32_vs_golden_and_oracle(name, golden_dir):
    g = np.load(golden_dir / f"e2e_{name}.npz")
    m = _product(name, False)
    x = _images(3).to(DEV)
    with torch.no_grad():
        p, z = m(x[:2])
        torch.cuda.synchronize()
        p, z, top = p.cpu().clone(), z.cpu().clone(), m.model[-1].top5.cpu().clone()
        _rules(p, z, top, torch.from_numpy(g["probs"]), torch.from_numpy(g["logits"]), f"{name} vs golden")
        assert np.array_equal(top.numpy(), g["top5"])
        po, zo = _oracle(name, False, 3)
        _rules(p, z, top, po[:2], zo[:2], f"{name} vs oracle")
        # a batch of 3 equals three batches of 1 to the same 1e-3
        p3, z3 = (t.cpu().clone() for t in m(x))
        torch.cuda.synchronize()
        _rules(p3, z3, m.model[-1].top5.cpu(), po, zo, f"{name} batch 3 vs oracle")
        for i in range(3):
            p1, z1 = (t.cpu().clone() for t in m(x[i:i + 1]))
            assert float((z1 - z3[i:i + 1]).abs().max()) <= TOL and float((p1 - p3[i:i + 1]).abs().max()) <= TOL
            assert torch.equal(m.model[-1].top5.cpu(), zo[i:i + 1].argsort(1, descending=True)[:, :5].to(torch.int32))


@pytest.mark.parametrize("dispatch", ["session", "serial", "throughput"])
@pytest.mark.parametrize("name", MODELS)
@KC.stop_after_fault
def test_model_bf16_smooth(name, dispatch):
    po, zo = _oracle(name, True, 2)
    m = _product(name, True, torch.bfloat16)
    x = _images(2).to(DEV).to(torch.bfloat16)
    with torch.no_grad(), _dispatch(dispatch):
        p, z = m(x)
        torch.cuda.synchronize()
    p, z, top = p.cpu(), z.cpu(), m.model[-1].top5.cpu()
    dz, dp = float((z - zo).abs().max()), float((p - po).abs().max())
    print(f"bf16 {name} {dispatch}: max|logit d| {dz:.4f} (logit std {float(zo.std(1).mean()):.2f}), max|prob d| {dp:.4f}")
    assert dp <= 0.05, dp  # the bf16 score tolerance of smoke()
    assert torch.equal(top[:, 0], zo.argmax(1).to(torch.int32)), (top[:, 0].tolist(), zo.argmax(1).tolist())
    worst = BF16_LOGIT_MEASURED[name]
    assert worst is not None, "the measured bf16 logit deviation has not been recorded"
    assert dz <= 2 * worst, (dz, worst)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", MODELS)
@KC.stop_after_fault
def test_model_graph_replay_equals_eager(name, dtype):
    m = _product(name, dtype == torch.bfloat16, dtype)
    x = _images(2).to(DEV).to(dtype)
    with torch.no_grad():
        p, z = m(x)
        torch.cuda.synchronize()
        p, z, top = p.cpu().clone(), z.cpu().clone(), m.model[-1].top5.cpu().clone()
        run = m.compile(x)
        pr, zr = run()
        torch.cuda.synchronize()
        assert torch.equal(pr.cpu(), p) and torch.equal(zr.cpu(), z) and torch.equal(pr._upa_top5.cpu(), top)
        pr.zero_()
        run()
        torch.cuda.synchronize()
        assert torch.equal(run.result[0].cpu(), p)  # the replay itself wrote it


# ---- 6. ClassificationValidator -----------------------------------------------------------------------------------------------------------
@KC.stop_after_fault
def test_classification_validator_exact_fractions():
    """8 images in batches of 3 / 3 / 2; targets from the checker's own ranking: its rank-1 class for images 0, 3, 6, its rank-3 class
    for 1, 4, a class outside its top-5 (rank 8) for 2, 5, 7 -> top1 = 3 / 8, top5 = 5 / 8 exactly."""
    from ultralytics_pro_amd.engine.validator import ClassificationValidator
    name = "yolov11n-cls"
    _, zo = _oracle(name, False, 8)
    order = zo.argsort(1, descending=True)
    rank = [0, 2, 7, 0, 2, 7, 0, 7]
    targets = torch.tensor([int(order[i, r]) for i, r in enumerate(rank)])
    m = _product(name, False)
    x = _images(8)
    batches = [dict(img=x[a:b], cls=targets[a:b]) for a, b in ((0, 3), (3, 6), (6, 8))]
    v = ClassificationValidator(m)
    stats = v(batches)
    want = C.ClassifyMetrics()
    want.process([t.to(torch.int32) for t in (targets[0:3], targets[3:6], targets[6:8])],
                 [order[a:b, :5].to(torch.int32) for a, b in ((0, 3), (3, 6), (6, 8))])
    assert stats == want.results_dict
    assert (stats["metrics/accuracy_top1"], stats["metrics/accuracy_top5"], stats["fitness"]) == (0.375, 0.625, 0.5)
    assert torch.equal(torch.cat(v.pred), order[:, :5].to(torch.int32))
    cm = v.metrics.confusion_matrix
    assert cm.shape == (80, 80) and int(cm.sum()) == 8 and int(np.trace(cm)) == 3
