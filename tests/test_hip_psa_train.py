"""-m gpu: the training forms of the YOLO11 kernels at the C ABI (upa_psa_attention_train_fwd / _bwd, upa_dwconv2d_train_fwd / _bwd)
against the float64 references and operand-derived bounds of tests/psa_train_ref.py, the train-mode composites of
engine/trainer.py (C3k2T, C2PSAT) against float64 autograd of the tests/classify_oracle modules, and whole yolov11n-cls steps against
the imported reference's record (tests/golden/train_yolov11n-cls.npz).

Kernel cases: outputs are NaN-filled buffers with spare columns and images, inputs are channel slices with NaN beside them, every call
runs twice (bit-identical) and, once per test, as a captured graph replay (bit-identical to eager)."""

import functools

import numpy as np
import pytest
import torch

from tests import classify_oracle as C
from tests import classify_train_oracle as T
from tests import kernel_check as KC
from tests import psa_train_ref as PR
from tests.yolo11_kernel_ref import CH, HD, KD, SCALE
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
UPA_EINVAL, UPA_EUNSUPPORTED = -1, -2
FAMILIES = ["uniform", "positive", "impulse", "peaked"]


def _code(dtype):
    return 1 if dtype == BF16 else 0


def _E(dtype):
    return 8 if dtype == BF16 else 4


def _replay(fn):
    """fn() launched once inside a captured graph on a side stream; returns after one replay."""
    DEV = KC.env()[0]
    s = torch.cuda.Stream(device=DEV)
    g = torch.cuda.CUDAGraph()
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fn(s.cuda_stream)
    g.replay()
    torch.cuda.synchronize()


# ---- 1. attention ---------------------------------------------------------------------------------------------------------------------
ATTN_HW = [(1, 1), (2, 2), (7, 7), (7, 9), (8, 8), (5, 13), (10, 13)]  # 1, 4, 49, 63, 64, 65, 130 tokens: below, at, above, across 64


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hw", ATTN_HW, ids=[f"{h}x{w}" for h, w in ATTN_HW])
@KC.stop_after_fault
def test_attention_train_fwd_and_bwd(hw, dtype):
    DEV, L, lib, st = KC.env()
    h, w = hw
    N, E, code = h * w, _E(dtype), _code(dtype)
    scale = PR.f32_scale(SCALE)
    report, graphed = [], False
    for heads in (1, 2, 3):
        for n in (1, 3):
            for family in FAMILIES:
                what = f"{family} n{n} {h}x{w} heads{heads} {dtype}"
                qkv, d_o = PR.attn_inputs(family, n, h, w, heads, dtype)
                qd = KC.slice_buf(qkv, dtype, E)           # qkv is a channel slice: NaN on both sides
                ld = qd.shape[-1]
                qp = qd.data_ptr() + E * qd.element_size()
                C_, ldo = heads * HD, heads * HD + 2 * E
                zero_w = torch.zeros(9, C_, dtype=F32, device=DEV)
                zero_b = torch.zeros(C_, dtype=F32, device=DEV)

                def fwd(stream=st):
                    o = KC.out_buf((n, h, w), ldo, dtype, spare=1)
                    lse = torch.full((n * heads * N + 3,), NAN, dtype=F32, device=DEV)
                    rc = lib.upa_psa_attention_train_fwd(qp, ld, n, h, w, heads, KD, HD, scale, o.data_ptr() + E * o.element_size(), ldo,
                                                         lse.data_ptr(), code, stream)
                    assert rc == 0, lib.upa_last_error()
                    return o, lse
                o_buf, lse_buf = KC.twice(fwd, what + " fwd")
                torch.cuda.synchronize()
                o = KC.payload(o_buf, n, C_, what + " o", offset=E)
                lse = lse_buf.cpu()
                assert bool(torch.isnan(lse[n * heads * N:]).all()), "lse wrote past its rows"
                lse = lse[:n * heads * N].view(n, heads, N)
                # o equals upa_psa_attention with a zero pe, bit for bit
                y = KC.out_buf((n, h, w), ldo, dtype, spare=1)
                rc = lib.upa_psa_attention(qp, ld, n, h, w, heads, KD, HD, scale, zero_w.data_ptr(), zero_b.data_ptr(),
                                           y.data_ptr() + E * y.element_size(), ldo, code, st)
                assert rc == 0, lib.upa_last_error()
                torch.cuda.synchronize()
                assert KC.same_bits(y, o_buf), what + ": train forward differs from upa_psa_attention with zero pe"
                r = PR.attn_fwd_ref(qkv, heads, scale)
                KC.check_bound(lse.to(F64), r["lse"], r["b_lse"], what + " lse", report)
                # backward from the forward's own o and lse (its inputs as given)
                dod = KC.slice_buf(d_o, dtype, E)
                ldd = dod.shape[-1]
                dop = dod.data_ptr() + E * dod.element_size()
                op = o_buf.data_ptr() + E * o_buf.element_size()
                lddq = heads * CH + 2 * E

                def bwd(stream=st):
                    g = KC.out_buf((n, h, w), lddq, dtype, spare=1)
                    rc = lib.upa_psa_attention_bwd(qp, ld, op, ldo, lse_buf.data_ptr(), dop, ldd, g.data_ptr() + E * g.element_size(), lddq,
                                                   n, h, w, heads, KD, HD, scale, None, 0, code, stream)
                    assert rc == 0, lib.upa_last_error()
                    return g
                g_buf = KC.twice(bwd, what + " bwd")
                torch.cuda.synchronize()
                got = KC.payload(g_buf, n, heads * CH, what + " dqkv", offset=E)
                ref, bound = PR.attn_bwd_ref(qkv, o.to(F64), lse.to(F64), d_o, heads, scale, dtype)
                KC.check_bound(got.to(F64), ref, bound, what + " dqkv", report)
                if not graphed and family == "uniform" and heads == 2:
                    graphed = True
                    outs = {}

                    def both(stream):
                        outs["f"] = fwd(stream)
                        outs["b"] = bwd(stream)
                    _replay(both)
                    assert KC.same_bits(outs["f"][0], o_buf) and KC.same_bits(outs["f"][1], lse_buf) and KC.same_bits(outs["b"], g_buf), \
                        what + ": graph replay differs from eager"
    assert graphed
    KC.print_report(report, f"attention train {h}x{w} {dtype}")


# ---- 2. depthwise ---------------------------------------------------------------------------------------------------------------------
DW_HW = [(1, 1), (1, 5), (2, 2), (3, 7), (7, 7), (20, 21)]


def _dw_call(x, dz, wt, dtype, acc_dx, acc_dw, with_dx=True, with_dw=True, stream=None, w_off=0, prev=None):
    """One forward + one backward on channel slices (NaN on both sides).  Returns (z_buf, dx_buf, dw_buf)."""
    DEV, L, lib, st = KC.env()
    st = st if stream is None else stream
    n, h, w, c = x.shape
    E, code = _E(dtype), _code(dtype)
    xd, dzd = KC.slice_buf(x, dtype, E), KC.slice_buf(dz, dtype, E)
    ld = xd.shape[-1]
    es = xd.element_size()
    wfull = torch.full((w_off + c * 9 + 4,), NAN, dtype=F32)
    wfull[w_off:w_off + c * 9] = wt.reshape(-1)
    wd = wfull.to(DEV)
    wp = wd.data_ptr() + 4 * w_off
    ldz = c + 2 * E
    z = KC.out_buf((n, h, w), ldz, dtype, spare=1)
    rc = lib.upa_dwconv2d_train_fwd(xd.data_ptr() + E * es, n, h, w, c, ld, wp, z.data_ptr() + E * es, ldz, code, st)
    assert rc == 0, lib.upa_last_error()
    dx = KC.out_buf((n, h, w), ldz, dtype, spare=1)
    dw = torch.full((c * 9 + 8,), NAN, dtype=F32, device=DEV)
    if prev is not None:
        if acc_dx:
            dx[:n, ..., E:E + c] = prev[0].to(dtype).to(DEV)
        if acc_dw:
            dw[4:4 + c * 9] = prev[1].reshape(-1).to(DEV)
    nws = lib.upa_dwconv2d_bwd_workspace_bytes(c)
    ws = torch.full((nws // 4,), NAN, dtype=F32, device=DEV)
    rc = lib.upa_dwconv2d_bwd(xd.data_ptr() + E * es, dzd.data_ptr() + E * es, n, h, w, c, ld, ld, wp,
                              dx.data_ptr() + E * es if with_dx else None, ldz, acc_dx, dw.data_ptr() + 16 if with_dw else None, acc_dw,
                              ws.data_ptr(), nws, code, st)
    assert rc == 0, lib.upa_last_error()
    return z, dx, dw, (xd, dzd, wd, ws)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("hw", DW_HW, ids=[f"{h}x{w}" for h, w in DW_HW])
@KC.stop_after_fault
def test_depthwise_train_fwd_and_bwd(hw, dtype):
    h, w = hw
    report, E = [], _E(dtype)
    for c in (8, 64, 72, 128):
        for n in (1, 3):
            for family in FAMILIES if c in (8, 72) else ["uniform"]:
                what = f"dw {family} n{n} {h}x{w} c{c} {dtype}"
                x, dz, wt = PR.dw_inputs(family, n, h, w, c, dtype)
                prev = (P.uniform("dwtrain:prevx:" + what, (n, h, w, c), -1.0, 1.0).to(dtype).float(),
                        P.uniform("dwtrain:prevw:" + what, (c, 1, 3, 3), -1.0, 1.0))
                for acc in (0, 1):
                    run = lambda: _dw_call(x, dz, wt, dtype, acc, acc, prev=prev)[:3]  # noqa: E731
                    z_b, dx_b, dw_b = KC.twice(run, what)
                    torch.cuda.synchronize()
                    z = KC.payload(z_b, n, c, what + " z", offset=E)
                    dx = KC.payload(dx_b, n, c, what + " dx", offset=E)
                    dwc = dw_b.cpu()
                    assert bool(torch.isnan(dwc[:4]).all()) and bool(torch.isnan(dwc[4 + c * 9:]).all()), what + ": dw wrote outside"
                    rz, bz = PR.dw_fwd_ref(x, wt, dtype)
                    rdx, bdx, rdw, bdw = PR.dw_bwd_ref(x, dz, wt, prev[0] if acc else None, prev[1] if acc else None, dtype)
                    KC.check_bound(z.to(F64), rz, bz, what + " z", report)
                    KC.check_bound(dx.to(F64), rdx, bdx, what + f" dx acc={acc}", report)
                    KC.check_bound(dwc[4:4 + c * 9].view(c, 1, 3, 3).to(F64), rdw, bdw, what + f" dw acc={acc}", report)
    KC.print_report(report, f"depthwise train {h}x{w} {dtype}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_depthwise_null_outputs_head_slice_and_graph(dtype):
    """dx = NULL and dw = NULL leave the other buffer's sentinels; the per-head form (the v slice of head 1 of a 2-head qkv: 64 of 256
    channels, weight pointer moved by 64 * 9 floats, dx accumulated into the dv slice of a dqkv buffer) and one graph replay."""
    DEV, L, lib, st = KC.env()
    E, code = _E(dtype), _code(dtype)
    n, h, w, c = 2, 7, 7, 64
    x, dz, wt = PR.dw_inputs("uniform", n, h, w, c, dtype)
    rdx, bdx, rdw, bdw = PR.dw_bwd_ref(x, dz, wt, out_dtype=dtype)
    _, dx_b, dw_b, _keep = _dw_call(x, dz, wt, dtype, 0, 0, with_dx=False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx_b.float()).all().cpu()), "dx = NULL but dx was written"
    KC.check_bound(dw_b.cpu()[4:4 + c * 9].view(c, 1, 3, 3).to(F64), rdw, bdw, "dw alone")
    _, dx_b, dw_b, _keep = _dw_call(x, dz, wt, dtype, 0, 0, with_dw=False)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw_b).all().cpu()), "dw = NULL but dw was written"
    KC.check_bound(KC.payload(dx_b, n, c, "dx alone", offset=E).to(F64), rdx, bdx, "dx alone")
    # the per-head slice form
    heads, hh = 2, 1
    qkv = torch.full((n, h, w, heads * CH), NAN, dtype=dtype)
    dqkv = torch.full((n, h, w, heads * CH), NAN, dtype=dtype)
    c0 = hh * CH + 2 * KD
    prev = P.uniform("dwtrain:dv", (n, h, w, c), -1.0, 1.0).to(dtype).float()
    qkv[..., c0:c0 + HD], dqkv[..., c0:c0 + HD] = x.to(dtype), prev.to(dtype)
    wall = torch.full((heads * HD, 1, 3, 3), NAN, dtype=F32)
    wall[hh * HD:(hh + 1) * HD] = wt
    qd, gd, wd, dzd = qkv.to(DEV), dqkv.to(DEV), wall.to(DEV), dz.to(dtype).to(DEV)
    dwd = torch.full((heads * HD * 9,), NAN, dtype=F32, device=DEV)
    nws = lib.upa_dwconv2d_bwd_workspace_bytes(HD)
    ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    es = qd.element_size()
    z = KC.out_buf((n, h, w), heads * HD, dtype, spare=1)

    def call(stream, gbuf, dwbuf, zbuf):
        rc = lib.upa_dwconv2d_train_fwd(qd.data_ptr() + c0 * es, n, h, w, HD, heads * CH, wd.data_ptr() + hh * HD * 36,
                                        zbuf.data_ptr() + hh * HD * es, heads * HD, code, stream)
        assert rc == 0, lib.upa_last_error()
        rc = lib.upa_dwconv2d_bwd(qd.data_ptr() + c0 * es, dzd.data_ptr(), n, h, w, HD, heads * CH, HD, wd.data_ptr() + hh * HD * 36,
                                  gbuf.data_ptr() + c0 * es, heads * CH, 1, dwbuf.data_ptr() + hh * HD * 36, 0, ws.data_ptr(), nws, code, stream)
        assert rc == 0, lib.upa_last_error()
    call(st, gd, dwd, z)
    torch.cuda.synchronize()
    rz, bz = PR.dw_fwd_ref(x, wt, dtype)
    KC.check_bound(KC.payload(z, n, HD, "head slice z", offset=hh * HD).to(F64), rz, bz, "head slice z")
    rdx, bdx, _, _ = PR.dw_bwd_ref(x, dz, wt, prev, None, dtype)
    KC.check_bound(KC.payload(gd, n, HD, "head slice dv", offset=c0).to(F64), rdx, bdx, "head slice dv")
    dwc = dwd.cpu().view(heads * HD, 9)
    assert bool(torch.isnan(dwc[:hh * HD]).all()), "wrote another head's weight gradient"
    KC.check_bound(dwc[hh * HD:].view(HD, 1, 3, 3).to(F64), rdw, bdw, "head slice dw")
    g2, dw2, z2 = dqkv.to(DEV), torch.full_like(dwd, NAN), KC.out_buf((n, h, w), heads * HD, dtype, spare=1)
    _replay(lambda s: call(s, g2, dw2, z2))
    assert KC.same_bits(g2, gd) and KC.same_bits(dw2, dwd) and KC.same_bits(z2, z), "graph replay differs from eager"


@KC.stop_after_fault
def test_refusals_launch_nothing():
    """Every refused call leaves every buffer's sentinel bits (the host-side list of tests/test_psa_train_ref.py, on device memory)."""
    DEV, L, lib, st = KC.env()
    buf = torch.full((1 << 16,), -7.0, dtype=F32, device=DEV)
    p = buf.data_ptr()
    o, o2, o3 = p + (1 << 16), p + (2 << 16), p + (3 << 16)
    s = float(SCALE)
    nws = lib.upa_dwconv2d_bwd_workspace_bytes(8)
    fwd = lambda q=p, ld=128, n=1, h=2, w=2, hd=1, kd=32, d=64, out=o, ldo=64, lse=o2, dt=0: lib.upa_psa_attention_train_fwd(  # noqa: E731
        q, ld, n, h, w, hd, kd, d, s, out, ldo, lse, dt, st)
    bwd = lambda q=p, ld=128, oo=o, ldo=64, lse=o2, do=o + 4096, ldd=64, dq=o3, lddq=128, n=1, h=2, w=2, hd=1, kd=32, d=64, dt=0: \
        lib.upa_psa_attention_bwd(q, ld, oo, ldo, lse, do, ldd, dq, lddq, n, h, w, hd, kd, d, s, None, 0, dt, st)  # noqa: E731
    dwf = lambda x=p, n=1, h=2, w=2, c=8, ldx=8, wt=o2, z=o, ldz=8, dt=0: lib.upa_dwconv2d_train_fwd(x, n, h, w, c, ldx, wt, z, ldz, dt, st)  # noqa: E731
    dwb = lambda x=p, dz=p + 4096, n=1, h=2, w=2, c=8, ldx=8, lddz=8, wt=o2, dx=o, lddx=8, dw=o3, ws=o3 + 4096, nw=nws, dt=0: \
        lib.upa_dwconv2d_bwd(x, dz, n, h, w, c, ldx, lddz, wt, dx, lddx, 0, dw, 0, ws, nw, dt, st)  # noqa: E731
    einval = [fwd(q=None), fwd(out=None), fwd(lse=None), fwd(ld=127), fwd(ldo=63), fwd(n=0), fwd(out=p + 64),
              bwd(q=None), bwd(oo=None), bwd(lse=None), bwd(do=None), bwd(dq=None), bwd(ld=120), bwd(lddq=127), bwd(ldo=8), bwd(ldd=8),
              bwd(dq=p + 64),
              dwf(x=None), dwf(wt=None), dwf(z=None), dwf(c=6), dwf(ldx=4), dwf(ldz=10), dwf(x=p + 4), dwf(z=p + 32),
              dwb(dz=None), dwb(dx=None, dw=None), dwb(wt=None), dwb(x=None), dwb(ws=None), dwb(nw=nws - 4), dwb(lddz=6), dwb(lddx=9),
              dwb(dx=p + 4096 + 32)]
    assert einval == [UPA_EINVAL] * len(einval), einval
    unsupported = [fwd(kd=16), fwd(d=32), fwd(dt=2), bwd(kd=64), bwd(d=128), bwd(dt=3), dwf(dt=2), dwb(dt=7)]
    assert unsupported == [UPA_EUNSUPPORTED] * len(unsupported), unsupported
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all()), "a refused call wrote a buffer"
    assert fwd() == 0 and dwf() == 0 and dwb() == 0  # the unmodified calls are accepted
    torch.cuda.synchronize()


# ---- 3. composites ----------------------------------------------------------------------------------------------------------------------
def _composite(kind, shape):
    """(HIP module on the device, its float64 oracle twin, T class name) with the same procedural weights."""
    from ultralytics_pro_amd.nn.modules import block as B
    n, c, h, w = shape
    if kind == "c2psa":
        mk = lambda mod: mod.C2PSA(c, c, 1)  # noqa: E731
    else:
        mk = lambda mod: mod.C3k2(c, c, 1, kind == "c3k2-c3k")  # noqa: E731
    from tests import yolo11_oracle as Y
    hip, ora = mk(B), mk(Y)
    torch.manual_seed(0)
    sd = {}
    for k, v in ora.state_dict().items():
        if not v.dtype.is_floating_point:
            sd[k] = v
        elif k.endswith("running_var"):
            sd[k] = P.uniform(f"comp:{kind}:{shape}:{k}", tuple(v.shape), 0.5, 1.5)
        elif k.endswith("bn.weight"):
            sd[k] = P.uniform(f"comp:{kind}:{shape}:{k}", tuple(v.shape), 0.5, 1.5)
        else:
            fan = max(1, int(np.prod(v.shape[1:])))
            sd[k] = P.uniform(f"comp:{kind}:{shape}:{k}", tuple(v.shape), -1.0, 1.0) * (fan ** -0.5 if v.dim() == 4 else 0.5)
    ora.load_state_dict(sd)
    hip.load_state_dict(sd)
    return hip, ora


COMPOSITES = [("c3k2", (2, 64, 6, 6)), ("c3k2", (2, 256, 2, 2)), ("c3k2-c3k", (2, 64, 6, 6)), ("c3k2-c3k", (2, 256, 2, 2)),
              ("c2psa", (2, 256, 2, 2)), ("c2psa", (2, 256, 7, 7)), ("c2psa", (2, 128, 6, 6))]


@pytest.mark.parametrize("kind,shape", COMPOSITES, ids=[f"{k}-{'x'.join(map(str, s))}" for k, s in COMPOSITES])
@KC.stop_after_fault
def test_composite_forward_and_gradients_match_float64_autograd(kind, shape):
    """C3k2T (c3k False / True) and C2PSAT alone, f32: forward, input gradient and every parameter gradient against float64 autograd of
    the oracle module in train mode.  Gates: the relative-norm gates tests/test_hip_classify_train.py holds the f32 step to - 2e-2 on
    each gradient's norm (parameters whose norm is above 1e-3 of the largest) - and, as a relative l2 DISTANCE (stricter than a norm
    gate: it sees a wrong direction), 2e-2 on the forward, the input gradient and every such parameter gradient."""
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.engine import trainer as TR
    DEV = KC.env()[0]
    hip, ora = _composite(kind, shape)
    x = P.uniform(f"comp:x:{kind}:{shape}", shape, -1.0, 1.0)
    dy = P.uniform(f"comp:dy:{kind}:{shape}", shape, -1.0, 1.0)
    ora = ora.double().train()
    xo = x.double().requires_grad_(True)
    yo = ora(xo)
    (yo * dy.double()).sum().backward()
    hip = hip.to(DEV).train()
    for p_ in hip.parameters():
        p_.grad = torch.zeros_like(p_)
    ctx = TR._Ctx(DEV, F32, 1)
    op = (TR.C2PSAT if kind == "c2psa" else TR.C3k2T)(ctx, hip, "m")
    pool = R.BufferPool()
    with R.static_buffers(pool):
        for cv in op.convs():
            cv.pack()
        xd = R.to_nhwc(x.to(DEV), F32, key=("test", "x"))
        y = op.forward(xd)
        dyd = R.to_nhwc(dy.to(DEV), F32, key=("test", "dy"))
        dx = R.alloc_nhwc(*shape, F32, DEV, key=("test", "dx"))
        op.backward(dyd, dx, False)
        for side in ctx.wgrad_streams:
            torch.cuda.current_stream(DEV).wait_stream(side)
        torch.cuda.synchronize()

    def dist(a, b):
        return float((a.double().cpu() - b).norm() / b.norm().clamp_min(1e-300))
    d_y, d_x = dist(y, yo.detach()), dist(dx, xo.grad)
    print(f"{kind} {shape}: forward {d_y:.2e}, dx {d_x:.2e}")
    assert d_y <= 2e-2 and d_x <= 2e-2
    named, ref = dict(hip.named_parameters()), dict(ora.named_parameters())
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


# ---- 4. whole steps of yolov11n-cls -----------------------------------------------------------------------------------------------------
NAME = "yolov11n-cls"
ATTN_KEYS = ["model.9.m.0.attn.pe.conv.weight", "model.9.m.0.attn.pe.bn.weight", "model.9.m.0.attn.pe.bn.bias", "model.9.m.0.attn.qkv.bn.weight"]
HEAD_KEYS = ["model.10.linear.weight", "model.10.linear.bias", "model.10.conv.bn.weight", "model.10.conv.bn.bias", "model.10.conv.conv.weight"]
# bf16 gates on loss / gradient norm = twice the worst measured over both steps of case a on an MI355X against the reference's record:
# loss 1.558 % / 2.143 % off at steps 0 / 1, gradient norm 0.577 % / 0.580 % (bf16 rounding differs per kernel tile: not derivable)
BF16_LOSS_RTOL, BF16_NORM_RTOL = 2 * 0.02143, 2 * 0.00580


def _trainer(nc, dtype=F32, **kw):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine.trainer import ClassificationTrainer
    from ultralytics_pro_amd.nn.tasks import ClassificationModel
    m = ClassificationModel(NAME + ".yaml", nc=nc)
    P.apply_procedural_weights(m, family=NAME)
    return m, ClassificationTrainer(m, dtype=dtype, device=DEV, yolo11=True, **kw)


@functools.lru_cache(maxsize=None)
def _batch(case, step):
    from tests.hip_utils import DEV
    b = T.golden_batch(case, step)
    return b["img"].to(DEV), {"cls": b["cls"]}


@pytest.mark.parametrize("case,dtype", [("a", F32), ("b", F32), ("a", BF16)], ids=["a-f32", "b-f32", "a-bf16"])
@KC.stop_after_fault
def test_training_step_matches_reference_golden(case, dtype, golden_dir):
    """Whole steps of yolov11n-cls against the imported reference's record.  f32: the tolerances of
    tests/test_hip_classify_train.py::test_training_step_matches_reference_golden unchanged (loss 2e-3, gradient norm 3e-3, per-parameter
    gradient norms 2e-2, head and attention gradients 5e-3 + 1e-5 max, stem weight 2e-5 abs, running statistics 2e-3, EMA sums
    1e-3 + 1e-2).  bf16: loss / gradient norm within BF16_LOSS_RTOL / BF16_NORM_RTOL, median per-parameter norm error 15 %.
    Measured on an MI355X: f32 loss within 6e-7 relative, gradient norm within 4.3e-5, per-parameter gradient norms within 3.3e-5 (cases a
    and b); bf16 median per-parameter norm error 1.7 % at step 0."""
    G = np.load(golden_dir / f"train_{NAME}.npz")
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
        print(f"case {case} {dtype} step {step}: loss {float(items[0]):.6f} (ref {float(ref_loss[0]):.6f}, rel "
              f"{abs(float(items[0]) - float(ref_loss[0])) / float(ref_loss[0]):.3e}) |grad| {norm:.4f} (ref {ref_norm:.4f}, rel "
              f"{abs(norm - ref_norm) / ref_norm:.3e})")
        coef = min(1.0, 10.0 / (ref_norm + 1e-6))
        l2 = np.array([float(named[k].grad.double().norm()) * coef for k in keys])
        ref_l2 = G[f"{case}_grad_l2_{step}"]
        big = ref_l2 > 1e-3 * ref_l2.max()
        rel = np.abs(l2[big] - ref_l2[big]) / ref_l2[big]
        print(f"   per-parameter gradient norms: worst {rel.max():.3e} ({np.array(keys)[big][rel.argmax()]}), median {np.median(rel):.3e}")
        rt_items, rt_norm = (2e-3, 3e-3) if f32 else (BF16_LOSS_RTOL, BF16_NORM_RTOL)
        assert items.shape == (1,)
        np.testing.assert_allclose(items.cpu().numpy(), ref_loss, rtol=rt_items)
        assert abs(norm - ref_norm) <= rt_norm * ref_norm
        if f32:
            np.testing.assert_allclose(l2[big], ref_l2[big], rtol=2e-2)
            if case == "a":
                for k in HEAD_KEYS + ATTN_KEYS:
                    want = G[f"a_grad[{k}]_{step}"]
                    got = named[k].grad.cpu().numpy()[:want.shape[0]] * coef
                    if k.endswith("pe.bn.bias"):
                        # proj's BatchNorm (batch statistics) removes any per-channel constant added in front of proj's 1x1 conv, so this
                        # gradient is exactly 0 and the reference's record is its own rounding noise (1e-10): nothing to compare element
                        # by element.  Both must be noise on the scale of the sibling gradient (pe.bn.weight), in the same 1e-5 form.
                        tiny = 1e-5 * float(np.abs(G[f"a_grad[{k[:-4]}weight]_{step}"]).max())
                        assert float(np.abs(want).max()) <= tiny and float(np.abs(got).max()) <= tiny, (k, float(np.abs(got).max()), tiny)
                        continue
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
            np.testing.assert_allclose(sd["model.10.linear.bias"].cpu().numpy(), G[f"{case}_linear_b_{step}"], rtol=0, atol=2e-5)
            fk = [str(k) for k in G[f"{case}_state_keys"]]
            ema = tr.ema_state_dict()
            got = np.array([float(ema[k].double().sum()) for k in fk])
            np.testing.assert_allclose(got, G[f"{case}_ema_sum_{step}"], rtol=1e-3, atol=1e-2)
            got = np.array([float(sd[k].double().norm()) for k in fk])
            np.testing.assert_allclose(got, G[f"{case}_state_l2_{step}"], rtol=1e-3, atol=1e-4)


@pytest.mark.parametrize("wgrad_streams", [0, 1])
@KC.stop_after_fault
def test_compiled_step_equals_eager_and_two_trainers_agree(wgrad_streams):
    """The hipGraph replay follows the eager step bit for bit (loss, parameters, EMA over four steps, bf16 with the GradScaler) and so
    do two eager trainers from the same start, with the weight gradients on the main stream (0) and on the side stream (1)."""
    runs = []
    for mode in ("eager", "eager", "compiled"):
        m, tr = _trainer(10, BF16, wgrad_streams=wgrad_streams, amp_scaler=True)
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
    m, tr = _trainer(10, F32)
    x, lab = _batch("a", 0)
    losses = [float(tr.step(x, lab).cpu()[0]) for _ in range(8)]
    print("losses:", [f"{v:.4f}" for v in losses])
    assert losses[-1] < losses[0], losses


@KC.stop_after_fault
def test_eval_after_training_sees_the_new_weights():
    """After two steps `model.eval()` logits equal the CPU oracle's eval logits from the trainer's current weights within the 1e-3 of
    tests/test_hip_classify.py; a forward BEFORE training fills the packed caches (pe's folded depthwise weights among them)."""
    m, tr = _trainer(10, F32)
    x, lab = _batch("a", 0)
    with torch.no_grad():
        m.eval()
        z0 = m(x)[1].cpu().clone()
    for s in (0, 1):
        tr.step(*_batch("a", s))
    torch.cuda.synchronize()
    o = C.ClassificationModel(NAME + ".yaml", nc=10)
    o.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
    o.eval()
    with torch.no_grad():
        zo = o(x.cpu())[1]
        m.eval()
        _, z = m(x)
        torch.cuda.synchronize()
        z = z.cpu()
    d, moved = float((z - zo).abs().max()), float((z - z0).abs().max())
    print(f"eval after two steps: max|logit d| vs oracle {d:.3e}; the steps moved the logits by {moved:.3e}")
    assert d <= 1e-3 and moved > 10 * 1e-3
