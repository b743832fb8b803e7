"""-m gpu: the fused depthwise 3x3 + BatchNorm(train) + activation entries (upa_dwconv2d_bn_act_fwd / upa_dwconv_bn_act_bwd) at the C ABI,
on tests/kernel_check.py's conventions: operands are channel slices of NaN-filled buffers with spare channels and a spare image, every
call runs twice and once as a graph replay (bit-identical), refusals leave their buffers untouched.

The kernels tile a map in bands of R = 8 rows and tiles of T = 16 columns: widths 1, T - 1, T, T + 1, 2 T + 1 and heights 1, 2, 3, R + 1,
2 R + 1 put a seam, a partial tile and a one-pixel tile in every position.

The gate is tests/dw_train_ref.py, the float64 reference pinned to autograd by tests/test_dw_train_ref.py: z from x and w; mean, var, the
running statistics and y from the stored z; dgamma, dbeta, dx and dw from x, dy and the stored z, mean and var, with the bound of dz carried
through the taps.  The fused entries are held to the bounds of a dz kept in float32, the composed form on the same inputs to the same
bounds plus its stored dz's rounding.  Measured on MI355X (worst error / bound): f32 0.36 - 0.47 (the running statistics lead), bf16 1.000
(exact ties of the bf16 store of y).  The summation order of z did not change: it is bit-equal to upa_dwconv2d_train_fwd.  On top of the
reference, the fused entries are held to the older kernels:
  z        the bits of upa_dwconv2d_train_fwd (the same fmaf chain; a tap outside the image adds an exact zero);
  mean/var tests/train_ref.bn_stats_ref of the stored z, the bound of tests/test_hip_train_kernels.py with the fused kernel's own number of
           float32 terms in front of float64: a thread's ceil(R T / slots) ceil(w / T) pixels, then the `slots` threads of a workgroup;
  y        the bits of upa_bn_act_fwd on (z, mean, var): it IS that launch;
  dgamma, dbeta   the bits of upa_bn_act_bwd (the same two launches);
  dx, dw   f32: dz in LDS is the value upa_bn_act_bwd stores, so dx carries the bits of upa_dwconv2d_bwd on that dz, and dw - another
           partition of the same sum - stays inside tests/psa_train_ref.dw_bwd_ref's bound on it.  bf16: the composed form rounds dz
           to bf16 and the fused one does not; the two differ by at most 2^-8 |dz| per element, carried through the taps
           (dx: sum |w| 2^-8 |dz| + the store's half ulp on each side; dw: sum 2^-8 |dz| |x|) on top of the same bounds."""

import numpy as np
import pytest
import torch

from tests import dw_train_ref as DR
from tests import kernel_check as KC
from tests import psa_train_ref as PR
from tests import train_ref as TR
from tests.yolo11_kernel_ref import CH, HD, KD, SCALE

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
UPA_EINVAL, UPA_EUNSUPPORTED = -1, -2
T_, R_ = 16, 8
U24, EPS, MOM = 2.0 ** -24, 1e-3, 0.03
WIDTHS, HEIGHTS = (1, T_ - 1, T_, T_ + 1, 2 * T_ + 1), (1, 2, 3, R_ + 1, 2 * R_ + 1)
# (n, h, w, c): every width and every height, c of 8 / 64 / 72 / 80, n of 1 and 3
SHAPES = [(3, 1, 2 * T_ + 1, 8), (1, 2, T_ - 1, 64), (3, 3, T_, 72), (1, R_ + 1, T_ + 1, 80), (1, 2 * R_ + 1, 1, 80), (3, 2 * R_ + 1, 2 * T_ + 1, 8),
          (1, R_ + 1, 2 * T_ + 1, 64), (1, 2 * R_ + 1, T_ + 1, 72)]
FAMILIES = ("uniform", "positive", "impulse", "constant")


def _inputs(family, shape, dtype):
    """x, dy (n, h, w, c) representable in `dtype`, w (c, 1, 3, 3), gamma, beta, running statistics (f32)."""
    from ultralytics_pro_amd.utils import procedural as P
    n, h, w, c = shape
    tag = f"dwbn:{family}:{shape}"
    lo = 0.0 if family == "positive" else -1.0
    x = P.uniform(tag + ":x", shape, lo, 1.0)
    dy = P.uniform(tag + ":dy", shape, lo, 1.0)
    if family == "impulse":  # lit pixels on both sides of every seam and at the corners, different per image
        mask = torch.zeros(n, h, w, 1)
        ys = {0, h - 1} | {y for s in range(R_, h, R_) for y in (s - 1, s)}
        xs = {0, w - 1} | {v for s in range(T_, w, T_) for v in (s - 1, s)}
        for b in range(n):
            for i, yy in enumerate(sorted(ys)):
                for j, xx in enumerate(sorted(xs)):
                    if (i + j + b) % 2 == 0:
                        mask[b, yy, xx] = 1.0
        x, dy = x * mask, dy * mask
    elif family == "constant":
        x, dy = torch.full(shape, 0.75), torch.full(shape, -0.5)
    x, dy = x.to(dtype).float(), dy.to(dtype).float()
    wt = P.uniform(tag + ":w", (c, 1, 3, 3), -1.0, 1.0)
    gamma, beta = P.uniform(tag + ":g", (c,), 0.5, 1.5), P.uniform(tag + ":b", (c,), -0.5, 0.5)
    return x, dy, wt, gamma, beta, P.uniform(tag + ":rm", (c,), -0.5, 0.5), P.uniform(tag + ":rv", (c,), 0.5, 1.5)


def _case(shape, dtype, act, family, acc, report, graph=False):
    DEV, L, lib, st = KC.env()
    n, h, w, c = shape
    E, code, bf = (8, 1, True) if dtype == BF16 else (4, 0, False)
    es = 2 if bf else 4
    npix = n * h * w
    what = f"dwbn {shape} {dtype} act={act} {family} acc={acc}"
    x, dy, wt, gamma, beta, rm0, rv0 = _inputs(family, shape, dtype)
    X, DY = KC.slice_buf(x, dtype, E, spare=1), KC.slice_buf(dy, dtype, E, spare=1)
    ld = c + 2 * E
    off = lambda t: t.data_ptr() + E * es  # noqa: E731
    wd, gd, bd = wt.to(DEV), gamma.to(DEV), beta.to(DEV)
    nwf, nwb = lib.upa_dwconv2d_bn_act_fwd_workspace_bytes(n, h, w, c), lib.upa_dwconv_bn_act_bwd_workspace_bytes(n, h, w, c)
    bands = n * -(-h // R_)
    assert nwf == bands * 2 * c * 4 and nwb == bands * c * 9 * 4
    red = torch.zeros(lib.upa_channel_reduce_workspace_bytes(c) // 8, dtype=F64, device=DEV)

    run0 = [torch.cat([v, torch.full((2,), NAN)]).to(DEV) for v in (rm0, rv0)]  # (device templates: a clone is capturable, an upload is not)

    def fwd(stream=st):
        z, y = KC.out_buf((n, h, w), ld, dtype, spare=1), KC.out_buf((n, h, w), ld, dtype, spare=1)
        stats = [torch.full((c + 2,), NAN, dtype=F32, device=DEV) for _ in range(2)] + [v.clone() for v in run0]
        ws = torch.full((nwf // 4 + 4,), NAN, dtype=F32, device=DEV)
        rc = lib.upa_dwconv2d_bn_act_fwd(off(X), n, h, w, c, ld, wd.data_ptr(), off(z), ld, MOM, *[s.data_ptr() for s in stats], gd.data_ptr(),
                                         bd.data_ptr(), EPS, act, off(y), ld, ws.data_ptr(), nwf, code, stream)
        assert rc == 0, lib.upa_last_error()
        return (z, y, ws) + tuple(stats)
    z_b, y_b, ws_f, mean_d, var_d, rm_d, rv_d = KC.twice(fwd, what + " fwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws_f.cpu()[nwf // 4:]).all()), what + ": wrote past the forward workspace"
    for v in (mean_d, var_d, rm_d, rv_d):
        assert bool(torch.isnan(v.cpu()[c:]).all()) and bool(torch.isfinite(v.cpu()[:c]).all()), what + ": statistics vector"
    # z: the bits of upa_dwconv2d_train_fwd
    z2 = KC.out_buf((n, h, w), ld, dtype, spare=1)
    assert lib.upa_dwconv2d_train_fwd(off(X), n, h, w, c, ld, wd.data_ptr(), off(z2), ld, code, st) == 0, lib.upa_last_error()
    torch.cuda.synchronize()
    assert KC.same_bits(z_b, z2), what + ": z differs from upa_dwconv2d_train_fwd"
    z = KC.payload(z_b, n, c, what + " z", offset=E)
    # tests/dw_train_ref.py: z from x and w; the statistics, the running statistics and y from the stored z, mean and var.  `terms`: the
    # fused kernel's longest float32 chain, from the shapes - a thread's ceil(R T / slots) ceil(w / T) pixels, then a workgroup's slots
    cgl = min(c // E, -(-(c // E) // -(-(c // E) // 16)))
    slots = 256 // cgl
    terms = -(-(R_ * T_) // slots) * -(-w // T_) + slots
    got_m, got_v = mean_d.cpu()[:c], var_d.cpu()[:c]
    F = DR.forward_ref(x, wt, gamma, beta, EPS, act, rm0, rv0, MOM, dtype=dtype, z=z, mean=got_m, var=got_v, terms=terms)
    KC.check_bound(z.to(F64), F["z"], F["b_z"], what + " z", report)
    KC.check_bound(got_m.to(F64), F["mean"], F["b_mean"], what + " mean", report)
    KC.check_bound(got_v.to(F64), F["var"], F["b_var"], what + " var", report)
    KC.check_bound(rm_d.cpu()[:c].to(F64), F["running_mean"], F["b_running_mean"], what + " running_mean", report)
    KC.check_bound(rv_d.cpu()[:c].to(F64), F["running_var"], F["b_running_var"], what + " running_var", report)
    # y: the launch of upa_bn_act_fwd on (z, mean, var)
    y2 = KC.out_buf((n, h, w), ld, dtype, spare=1)
    assert lib.upa_bn_act_fwd(off(z_b), npix, c, ld, mean_d.data_ptr(), var_d.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, act, off(y2), ld, None, 0,
                              code, st) == 0, lib.upa_last_error()
    torch.cuda.synchronize()
    assert KC.same_bits(y_b, y2), what + ": y differs from upa_bn_act_fwd"
    KC.check_bound(KC.payload(y_b, n, c, what + " y", offset=E).to(F64), F["y"], F["b_y"], what + " y", report)
    # ---- backward ----
    from ultralytics_pro_amd.utils import procedural as P
    dx0 = P.uniform(what + ":dx0", shape, -1.0, 1.0).to(dtype).float()
    dw0, dg0, db0 = (P.uniform(what + f":{k}", s, -1.0, 1.0) for k, s in (("dw0", (c, 1, 3, 3)), ("dg0", (c,)), ("db0", (c,))))

    g0 = (KC.slice_buf(dx0, dtype, E, spare=1) if acc else KC.out_buf((n, h, w), ld, dtype, spare=1),
          torch.cat([dw0.reshape(-1) if acc else torch.full((c * 9,), NAN), torch.full((3,), NAN)]).to(DEV),
          torch.cat([dg0, torch.full((2,), NAN)]).to(DEV), torch.cat([db0, torch.full((2,), NAN)]).to(DEV))

    def grads():
        return tuple(t.clone() for t in g0)

    def bwd(stream=st):
        dx, dw, dg, db = grads()
        ws = torch.full((nwb // 4 + 4,), NAN, dtype=F32, device=DEV)
        rc = lib.upa_dwconv_bn_act_bwd(off(X), n, h, w, c, ld, off(z_b), off(DY), ld, ld, mean_d.data_ptr(), var_d.data_ptr(), gd.data_ptr(),
                                       bd.data_ptr(), EPS, act, dg.data_ptr(), db.data_ptr(), red.data_ptr(), wd.data_ptr(), dw.data_ptr(), acc,
                                       off(dx), ld, acc, ws.data_ptr(), nwb, code, stream)
        assert rc == 0, lib.upa_last_error()
        return dx, dw, dg, db, ws
    dx_b, dw_b, dg_b, db_b, ws_b = KC.twice(bwd, what + " bwd")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws_b.cpu()[nwb // 4:]).all()), what + ": wrote past the backward workspace"
    # the composed form on the same inputs
    dx_c, dw_c, dg_c, db_c = grads()
    dz_c = KC.out_buf((n, h, w), ld, dtype, spare=1)
    ws_c = torch.empty(lib.upa_dwconv2d_bwd_workspace_bytes(c), dtype=torch.uint8, device=DEV)
    assert lib.upa_bn_act_bwd(off(z_b), off(DY), npix, c, ld, ld, mean_d.data_ptr(), var_d.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, act,
                              off(dz_c), ld, dg_c.data_ptr(), db_c.data_ptr(), 1, red.data_ptr(), code, st) == 0, lib.upa_last_error()
    assert lib.upa_dwconv2d_bwd(off(X), off(dz_c), n, h, w, c, ld, ld, wd.data_ptr(), off(dx_c), ld, acc, dw_c.data_ptr(), acc, ws_c.data_ptr(),
                                ws_c.numel(), code, st) == 0, lib.upa_last_error()
    torch.cuda.synchronize()
    assert KC.same_bits(dg_b, dg_c) and KC.same_bits(db_b, db_c), what + ": dgamma / dbeta differ from upa_bn_act_bwd"
    assert bool(torch.isnan(dw_b.cpu()[c * 9:]).all()) and bool(torch.isnan(dg_b.cpu()[c:]).all())
    dz = KC.payload(dz_c, n, c, what + " dz", offset=E)
    dx = KC.payload(dx_b, n, c, what + " dx", offset=E).to(F64)
    dw = dw_b.cpu()[:c * 9].view(c, 1, 3, 3).to(F64)
    rdx, bdx, rdw, bdw = PR.dw_bwd_ref(x, dz, wt, dx0 if acc else None, dw0 if acc else None, out_dtype=dtype)
    if not bf:
        assert KC.same_bits(dx_b, dx_c), what + ": f32 dx differs from upa_dwconv2d_bwd on the stored dz"
    else:  # the fused dz is the composed one before its rounding to bf16
        h8 = 1.01 * 2.0 ** -8
        adz, ax, aw = dz.to(F64).abs(), x.to(F64).abs(), wt.to(F64).abs()
        ex, ew = torch.zeros_like(adz), torch.zeros(c, 1, 3, 3, dtype=F64)
        for kh in range(3):
            for kw in range(3):
                ex += aw[:, 0, kh, kw] * PR._shift(adz, -(kh - 1), -(kw - 1))
                ew[:, 0, kh, kw] = (adz * PR._shift(ax, kh - 1, kw - 1)).sum(dim=(0, 1, 2))
        bdx = bdx + h8 * ex + h8 * (rdx.abs() + h8 * ex)  # (the second term: the half ulp of the fused store, around its own value)
        bdw = bdw + h8 * ew
    # tests/dw_train_ref.py on the operands the backward read (x, dy, the stored z, mean, var): nothing of the code under test in it.  The
    # fused entries keep dz in float32; the composed form stores it once in `dtype` (the reference's rounding term)
    dg0_, db0_ = (dg0, db0)
    for tag, (gx, gw, gg, gb), dzt in (("fused", (dx_b, dw_b, dg_b, db_b), F32), ("composed", (dx_c, dw_c, dg_c, db_c), dtype)):
        B = DR.backward_ref(x, z, dy, wt, got_m, got_v, gamma, beta, EPS, act, dx0 if acc else None, dw0 if acc else None, dg0_, db0_,
                            out_dtype=dtype, dz_dtype=dzt)
        KC.check_bound(KC.payload(gx, n, c, what + " dx", offset=E).to(F64), B["dx"], B["b_dx"], f"{what} dx {tag} vs dw_train_ref", report)
        KC.check_bound(gw.cpu()[:c * 9].view(c, 1, 3, 3).to(F64), B["dw"], B["b_dw"], f"{what} dw {tag} vs dw_train_ref", report)
        KC.check_bound(gg.cpu()[:c].to(F64), B["dgamma"], B["b_dgamma"], f"{what} dgamma {tag} vs dw_train_ref", report)
        KC.check_bound(gb.cpu()[:c].to(F64), B["dbeta"], B["b_dbeta"], f"{what} dbeta {tag} vs dw_train_ref", report)
    KC.check_bound(dz.to(F64), B["dz"], B["b_dz"], what + " dz composed vs dw_train_ref", report)
    KC.check_bound(dx, rdx, bdx, what + " dx", report)
    KC.check_bound(dw, rdw, bdw, what + " dw", report)
    KC.check_bound(dw_c.cpu()[:c * 9].view(c, 1, 3, 3).to(F64), rdw, PR.dw_bwd_ref(x, dz, wt, None, dw0 if acc else None)[3], what + " dw composed", report)
    if graph:
        outs = {}

        def both(stream):
            outs["f"], outs["b"] = fwd(stream), bwd(stream)
        s = torch.cuda.Stream(device=DEV)
        gr = torch.cuda.CUDAGraph()
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            with torch.cuda.graph(gr, stream=s):
                both(s.cuda_stream)
        gr.replay()
        torch.cuda.synchronize()
        assert all(KC.same_bits(a, b) for a, b in zip(outs["f"], (z_b, y_b, ws_f, mean_d, var_d, rm_d, rv_d))), what + ": forward graph replay"
        # (bwd() clones its gradient templates on every call, so accumulate = 1 replays on the same start values)
        assert all(KC.same_bits(a, b) for a, b in zip(outs["b"], (dx_b, dw_b, dg_b, db_b, ws_b))), what + ": backward graph replay differs from eager"


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n{}_{}x{}_c{}".format(*s))
@KC.stop_after_fault
def test_fused_depthwise_bn_act_forward_and_backward(shape, dtype):
    report = []
    i = SHAPES.index(shape)
    for k, family in enumerate(FAMILIES):
        _case(shape, dtype, (i + k) % 2, family, (i + k // 2) % 2, report, graph=(family == "uniform" and i in (3, 5)))
    _case(shape, dtype, 1 - i % 2, "uniform", 1 - i % 2, report)
    KC.print_report(report, f"dwbn {shape} {dtype}", "comparisons")


@KC.stop_after_fault
def test_refusals_launch_nothing():
    DEV, L, lib, st = KC.env()
    buf = torch.full((1 << 16,), -7.0, dtype=F32, device=DEV)
    p = buf.data_ptr()
    blk = 1 << 14  # bytes between the views below; n 1, 4 x 4, c 8 f32: 512 bytes each
    x, z, y, dy, dx, mean, var, g, b, wt, dw, ws = (p + i * blk for i in range(12))
    # the channel-reduction scratch at its full size (upa_channel_reduce_workspace_bytes: the combined sums sit behind 2048 rows of partials)
    redbuf = torch.full((lib.upa_channel_reduce_workspace_bytes(8) // 8,), -7.0, dtype=F64, device=DEV)
    red = redbuf.data_ptr()

    def fwd(x=x, z=z, y=y, c=8, ldx=8, ldz=8, ldy=8, n=1, h=4, w=4, act=1, dt=0, ws=ws, nw=1 << 14, wt=wt):
        return lib.upa_dwconv2d_bn_act_fwd(x, n, h, w, c, ldx, wt, z, ldz, 0.03, mean, var, None, None, g, b, 1e-3, act, y, ldy, ws, nw, dt, st)

    def bwd(x=x, z=z, dy=dy, dx=dx, c=8, ldx=8, ldz=8, lddy=8, lddx=8, n=1, h=4, w=4, act=1, dt=0, ws=ws, nw=1 << 14, dw=dw, red=red):
        return lib.upa_dwconv_bn_act_bwd(x, n, h, w, c, ldx, z, dy, ldz, lddy, mean, var, g, b, 1e-3, act, g + 64, b + 64, red, wt, dw, 0, dx, lddx, 0,
                                         ws, nw, dt, st)
    einval = [fwd(c=6), fwd(ldx=4), fwd(ldz=10), fwd(ldy=6), fwd(x=x + 4), fwd(z=z + 8), fwd(z=x + 64), fwd(y=x), fwd(y=z + 32), fwd(nw=8),
              fwd(ws=ws + 4), fwd(n=1, h=1, w=1), fwd(x=None), fwd(wt=None), fwd(n=0),
              bwd(c=6), bwd(ldz=4), bwd(lddy=10), bwd(lddx=6), bwd(dy=dy + 4), bwd(dx=z + 32), bwd(dx=dy), bwd(dx=x + 16), bwd(nw=8), bwd(h=1, w=1),
              bwd(dw=None), bwd(red=None)]
    assert einval == [UPA_EINVAL] * len(einval), einval
    unsupported = [fwd(dt=2), fwd(act=2), bwd(dt=3), bwd(act=2)]
    assert unsupported == [UPA_EUNSUPPORTED] * len(unsupported), unsupported
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all()) and bool((redbuf == -7.0).all()), "a refused call wrote a buffer"
    assert bwd(dx=x + 32, ldx=16, lddx=16, h=2) == 0, lib.upa_last_error()  # dx as the other channel slice of x's buffer is accepted
    assert fwd() == 0 and bwd() == 0, lib.upa_last_error()  # and so are the unmodified calls
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_attention_backward_at_400_tokens(dtype):
    """upa_psa_attention_bwd on the map yolov11n's C2PSA sees at 640 pixels: 2 x 128 x 20 x 20 (two heads, 400 tokens - seven streamed
    blocks of 64 keys, the last one ragged), against tests/psa_train_ref.py's bounds.  tests/test_hip_psa_train.py stops at 130 tokens."""
    DEV, L, lib, st = KC.env()
    n, h, w, heads = 2, 20, 20, 2
    N, E, code = h * w, (8 if dtype == BF16 else 4), (1 if dtype == BF16 else 0)
    scale = PR.f32_scale(SCALE)
    report = []
    for family in ("uniform", "peaked"):
        what = f"{family} n{n} {h}x{w} heads{heads} {dtype}"
        qkv, d_o = PR.attn_inputs(family, n, h, w, heads, dtype)
        qd, dod = KC.slice_buf(qkv, dtype, E), KC.slice_buf(d_o, dtype, E)
        es = qd.element_size()
        ld, ldd, ldo, lddq = qd.shape[-1], dod.shape[-1], heads * HD + 2 * E, heads * CH + 2 * E
        o_buf = KC.out_buf((n, h, w), ldo, dtype, spare=1)
        lse_buf = torch.full((n * heads * N + 3,), NAN, dtype=F32, device=DEV)
        assert lib.upa_psa_attention_train_fwd(qd.data_ptr() + E * es, ld, n, h, w, heads, KD, HD, scale, o_buf.data_ptr() + E * es, ldo,
                                               lse_buf.data_ptr(), code, st) == 0, lib.upa_last_error()

        def bwd(stream=st):
            g = KC.out_buf((n, h, w), lddq, dtype, spare=1)
            rc = lib.upa_psa_attention_bwd(qd.data_ptr() + E * es, ld, o_buf.data_ptr() + E * es, ldo, lse_buf.data_ptr(), dod.data_ptr() + E * es,
                                           ldd, g.data_ptr() + E * es, lddq, n, h, w, heads, KD, HD, scale, None, 0, code, stream)
            assert rc == 0, lib.upa_last_error()
            return g
        g_buf = KC.twice(bwd, what + " bwd")
        torch.cuda.synchronize()
        o = KC.payload(o_buf, n, heads * HD, what + " o", offset=E)
        lse = lse_buf.cpu()
        assert bool(torch.isnan(lse[n * heads * N:]).all()), "lse wrote past its rows"
        lse = lse[:n * heads * N].view(n, heads, N)
        r = PR.attn_fwd_ref(qkv, heads, scale)
        KC.check_bound(lse.to(F64), r["lse"], r["b_lse"], what + " lse", report)
        got = KC.payload(g_buf, n, heads * CH, what + " dqkv", offset=E)
        ref, bound = PR.attn_bwd_ref(qkv, o.to(F64), lse.to(F64), d_o, heads, scale, dtype)
        KC.check_bound(got.to(F64), ref, bound, what + " dqkv", report)
    KC.print_report(report, f"attention backward 400 tokens {dtype}")
