"""-m gpu: the training-step kernels of csrc/train.hip (and the entries of conv.hip / elementwise.hip the backward pass uses) called
through the C ABI on channel slices of wider buffers and compared per element with the float64 restatements of tests/train_ref.py.

Buffers, sentinels, the two bit-identical runs, the per-element bounds and the fault latch: the conventions of tests/kernel_check.py:
every view of
one call has its own pitch (c + 2 E, c + 3 E, ...), accumulating outputs are pre-filled with known finite values, per-channel float32
outputs sit at offset 4 of a NaN-filled array eight longer than c.  Each bound is built from the magnitude term train_ref returns next to
the reference; the docstrings carry the derivations.  The `print`s give the worst error / bound of each group (pytest -s)."""

import ctypes as C
import math

import pytest
import torch

from tests import conv_ref as CR
from tests import train_ref as TR
from tests import kernel_check as KC

pytestmark = pytest.mark.gpu

SPARE, PAD = 4, 7.0
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NONE, SILU = TR.ACT_NONE, TR.ACT_SILU
UPA_OK, UPA_EINVAL, UPA_EUNSUPPORTED = 0, -1, -2
U24 = TR.U24
MOM, EPS = 0.03, TR.BN_EPS
NAN = float("nan")


def _opts(**kw):
    from ultralytics_pro_amd import _lib as L
    return L.Opts(**kw)


def _es(dtype):
    return torch.empty(0, dtype=dtype).element_size()


def _rows(t):
    """NCHW -> (pixels, c)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def _nchw(m, n, h, w):
    return m.reshape(n, h, w, -1).permute(0, 3, 1, 2)


class _In:
    """An input view: `mat` (rows, c) at channel offset E of a buffer c + groups * E wide."""

    def __init__(self, mat, dtype, groups=2, poison=False):
        self.rows, self.c = mat.shape
        self.es = _es(dtype)
        E = self.E = 16 // self.es
        self.ld = self.c + groups * E
        self.buf = KC.slice_buf(mat, dtype, E, tail=(groups - 1) * E, fill=NAN if poison else PAD)
        self.ptr = self.buf.data_ptr() + E * self.es


class _Out:
    """An output view: (rows, c) at channel offset E of a NaN-filled buffer c + groups * E wide with SPARE rows more; `prefill`
    (rows, c) for accumulating calls."""

    def __init__(self, rows, c, dtype, groups=3, prefill=None):
        self.rows, self.c, self.dtype = rows, c, dtype
        self.es = _es(dtype)
        E = self.E = 16 // self.es
        self.ld = c + groups * E
        self.buf = (KC.out_buf((rows,), self.ld, dtype, SPARE) if prefill is None else
                    KC.slice_buf(prefill, dtype, E, tail=(groups - 1) * E, spare=SPARE))
        self.ptr = self.buf.data_ptr() + E * self.es

    def untouched(self):
        return bool(torch.isnan(self.buf.float()).all())

    def payload(self, what):
        return KC.payload(self.buf, self.rows, self.c, what, offset=self.E).double()


class _Vec:
    """A float32 per-channel array at offset 4 of a NaN-filled array eight longer."""

    def __init__(self, c, prefill=None):
        self.c = c
        self.buf = KC.out_buf((1,), c + 8, F32, 0)[0] if prefill is None else KC.slice_buf(prefill.float()[None], F32, 4)[0]
        self.ptr = self.buf.data_ptr() + 16

    def payload(self, what):
        return KC.payload(self.buf[None], 1, self.c, what, offset=4)[0].double()


def _dev(t, dtype=F32):
    return t.to(dtype).contiguous().to(KC.env()[0])


def _pair(outs, what):
    """outs: two lists of _Out / _Vec from two runs of one call -> their payloads (first run), after asserting identical bits."""
    for a, b in zip(*outs):
        assert KC.same_bits(a.buf, b.buf), f"{what}: two runs differ"
    return [a.payload(what) for a in outs[0]]


def _out_round(ref, arith, dtype):
    """The bound of a value computed to within `arith` and stored once in `dtype`."""
    if dtype == BF16:
        return arith + TR.half_ulp_bf16(ref.abs() + arith)
    return arith + U24 * ref.abs()


def _reduce_ws(c):
    DEV, L, lib, _ = KC.env()
    return torch.zeros(lib.upa_channel_reduce_workspace_bytes(c) // 8, dtype=F64, device=DEV)


# =====================================================================================================================
# a. channel reductions and the BatchNorm apply kernels
# =====================================================================================================================
def _bn_one(dtype, c, case, report):
    DEV, L, lib, st = KC.env()
    npix, family, act, acc, with_res, running, seed = case
    code = L.dtype_code(dtype)
    what = f"{'bf16' if dtype == BF16 else 'f32'} c{c} npix{npix} {family} act{act} acc{acc} res{int(with_res)} run{int(running)}"
    z, dy, res, gamma, beta = TR.bn_family(family, npix, c, dtype, seed)
    poison = family == "poison"
    Z, DY, RES = _In(z, dtype, 2, poison), _In(dy, dtype, 4, poison), _In(res, dtype, 6, poison)
    rm0, rv0 = torch.linspace(-0.1, 0.1, c), torch.linspace(0.5, 1.5, c)
    g0, b0 = torch.linspace(-1.0, 1.0, c), torch.linspace(2.0, -2.0, c)
    mean, var, run, A1, A2 = TR.bn_stats_ref(z, rm0, rv0, MOM)
    ws = _reduce_ws(c)
    # ---- upa_bn_stats + upa_bn_finalize ----
    outs = []
    for _ in range(2):
        o = [_Vec(c), _Vec(c)] + ([_Vec(c, rm0), _Vec(c, rv0)] if running else [])
        L.check(lib.upa_bn_stats(Z.ptr, npix, c, Z.ld, ws.data_ptr(), code, st), what)
        L.check(lib.upa_bn_finalize(ws.data_ptr(), npix, c, MOM, o[0].ptr, o[1].ptr, o[2].ptr if running else None,
                                    o[3].ptr if running else None, st), what)
        outs.append(o)
    got = _pair(outs, what + " stats")
    dsum = 1.01 * 64 * U24 * A1 / npix
    b_mean = dsum + U24 * mean.abs() + 1e-300
    b_var = 1.01 * 65 * U24 * A2 / npix + 2 * mean.abs() * dsum + dsum * dsum + U24 * var.abs() + 1e-300
    KC.check_bound(got[0], mean, b_mean, what + " mean", report)
    KC.check_bound(got[1], var, b_var, what + " var", report)
    assert float(got[1].min()) >= 0.0, what + ": negative variance"
    if running:
        m = TR.f32(MOM)
        unb = npix / (npix - 1) if npix > 1 else 1.0
        KC.check_bound(got[2], run[0], m * b_mean + 4 * U24 * ((1 - m) * rm0.double().abs() + m * mean.abs()), what + " running mean", report)
        KC.check_bound(got[3], run[1], m * unb * b_var + 5 * U24 * ((1 - m) * rv0.double().abs() + m * unb * var.abs()), what + " running var", report)
    # ---- upa_channel_sum ----
    outs = []
    for _ in range(2):
        o = [_Vec(c, g0 if acc else None)]
        L.check(lib.upa_channel_sum(Z.ptr, npix, c, Z.ld, o[0].ptr, acc, ws.data_ptr(), code, st), what)
        outs.append(o)
    ref = z.double().sum(0) + (g0.double() if acc else 0.0)
    KC.check_bound(_pair(outs, what + " channel_sum")[0], ref, 1.01 * 64 * U24 * A1 + 2 * U24 * ref.abs() + 1e-300, what + " channel_sum", report)
    # ---- upa_bn_act_fwd / upa_bn_act_bwd with the float32-rounded reference statistics ----
    m32, v32 = mean.float(), var.float()
    md, vd, gd, bd = _dev(m32), _dev(v32), _dev(gamma), _dev(beta)
    outs = []
    for _ in range(2):
        o = [_Out(npix, c, dtype, 3)]
        L.check(lib.upa_bn_act_fwd(Z.ptr, npix, c, Z.ld, md.data_ptr(), vd.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, act, o[0].ptr,
                                   o[0].ld, RES.ptr if with_res else None, RES.ld if with_res else 0, code, st), what)
        outs.append(o)
    yr, My = TR.bn_act_fwd_ref(z, m32, v32, gamma, beta, EPS, act, res if with_res else None)
    KC.check_bound(_pair(outs, what + " fwd")[0], yr, _out_round(yr, 4 * TR.C1_FWD_CPU * U24 * My, dtype) + 1e-300, what + " y", report)
    outs = []
    for _ in range(2):
        o = [_Out(npix, c, dtype, 5), _Vec(c, g0 if acc else None), _Vec(c, b0 if acc else None)]
        L.check(lib.upa_bn_act_bwd(Z.ptr, DY.ptr, npix, c, Z.ld, DY.ld, md.data_ptr(), vd.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS, act,
                                   o[0].ptr, o[0].ld, o[1].ptr, o[2].ptr, acc, ws.data_ptr(), code, st), what)
        outs.append(o)
    got = _pair(outs, what + " bwd")
    dz, dgamma, dbeta, Mdz, Sb, Sg, T, Tb, Tg = TR.bn_act_bwd_ref(z, dy, m32, v32, gamma, beta, EPS, act)
    b_dg = 1.01 * (64 + 8) * U24 * Sg + 16 * U24 * Tg
    b_db = 1.01 * (64 + 2) * U24 * Sb + 16 * U24 * Tb
    rstd, xh, _ = TR._bn_u(z, m32, v32, gamma, beta, EPS)
    feed = (gamma.double() * rstd).abs() * (b_db + U24 * dbeta.abs() + xh.abs() * (b_dg + U24 * dgamma.abs())) / npix
    KC.check_bound(got[0], dz, _out_round(dz, 4 * TR.C1_BWD_CPU * U24 * (Mdz + T) + feed, dtype) + 1e-300, what + " dz", report)
    rg, rb = dgamma + (g0.double() if acc else 0.0), dbeta + (b0.double() if acc else 0.0)
    KC.check_bound(got[1], rg, b_dg + U24 * dgamma.abs() + 2 * U24 * rg.abs() + 1e-300, what + " dgamma", report)
    KC.check_bound(got[2], rb, b_db + U24 * dbeta.abs() + 2 * U24 * rb.abs() + 1e-300, what + " dbeta", report)


@pytest.mark.parametrize("dtype,c", [(d, c) for d in (F32, BF16) for c in TR.BN_CHANNELS[d]], ids=lambda v: str(v).replace("torch.", ""))
@KC.stop_after_fault
def test_channel_reductions_and_bn_apply(dtype, c):
    """upa_bn_stats + upa_bn_finalize, upa_channel_sum, upa_bn_act_fwd, upa_bn_act_bwd on slices: channel-group counts that leave
    idle threads (12, 10, 36 / 34) and the launcher's largest (256), every pixel count of TR.BN_NPIX with every family (at 256 groups the two largest counts with two families), the options
    (activation, accumulate, residual, running statistics) walking all sixteen combinations (TR.bn_cases).

    Bounds, u = 2^-24.  channel_reduce_kernel adds at most 64 pixels (16 trips of U = 4) into a float32 partial before folding it
    into float64, so a sum of terms t errs by at most 64 u sum|t| plus c0 u sum|t| for the roundings inside a term (1.01: higher orders):
      sum z      c0 = 0                              mean: 64 u A1 / npix + u |mean| (the float32 store)
      sum z^2    c0 = 1 (the square)                 var:  65 u A2 / npix + 2 |mean| d(mean) + d(mean)^2 + u |var| - the cancellation
                 term is why the `offset` family (z near 100) only holds var to about 0.04 absolute: the float32 squares of 64 pixels
                 are summed before float64 sees them
      running    momentum x the above + the update's four float32 operations
      sum du     c0 = 2 (the derivative's product, the add)     dbeta:  66 u S_beta + 16 u T_beta + the float32 store / accumulate
      sum du xh  c0 = 8 (rstd: add, sqrt, divide; xhat: subtract, multiply; du: multiply; the product; slack 1)
                                                     dgamma: 72 u S_gamma + 16 u T_gamma + store
                 16 u T: SiLU' = s (1 + u (1 - s)) costs the rounding of u (7 roundings through a slope below 1 / 2), the exponential
                 and reciprocal (|u| + 4) and four more operations, all absolute in |dy| (1 + |u|) - see TR.bn_act_bwd_ref.
    y and dz: c1 u M with c1 = 4 x the float32 CPU restatement's worst error / (u M) over these very cases (forward 4.667 -> recorded 5.0,
    kernels allowed 20; backward 6.654 -> 7.0, allowed 28; tests/test_train_ref.py::test_c1_constants); dz also gets what the kernels'
    own sums may differ by, |gamma rstd| (d(dbeta) + |xhat| d(dgamma)) / npix; bf16 outputs add half a bf16 ulp.
    Measured on MI355X (worst error / bound, information only): float32 0.28 - 0.39 (the running statistics and dbeta lead, y and dz stay
    below 0.3); bf16 1.000 on y - exact ties of the output rounding, the arithmetic term being a thousandth of half a bf16 ulp."""
    report = []
    for case in TR.bn_cases(dtype, c):
        _bn_one(dtype, c, case, report)
    KC.print_report(report, f"bn {dtype} c{c}", "comparisons")


@KC.stop_after_fault
def test_reductions_large_grid_switch():
    """npix = 1 500 001 > 1.5 M: reduce_grid's 1024-block form, c = 8 bf16 (24 MB), upa_bn_stats + upa_bn_finalize and upa_bn_act_bwd,
    uniform family and the impulse family (whose first-chunk pixel moves with the grid).  Same bounds as above.
    Measured on MI355X: 0.998 (dz, the bf16 output rounding)."""
    DEV, L, lib, st = KC.env()
    npix, c, dtype = 1500001, 8, BF16
    assert TR.reduce_grid(npix) == 1024 and TR.reduce_grid(npix - 1) == 512
    code = L.dtype_code(dtype)
    report = []
    for family in ("uniform", "impulse"):
        what = f"large grid {family}"
        z, dy, _, gamma, beta = TR.bn_family(family, npix, c, dtype, 77)
        Z, DY = _In(z, dtype, 2), _In(dy, dtype, 4)
        ws = _reduce_ws(c)
        mean, var, _, A1, A2 = TR.bn_stats_ref(z)
        outs = []
        for _ in range(2):
            o = [_Vec(c), _Vec(c)]
            L.check(lib.upa_bn_stats(Z.ptr, npix, c, Z.ld, ws.data_ptr(), code, st), what)
            L.check(lib.upa_bn_finalize(ws.data_ptr(), npix, c, MOM, o[0].ptr, o[1].ptr, None, None, st), what)
            outs.append(o)
        got = _pair(outs, what)
        dsum = 1.01 * 64 * U24 * A1 / npix
        KC.check_bound(got[0], mean, dsum + U24 * mean.abs() + 1e-300, what + " mean", report)
        KC.check_bound(got[1], var, 1.01 * 65 * U24 * A2 / npix + 2 * mean.abs() * dsum + dsum * dsum + U24 * var.abs() + 1e-300, what + " var", report)
        m32, v32 = mean.float(), var.float()
        md, vd, gd, bd = _dev(m32), _dev(v32), _dev(gamma), _dev(beta)
        outs = []
        for _ in range(2):
            o = [_Out(npix, c, dtype, 3), _Vec(c), _Vec(c)]
            L.check(lib.upa_bn_act_bwd(Z.ptr, DY.ptr, npix, c, Z.ld, DY.ld, md.data_ptr(), vd.data_ptr(), gd.data_ptr(), bd.data_ptr(), EPS,
                                       SILU, o[0].ptr, o[0].ld, o[1].ptr, o[2].ptr, 0, ws.data_ptr(), code, st), what)
            outs.append(o)
        got = _pair(outs, what + " bwd")
        dz, dgamma, dbeta, Mdz, Sb, Sg, T, Tb, Tg = TR.bn_act_bwd_ref(z, dy, m32, v32, gamma, beta, EPS, SILU)
        b_dg, b_db = 1.01 * 72 * U24 * Sg + 16 * U24 * Tg, 1.01 * 66 * U24 * Sb + 16 * U24 * Tb
        rstd, xh, _ = TR._bn_u(z, m32, v32, gamma, beta, EPS)
        feed = (gamma.double() * rstd).abs() * (b_db + U24 * dbeta.abs() + xh.abs() * (b_dg + U24 * dgamma.abs())) / npix
        KC.check_bound(got[0], dz, _out_round(dz, 4 * TR.C1_BWD_CPU * U24 * (Mdz + T) + feed, dtype) + 1e-300, what + " dz", report)
        KC.check_bound(got[1], dgamma, b_dg + 2 * U24 * dgamma.abs() + 1e-300, what + " dgamma", report)
        KC.check_bound(got[2], dbeta, b_db + 2 * U24 * dbeta.abs() + 1e-300, what + " dbeta", report)
    KC.print_report(report, "large grid", "comparisons")


# =====================================================================================================================
# b. the one-call forms
# =====================================================================================================================
def _pack(w, dtype):
    DEV, L, lib, _ = KC.env()
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    code = L.dtype_code(dtype)
    packed = torch.empty(lib.upa_conv_packed_weight_bytes(cout, cin, k, code), dtype=torch.uint8)
    wc = w.contiguous().float()
    L.check(lib.upa_pack_conv_weight(wc.data_ptr(), cout, cin, k, code, packed.data_ptr()), "pack")
    return packed.to(DEV)


def _pack_dev(w_dev, cout, cin, k, dtype, flip):
    """upa_pack_conv_weight_dev of a float32 OIHW device tensor; flip = 1: the transposed, flipped weights of the data gradient."""
    DEV, L, lib, st = KC.env()
    code = L.dtype_code(dtype)
    nb = lib.upa_conv_packed_weight_bytes(cin, cout, k, code) if flip else lib.upa_conv_packed_weight_bytes(cout, cin, k, code)
    out = torch.empty(nb, dtype=torch.uint8, device=DEV)
    L.check(lib.upa_pack_conv_weight_dev(w_dev.data_ptr(), cout, cin, k, code, flip, out.data_ptr(), st), "pack_dev")
    return out


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@KC.stop_after_fault
def test_one_call_forms_equal_their_separate_calls(dtype, k):
    """upa_conv2d_bn_act_fwd and upa_conv_bn_act_bwd on 2 x (24 -> 40) x 9 x 13 slice views against the calls they stand for, bit for
    bit: forward against upa_conv2d_bias_act + upa_bn_stats + upa_bn_finalize + upa_bn_act_fwd (no_epi_stats = 1 on both sides) and
    against upa_conv2d_bn_stats + upa_bn_act_fwd (default options); backward against upa_bn_act_bwd + upa_conv2d_wgrad +
    upa_conv2d_bias_act with the flipped weights - on the caller's stream and with the weight gradient on a side stream (joined by a
    device synchronise before dw is read), accumulating into dx and not, and with w_packed_t = NULL (dx stays NaN)."""
    DEV, L, lib, st = KC.env()
    n, cin, cout, h, w, p = 2, 24, 40, 9, 13, k // 2
    code = L.dtype_code(dtype)
    npix = n * h * w
    x, dy, wt = TR.conv_grad_family(n, cin, cout, h, w, k, 1, p, dtype, 31 + k)
    z0, _, res, gamma, beta = TR.bn_family("uniform", npix, cout, dtype, 32 + k)
    X, DY, RES = _In(_rows(x), dtype, 2), _In(_rows(dy), dtype, 4), _In(res, dtype, 6)
    wp = _pack(wt, dtype)
    wdev = _dev(wt)
    wpt = _pack_dev(wdev, cout, cin, k, dtype, 1)
    gd, bd = _dev(gamma), _dev(beta)
    rm0, rv0 = torch.linspace(-0.1, 0.1, cout), torch.linspace(0.5, 1.5, cout)
    ws = _reduce_ws(cout)

    def fwd(mode, opts):
        o = dict(z=_Out(npix, cout, dtype, 3), y=_Out(npix, cout, dtype, 5), m=_Vec(cout), v=_Vec(cout), rm=_Vec(cout, rm0), rv=_Vec(cout, rv0))
        conv = (X.ptr, n, h, w, cin, X.ld, wp.data_ptr(), o["z"].ptr, cout, o["z"].ld, k, 1, p, MOM, o["m"].ptr, o["v"].ptr, o["rm"].ptr, o["rv"].ptr)
        act = (gd.data_ptr(), bd.data_ptr(), EPS, SILU, o["y"].ptr, o["y"].ld, RES.ptr, RES.ld)
        if mode == "one":
            L.check(lib.upa_conv2d_bn_act_fwd(*conv, *act, ws.data_ptr(), code, C.byref(opts), st), "one-call forward")
            return o
        if mode == "stats":
            L.check(lib.upa_conv2d_bn_stats(*conv, ws.data_ptr(), code, C.byref(opts), st), "bn_stats")
        else:
            L.check(lib.upa_conv2d_bias_act(X.ptr, n, h, w, cin, X.ld, wp.data_ptr(), None, o["z"].ptr, cout, o["z"].ld, None, 0, k, 1, p, NONE,
                                            code, C.byref(opts), st), "conv")
            L.check(lib.upa_bn_stats(o["z"].ptr, npix, cout, o["z"].ld, ws.data_ptr(), code, st), "stats")
            L.check(lib.upa_bn_finalize(ws.data_ptr(), npix, cout, MOM, o["m"].ptr, o["v"].ptr, o["rm"].ptr, o["rv"].ptr, st), "finalize")
        L.check(lib.upa_bn_act_fwd(o["z"].ptr, npix, cout, o["z"].ld, o["m"].ptr, o["v"].ptr, *act, code, st), "bn_act_fwd")
        return o

    for one, sep, opts in (("one", "separate", _opts(no_epi_stats=1)), ("one", "stats", _opts())):
        a, b = fwd(one, opts), fwd(sep, opts)
        torch.cuda.synchronize()
        for key in a:
            assert KC.same_bits(a[key].buf, b[key].buf), f"forward {sep}: {key} differs"
            a[key].payload(f"forward {key}")
    zv = a["z"]  # the stored z of the last run: the backward's input, read in place
    md, vd = a["m"], a["v"]
    side = torch.cuda.Stream(device=DEV)
    nws = lib.upa_conv2d_wgrad_workspace_bytes(cin, cout, k)
    g0, b0 = torch.linspace(-1.0, 1.0, cout), torch.linspace(2.0, -2.0, cout)
    dw0 = torch.linspace(-1.0, 1.0, cout * cin * k * k)
    dx0 = TR.stored(torch.linspace(-2.0, 2.0, npix * cin).reshape(npix, cin), dtype)
    opts = _opts()

    def bwd(mode, side_stream, acc_dx, with_dx):
        o = dict(dz=_Out(npix, cout, dtype, 9), dg=_Vec(cout, g0), db=_Vec(cout, b0), dw=_Vec(cout * cin * k * k, dw0),
                 dx=_Out(npix, cin, dtype, 7, dx0 if acc_dx else None))
        wws = torch.empty(nws, dtype=torch.uint8, device=DEV)
        bn = (md.ptr, vd.ptr, gd.data_ptr(), bd.data_ptr(), EPS, SILU, o["dz"].ptr, o["dz"].ld, o["dg"].ptr, o["db"].ptr)
        if mode == "one":
            L.check(lib.upa_conv_bn_act_bwd(X.ptr, n, h, w, cin, X.ld, zv.ptr, DY.ptr, cout, zv.ld, DY.ld, *bn, ws.data_ptr(), o["dw"].ptr,
                                            wws.data_ptr(), nws, side_stream.cuda_stream if side_stream is not None else None,
                                            wpt.data_ptr() if with_dx else None, o["dx"].ptr if with_dx else None, o["dx"].ld if with_dx else 0,
                                            acc_dx, k, p, code, C.byref(opts), st), "one-call backward")
        else:
            L.check(lib.upa_bn_act_bwd(zv.ptr, DY.ptr, npix, cout, zv.ld, DY.ld, *bn, 1, ws.data_ptr(), code, st), "bn_act_bwd")
            L.check(lib.upa_conv2d_wgrad(X.ptr, n, h, w, cin, X.ld, o["dz"].ptr, cout, o["dz"].ld, o["dw"].ptr, k, 1, p, 1, code, wws.data_ptr(), nws,
                                         st), "wgrad")
            if with_dx:
                L.check(lib.upa_conv2d_bias_act(o["dz"].ptr, n, h, w, cout, o["dz"].ld, wpt.data_ptr(), None, o["dx"].ptr, cin, o["dx"].ld,
                                                o["dx"].ptr if acc_dx else None, o["dx"].ld if acc_dx else 0, k, 1, k - 1 - p, NONE, code,
                                                C.byref(opts), st), "dgrad")
        torch.cuda.synchronize()  # joins the side stream before anything is read
        return o, wws

    for side_stream, acc_dx, with_dx in ((None, 0, True), (side, 1, True), (side, 0, False), (None, 1, True)):
        (a, _wa), (b, _wb) = bwd("one", side_stream, acc_dx, with_dx), bwd("separate", None, acc_dx, with_dx)
        for key in a:
            assert KC.same_bits(a[key].buf, b[key].buf), f"backward side={side_stream is not None} acc={acc_dx} dx={with_dx}: {key} differs"
        for key in ("dz", "dg", "db", "dw"):
            a[key].payload(f"backward {key}")
        if with_dx:
            a["dx"].payload("backward dx")
        else:
            assert a["dx"].untouched(), "w_packed_t = NULL: dx written"
    print(f"one-call forms {dtype} k{k}: identical to their separate calls")


# =====================================================================================================================
# c. the stride-2 data gradient: three routes
# =====================================================================================================================
def _fused_expected(cin, n, oh, ow):
    """conv_big.hip big_prepare + upa_conv_big_launch_interleave restated: the interleaving epilogue exists for 128-channel columns
    (eight n-tiles per workgroup) only.  4 cin <= 96 takes 64- / 96-channel columns, and a multiple of 64 is split into 64-channel
    columns while 128-pixel x 128-channel workgroups would be fewer than the compute units."""
    ntn = -(-4 * cin // 16)
    ntb = 4 if ntn <= 4 else (6 if ntn <= 6 else 8)
    px = n * (oh + 1) * (ow + 1)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if ntb == 8 and ntn % 4 == 0 and (px + 127) // 128 * -(-ntn // 8) < cus:
        ntb = 4
    return ntb == 8


def _dgrad_case(cin, cout, hw, n, acc, dtype, report, seed):
    DEV, L, lib, st = KC.env()
    h, w = hw
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    code = L.dtype_code(dtype)
    what = f"dgrad s2 {'bf16' if dtype == BF16 else 'f32'} {cin}<-{cout} dx {h}x{w} acc{acc}"
    _, dz, wt = TR.conv_grad_family(n, cin, cout, h, w, 3, 2, 1, dtype, seed)
    assert tuple(dz.shape[2:]) == (oh, ow)
    dx0 = TR.stored(torch.linspace(-2.0, 2.0, n * h * w * cin).reshape(-1, cin), dtype) if acc else None
    v, S = TR.dgrad_ref(dz, wt, 2, 1, hw)
    ref = v + (_nchw(dx0.double(), n, h, w) if acc else 0.0)
    DZ = _In(_rows(dz), dtype, 2)
    wdev = _dev(wt)
    # the phase weights: a pure permutation with zeros
    pv = torch.full((16 * cin * cout + 8,), NAN, device=DEV)
    L.check(lib.upa_dgrad_s2_phase_weights(wdev.data_ptr(), cout, cin, pv.data_ptr() + 16, st), what)
    got_v = pv.cpu()
    assert bool(torch.isnan(got_v[:4]).all()) and bool(torch.isnan(got_v[-4:]).all())
    assert torch.equal(got_v[4:-4].reshape(4, cin, cout, 2, 2), TR.phase_weights_ref(wt)), what + ": phase weights"
    phase = _pack_dev(pv[4:-4], 4 * cin, cout, 2, dtype, 0)
    wpt = _pack_dev(wdev, cout, cin, 3, dtype, 1)

    def check(outs, route, K, extra=0.0):
        got = _nchw(_pair(outs, f"{what} {route}")[0], n, h, w)
        bound = CR.conv_bound(v, S, ref, K, NONE, dtype) + extra
        KC.check_bound(got, ref, bound, f"{what} {route}", report)

    # route 1: the interleaving epilogue of conv_big
    if dtype == BF16:
        outs, rcs = [], []
        for _ in range(2):
            o = _Out(n * h * w, cin, dtype, 3, dx0)
            rcs.append(lib.upa_conv2d_dgrad_s2(DZ.ptr, n, oh, ow, cout, DZ.ld, phase.data_ptr(), o.ptr, h, w, cin, o.ld, acc, code,
                                               C.byref(_opts(conv_big=2)), st))
            outs.append([o])
        expect = UPA_OK if _fused_expected(cin, n, oh, ow) else UPA_EUNSUPPORTED
        assert rcs == [expect, expect], f"{what}: fused entry returned {rcs}, the dispatch rule says {expect}"
        if expect == UPA_OK:
            check(outs, "fused", 4 * cout)
        else:
            torch.cuda.synchronize()
            assert all(KC.same_bits(o[0].buf, _Out(n * h * w, cin, dtype, 3, dx0).buf) for o in outs), what + ": a refused call wrote to dx"
    # the refusal: conv_big = 1 (and float32 always)
    o = _Out(n * h * w, cin, dtype, 3)
    rc = lib.upa_conv2d_dgrad_s2(DZ.ptr, n, oh, ow, cout, DZ.ld, phase.data_ptr(), o.ptr, h, w, cin, o.ld, acc, code, C.byref(_opts(conv_big=1)), st)
    torch.cuda.synchronize()
    assert rc == UPA_EUNSUPPORTED and o.untouched(), f"{what}: conv_big = 1 returned {rc}"
    opts = _opts(conv_big=1) if dtype == BF16 else _opts()
    # route 2: the phase convolution + upa_interleave2x
    outs = []
    for _ in range(2):
        t = _Out(n * (oh + 1) * (ow + 1), 4 * cin, dtype, 5)
        o = _Out(n * h * w, cin, dtype, 3, dx0)
        L.check(lib.upa_conv2d_bias_act(DZ.ptr, n, oh, ow, cout, DZ.ld, phase.data_ptr(), None, t.ptr, 4 * cin, t.ld, None, 0, 2, 1, 1, NONE, code,
                                        C.byref(opts), st), what)
        tp = [t.ptr + ph * cin * t.es for ph in range(4)]
        L.check(lib.upa_interleave2x(tp[0], tp[1], tp[2], tp[3], n, oh + 1, ow + 1, cin, t.ld, o.ptr, h, w, o.ld, acc, code, st), what)
        outs.append([o, t])
    # (accumulating: the phase value is stored once before the interleave pass adds and stores again)
    extra = (TR.half_ulp_bf16(v.abs() + CR.conv_bound(v, S, v, 4 * cout, NONE, dtype)) if dtype == BF16 else U24 * v.abs()) if acc else 0.0
    check([[r[0]] for r in outs], "phase + interleave", 4 * cout, extra)
    assert KC.same_bits(outs[0][1].buf, outs[1][1].buf)
    outs[0][1].payload(what + " phase maps")
    # route 3: upa_dilate2x + the flipped 3 x 3 convolution
    outs = []
    for _ in range(2):
        up = _Out(n * h * w, cout, dtype, 5)
        o = _Out(n * h * w, cin, dtype, 3, dx0)
        L.check(lib.upa_dilate2x(DZ.ptr, n, oh, ow, cout, DZ.ld, up.ptr, h, w, up.ld, code, st), what)
        L.check(lib.upa_conv2d_bias_act(up.ptr, n, h, w, cout, up.ld, wpt.data_ptr(), None, o.ptr, cin, o.ld, o.ptr if acc else None,
                                        o.ld if acc else 0, 3, 1, 1, NONE, code, C.byref(opts), st), what)
        outs.append([o, up])
    check([[r[0]] for r in outs], "dilate + flipped conv", 9 * cout)
    upv = _nchw(outs[0][1].payload(what + " dilated"), n, h, w)  # exact: dz at the even pixels, zero elsewhere
    want = torch.zeros(n, cout, h, w, dtype=F64)
    want[:, :, ::2, ::2] = dz.double()
    assert torch.equal(upv, want), what + ": upa_dilate2x"


@pytest.mark.parametrize("cin,cout", TR.DGRAD_CHANNELS)
@KC.stop_after_fault
def test_stride2_data_gradient_routes_bf16(cin, cout):
    """The three routes to the data gradient of a 3 x 3 stride-2 convolution against TR.dgrad_ref, n = 2, dx maps 13 x 11, 16 x 16 and
    7 x 20 (odd sizes: phase pixels past the last row / column), accumulate 0 and 1, dz and dx as slices.
      fused      upa_conv2d_dgrad_s2 under conv_big = 2.  Reading conv_big.hip, the interleaving epilogue is instantiated for
                 128-channel columns only: at these map sizes that is 4 cin = 160 (cin 40, the column boundary inside a phase);
                 4 cin = 64 and 96 take the 64- / 96-channel workgroups and 4 cin = 256 is split into 64-channel columns on maps
                 this small (test_stride2_fused_128_columns reaches it) - there the entry must return UPA_EUNSUPPORTED and leave
                 dx as it was.  _fused_expected restates the rule and the return code is asserted against it;
      phases     conv_big = 1: the fused entry refuses (dx still NaN), then the k = 2 phase convolution + upa_interleave2x;
      dilate     upa_dilate2x (exact) + upa_conv2d_bias_act with the transposed, flipped weights.
    Bound: CR.conv_bound with K = 4 cout (phase routes: at most four taps reach a pixel) or 9 cout, the pre-fill as the residual;
    the interleave route rounds twice when it accumulates (half a bf16 ulp more).  upa_dgrad_s2_phase_weights is compared exactly
    with TR.phase_weights_ref.  Measured on MI355X: 0.958 - 0.976 on every route (the bf16 output rounding), float32 0.033."""
    report = []
    for i, hw in enumerate(TR.DGRAD_MAPS):
        for acc in (0, 1):
            _dgrad_case(cin, cout, hw, 2, acc, BF16, report, 1000 + cin + 10 * i + acc)
    KC.print_report(report, f"dgrad s2 bf16 {cin}<-{cout}", "comparisons")


@KC.stop_after_fault
def test_stride2_data_gradient_routes_f32():
    """float32 has the two fallback routes only: the fused entry refuses, the phase and dilate routes meet the float32 bound."""
    report = []
    for cin, cout in ((12, 20), (24, 64)):
        for i, hw in enumerate(TR.DGRAD_MAPS):
            _dgrad_case(cin, cout, hw, 2, i % 2, F32, report, 1100 + cin + i)
    KC.print_report(report, "dgrad s2 f32", "comparisons")


@KC.stop_after_fault
def test_stride2_fused_128_columns():
    """64 <- 128 with enough pixels that big_prepare keeps 128-channel columns (2 x 92 x 92 phase pixels >= 128 per compute unit pair):
    the fused form on 4 cin = 256, a phase boundary on the column boundary, odd dx map 183 x 182, accumulate 1."""
    report = []
    n, h, w = 2, 183, 182
    if not _fused_expected(64, n, (h - 1) // 2 + 1, (w - 1) // 2 + 1):
        n = 4
    assert _fused_expected(64, n, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    _dgrad_case(64, 128, (h, w), n, 1, BF16, report, 1200)
    KC.print_report(report, "dgrad s2 fused 64<-128", "comparisons")


# =====================================================================================================================
# d. upa_conv2d_wgrad: the float32 instantiations and the bf16 generic fallback
# =====================================================================================================================
@pytest.mark.parametrize("case", TR.WGRAD_CASES, ids=[c[6].split(":")[0].replace(" ", "_").replace(",", "") + f"_{c[1]}-{c[2]}" for c in TR.WGRAD_CASES])
@KC.stop_after_fault
def test_wgrad_generic_branches(case):
    """wgrad_kernel<T, MT, NT, KK> on 2 x 9 x 13 maps, ragged channel counts, x and dz slices, accumulate 0 and 1.  The branch each
    shape takes is read off upa_conv2d_wgrad's dispatch (wgrad_small: cin <= 32 or cout <= 32; the bf16 ring forms need k = 3, or
    k = 1 with stride 1 and cin, cout >= 32) and stated with the case in TR.WGRAD_CASES.
    Bound: K u S + u |ref| with K = n oh ow the terms per element - one float32 rounding per MFMA accumulation step (bf16 products
    are exact, float32 ones are fused), the partial blocks only shorten the chains; u |ref| for the final add and store.
    Measured on MI355X: 0.003 - 0.028 (a worst-case chain bound; random signs stay far inside it)."""
    DEV, L, lib, st = KC.env()
    dtype, cin, cout, k, s, p, branch = case
    n, h, w = TR.WGRAD_MAP
    code = L.dtype_code(dtype)
    x, dz, _ = TR.conv_grad_family(n, cin, cout, h, w, k, s, p, dtype, cin * 7 + cout)
    X, DZ = _In(_rows(x), dtype, 2), _In(_rows(dz), dtype, 4)
    dw, S = TR.wgrad_ref(x, dz, k, s, p)
    K = n * dz.shape[2] * dz.shape[3]
    nws = lib.upa_conv2d_wgrad_workspace_bytes(cin, cout, k)
    wws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    report = []
    for acc in (0, 1):
        dw0 = torch.linspace(-3.0, 3.0, dw.numel())
        outs = []
        for _ in range(2):
            o = [_Vec(dw.numel(), dw0 if acc else None)]
            L.check(lib.upa_conv2d_wgrad(X.ptr, n, h, w, cin, X.ld, DZ.ptr, cout, DZ.ld, o[0].ptr, k, s, p, acc, code, wws.data_ptr(), nws, st), branch)
            outs.append(o)
        ref = dw.reshape(-1) + (dw0.double() if acc else 0.0)
        KC.check_bound(_pair(outs, branch)[0], ref, K * U24 * S.reshape(-1) + U24 * ref.abs() + 1e-300, f"{branch} acc{acc}", report)
    KC.print_report(report, f"wgrad {branch}", "comparisons")


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@KC.stop_after_fault
def test_wgrad_refuses_k5(dtype):
    DEV, L, lib, st = KC.env()
    n, h, w = TR.WGRAD_MAP
    cin, cout = 40, 40
    x, dz, _ = TR.conv_grad_family(n, cin, cout, h, w, 5, 1, 2, dtype, 9)
    X, DZ = _In(_rows(x), dtype, 2), _In(_rows(dz), dtype, 4)
    o = _Vec(cout * cin * 25)
    nws = lib.upa_conv2d_wgrad_workspace_bytes(cin, cout, 5)
    wws = torch.empty(nws, dtype=torch.uint8, device=DEV)
    rc = lib.upa_conv2d_wgrad(X.ptr, n, h, w, cin, X.ld, DZ.ptr, cout, DZ.ld, o.ptr, 5, 1, 2, 0, L.dtype_code(dtype), wws.data_ptr(), nws, st)
    torch.cuda.synchronize()
    assert rc == UPA_EUNSUPPORTED and bool(torch.isnan(o.buf).all())


# =====================================================================================================================
# e. pooling and upsampling backward
# =====================================================================================================================
def _pool_call(X, DY, o, n, h, w, c, k, s, p, acc, code, wsb, nws=None):
    _, _, lib, st = KC.env()
    return lib.upa_maxpool2d_bwd(X.ptr, DY.ptr, n, h, w, c, X.ld, DY.ld, k, s, p, o.ptr, o.ld, acc, code, wsb.data_ptr(),
                                 wsb.numel() if nws is None else nws, st)


@pytest.mark.parametrize("ksp", TR.POOL_KSP, ids=lambda v: f"k{v[0]}s{v[1]}p{v[2]}")
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_maxpool_backward(dtype, ksp):
    """upa_maxpool2d_bwd against TR.maxpool_bwd_ref (torch's first-maximum rule, proved on the CPU): every (k, s, p) on maps from
    1 x 1 (smaller than the window: the unrolled bf16 k = 5 kernels clamp their addresses) to 9 x 11 and 8 x 16, c = E and 5 E,
    accumulate 0 and 1, the ties / flat / neginf families.  dy holds multiples of 1 / 128, so float32 adds without rounding:
    float32 results are exact; a bf16 result is the exact sum rounded once - half a bf16 ulp of the float64 sum plus k^2 2^-24 A.
    A map the window does not fit (k > h + 2 p) is refused.  Measured on MI355X: float32 exact, bf16 1.000 (exact ties of the one rounding)."""
    DEV, L, lib, st = KC.env()
    k, s, p = ksp
    code = L.dtype_code(dtype)
    E = 16 // _es(dtype)
    n = 2
    report = []
    for (h, w) in TR.POOL_MAPS:
        for c in (E, 5 * E):
            for fi, family in enumerate(TR.POOL_FAMILIES):
                what = f"pool {'bf16' if dtype == BF16 else 'f32'} k{k}s{s}p{p} {h}x{w} c{c} {family}"
                if h + 2 * p < k or w + 2 * p < k:
                    X, DY, o = _In(torch.zeros(n * h * w, c), dtype, 2), _In(torch.zeros(n, c), dtype, 4), _Out(n * h * w, c, dtype, 3)
                    wsb = torch.empty(64 * c, dtype=torch.uint8, device=DEV)
                    assert _pool_call(X, DY, o, n, h, w, c, k, s, p, 0, code, wsb) == UPA_EINVAL and o.untouched(), what
                    continue
                x, dy = TR.pool_family(family, n, c, h, w, k, s, p, dtype, h * 31 + w + fi)
                oh, ow = dy.shape[2:]
                ref0, A = TR.maxpool_bwd_ref(x, dy, k, s, p)
                X, DY = _In(_rows(x), dtype, 2), _In(_rows(dy), dtype, 4)
                nws = lib.upa_maxpool2d_bwd_workspace_bytes(n, h, w, c, k, s, p)
                assert nws == n * oh * ow * c
                wsb = torch.empty(nws, dtype=torch.uint8, device=DEV)
                for acc in (0, 1):
                    dx0 = (torch.arange(n * h * w * c).reshape(-1, c) % 33 - 16).float() / 16 if acc else None
                    outs = []
                    for _ in range(2):
                        o = [_Out(n * h * w, c, dtype, 3, dx0)]
                        L.check(_pool_call(X, DY, o[0], n, h, w, c, k, s, p, acc, code, wsb), what)
                        outs.append(o)
                    got = _nchw(_pair(outs, what)[0], n, h, w)
                    ref = ref0 + (_nchw(dx0.double(), n, h, w) if acc else 0.0)
                    if dtype == F32:
                        assert torch.equal(got, ref), f"{what} acc{acc}: not exact"
                        report.append((0.0, what))
                    else:
                        arith = k * k * U24 * (A + (_nchw(dx0.double().abs(), n, h, w) if acc else 0.0))
                        KC.check_bound(got, ref, _out_round(ref, arith, dtype) + 1e-300, f"{what} acc{acc}", report)
    KC.print_report(report, f"maxpool bwd {dtype} {ksp}", "comparisons")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_upsample_backward(dtype):
    """upa_upsample2x_bwd on 1 x 1 and 5 x 7 maps, slices, accumulate 0 and 1; dy multiples of 1 / 128: float32 exact, bf16 rounded once."""
    DEV, L, lib, st = KC.env()
    code = L.dtype_code(dtype)
    E = 16 // _es(dtype)
    report = []
    for (h, w) in ((1, 1), (5, 7)):
        for c in (E, 3 * E):
            n = 2
            dy = ((torch.rand(n, c, 2 * h, 2 * w, generator=torch.Generator().manual_seed(h + c)) * 2 - 1) * 128).round() / 128
            ref0, A = TR.upsample2x_bwd_ref(dy)
            DY = _In(_rows(dy), dtype, 2)
            for acc in (0, 1):
                what = f"upsample bwd {h}x{w} c{c} acc{acc}"
                dx0 = (torch.arange(n * h * w * c).reshape(-1, c) % 33 - 16).float() / 16 if acc else None
                outs = []
                for _ in range(2):
                    o = [_Out(n * h * w, c, dtype, 3, dx0)]
                    L.check(lib.upa_upsample2x_bwd(DY.ptr, n, h, w, c, DY.ld, o[0].ptr, o[0].ld, acc, code, st), what)
                    outs.append(o)
                got = _nchw(_pair(outs, what)[0], n, h, w)
                ref = ref0 + (_nchw(dx0.double(), n, h, w) if acc else 0.0)
                if dtype == F32:
                    assert torch.equal(got, ref), what
                    report.append((0.0, what))
                else:
                    KC.check_bound(got, ref, _out_round(ref, 5 * U24 * (A + ref.abs()), dtype) + 1e-300, what, report)
    KC.print_report(report, f"upsample bwd {dtype}", "comparisons")


# =====================================================================================================================
# f. optimizer and the element-wise movers
# =====================================================================================================================
@pytest.mark.parametrize("n", [1, 255, 1025, 1048577])
@KC.stop_after_fault
def test_sumsq(n):
    """upa_sumsq against the exactly rounded sum (math.fsum of the exact float64 squares), accumulate 0 and 1, three runs bit-identical.
    Bound: the squares are exact in float64; a thread adds ceil(n / (256 grid)) of them in turn, eight tree levels fold a block, the
    fold kernel adds ceil(grid / 256) partials per thread and folds eight more levels, one more add accumulates: every partial sum is
    at most the total, so D 2^-53 sum g^2 with D the number of additions on the longest path - 1 + 8 for n = 255, 23 for n = 1 048 577
    (inside the 4 2^-53 sum g^2 log2(blocks) = 40 2^-53 sum g^2 the 1024-block case was specified with; one block has log2 = 0 but
    still folds eight levels).  n = 1 is exact.  Measured on MI355X: every case came out exactly rounded (error 0)."""
    DEV, L, lib, st = KC.env()
    g = (torch.rand(n, generator=torch.Generator().manual_seed(n)) * 2 - 1) * 3
    gd = _dev(g)
    ws = torch.zeros(lib.upa_sumsq_workspace_bytes() // 8, dtype=F64, device=DEV)
    ref = TR.sumsq_ref(g)
    grid = max(1, min(1024, -(-n // 1024)))
    D = (-(-n // (256 * grid)) - 1) + 8 + (-(-grid // 256) - 1) + 8 + 1
    if n == 1:
        D = 0
    for acc in (0, 1):
        runs = []
        for _ in range(3):
            out = torch.full((3,), NAN, dtype=F64)
            out[1] = 0.5 if acc else NAN
            out = out.to(DEV)
            L.check(lib.upa_sumsq(gd.data_ptr(), n, out.data_ptr() + 8, acc, ws.data_ptr(), st), "sumsq")
            runs.append(out.cpu())
        assert all(KC.same_bits(runs[0], r) for r in runs[1:]), "sumsq: runs differ"
        assert math.isnan(runs[0][0]) and math.isnan(runs[0][2])
        want = ref + (0.5 if acc else 0.0)
        err = abs(float(runs[0][1]) - want)
        bound = D * 2.0 ** -53 * want + (2.0 ** -53 * want if n > 1 else 0.0)  # (+ the reference's own final rounding)
        print(f"sumsq n {n} acc {acc}: error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def _sgd_bounds(M, prev, lr, mom, wd, d, first, skipped):
    """Per-element bounds after one step from the magnitude terms M = (Mg, Mb, Mp, Me) and the bounds `prev` = (eb, ep, ee) on the state
    the step started from: 6 u Mg for the clipped, decayed gradient (the coefficient: sqrt, cast, add, divide = 4, the product, the
    add), 2 u Mb, 3 u Mp, 4 u Me for the momentum, parameter and EMA lines, and the state's error carried through the same lines."""
    Mg, Mb, Mp, Me = M
    eb, ep, ee = prev
    if not skipped:
        eg = wd * ep + 6 * U24 * Mg
        eb = (0.0 if first else mom * eb) + eg + 2 * U24 * Mb
        ep = ep + lr * (eg + mom * eb) + 3 * U24 * Mp
    ee = d * ee + (1 - d) * ep + 4 * U24 * Me
    return eb, ep, ee


@pytest.mark.parametrize("n", [1, 1000, 300001])
@KC.stop_after_fault
def test_sgd_nesterov_ema(n):
    """upa_sgd_nesterov_ema and upa_sgd_nesterov_ema_scaled against TR.sgd_ref over three steps (the reference keeps its own float32
    state; the bound of a step carries the bound of the state it started from, _sgd_bounds): a clipping step (1) and two that do not
    clip, weight_decay 5e-4 and 0, ema = NULL, the decay read from ema_d_dev while the scalar ema_d holds a wrong value, zero_grad 0
    and 1.  Scaled: grad_sumsq finite lands on the unscaled step's bound; inf and NaN leave p and the momentum buffer bit-identical,
    still move the EMA and still zero the gradient.  Measured on MI355X: 0.20 / 0.37 / 0.44 for n = 1 / 1000 / 300 001."""
    DEV, L, lib, st = KC.env()
    gen = torch.Generator().manual_seed(n)
    p0 = torch.rand(n, generator=gen) * 2 - 1
    lr, mom, max_norm = 0.01, 0.9, 10.0
    report = []
    for wd, with_ema, use_dev, zero, scale in ((5e-4, True, False, 1, None), (0.0, False, False, 0, None), (5e-4, True, True, 0, None),
                                               (5e-4, True, True, 1, 1024.0)):
        P, B, Em = p0.clone(), torch.zeros(n), p0.clone()  # the reference's float32 state
        Pd, Bd, Ed = _dev(P), _dev(B), _dev(Em)
        prev = (torch.zeros(n, dtype=F64),) * 3
        sstate = _dev(torch.tensor([scale or 1.0, 0.0, 0.0, 0.0]))
        for step in range(3):
            what = f"sgd n{n} wd{wd} ema{int(with_ema)} dev{int(use_dev)} zero{zero} scale{scale} step{step}"
            g = (torch.rand(n, generator=gen) * 2 - 1) * (50.0 if step == 1 else 0.01) * (scale or 1.0)
            ss = TR.sumsq_ref(g)
            if step == 1:
                assert math.sqrt(ss) / (scale or 1.0) > max_norm or n == 1
            d = 0.9999 * (1 - math.exp(-(step + 1) / 2000.0)) if step < 2 else 0.75
            Gd, ssd, dd = _dev(g), _dev(torch.tensor([ss]), F64), _dev(torch.tensor([d]))
            args = (Pd.data_ptr(), Gd.data_ptr(), Bd.data_ptr(), Ed.data_ptr() if with_ema else None, n, ssd.data_ptr(), max_norm, lr, mom, wd,
                    int(step == 0), 0.123 if use_dev else d, dd.data_ptr() if use_dev else None, zero)
            if scale is None:
                L.check(lib.upa_sgd_nesterov_ema(*args, st), what)
            else:
                L.check(lib.upa_sgd_nesterov_ema_scaled(*args, sstate.data_ptr(), st), what)
            (pn, gn, bn, en), M = TR.sgd_ref(P, g, B, Em if with_ema else None, ss, max_norm, lr, mom, wd, step == 0, d, zero, scale)
            prev = _sgd_bounds(M, prev, lr, mom, wd, TR.f32(d), step == 0, False)
            KC.check_bound(Bd.cpu().double(), bn, prev[0] + U24 * bn.abs() + 1e-300, what + " momentum", report)
            KC.check_bound(Pd.cpu().double(), pn, prev[1] + U24 * pn.abs() + 1e-300, what + " p", report)
            if with_ema:
                KC.check_bound(Ed.cpu().double(), en, prev[2] + U24 * en.abs() + 1e-300, what + " ema", report)
                Em = en.float()
            else:
                assert torch.equal(Ed.cpu(), p0), what + ": ema = NULL, but the buffer moved"
            assert torch.equal(Gd.cpu(), gn.float()), what + ": gradient after the step"
            P, B = pn.float(), bn.float()
            prev = (prev[0] + U24 * bn.abs(), prev[1] + U24 * pn.abs(), prev[2] + (U24 * en.abs() if with_ema else 0.0))  # the reference's own rounding
        if scale is not None:  # overflowing steps from the state the kernel is in
            for bad in (math.inf, math.nan):
                Gd, ssd = _dev(torch.ones(n)), _dev(torch.tensor([bad]), F64)
                pb, bb, eb = Pd.clone(), Bd.clone(), Ed.clone()
                L.check(lib.upa_sgd_nesterov_ema_scaled(Pd.data_ptr(), Gd.data_ptr(), Bd.data_ptr(), Ed.data_ptr(), n, ssd.data_ptr(), max_norm,
                                                        lr, mom, wd, 0, 0.5, None, 1, sstate.data_ptr(), st), "overflow")
                assert KC.same_bits(Pd, pb) and KC.same_bits(Bd, bb), f"grad_sumsq {bad}: p or the momentum buffer moved"
                assert float(Gd.abs().max()) == 0.0
                want = eb.cpu().double() * 0.5 + 0.5 * pb.cpu().double()
                KC.check_bound(Ed.cpu().double(), want, 4 * U24 * (eb.cpu().double().abs() + pb.cpu().double().abs()) + 1e-300, f"ema of a skipped step {bad}", report)
    KC.print_report(report, f"sgd n{n}", "comparisons")


@KC.stop_after_fault
def test_grad_scaler_update_sequence():
    """upa_grad_scaler_update over a scripted sequence, all four state floats against TR.scaler_ref after every step: clean steps up to
    growth_interval (4), an overflow at tracker = interval - 1, two overflows in a row (inf, then NaN), growth again."""
    DEV, L, lib, st = KC.env()
    state = [65536.0, 0.0, 0.0, 0.0]
    sd = _dev(torch.tensor(state))
    seq = [1.0] * 4 + [2.0] * 3 + [math.inf] + [3.0] + [math.inf, math.nan] + [1.0] * 4
    for i, ss in enumerate(seq):
        ssd = _dev(torch.tensor([ss]), F64)
        L.check(lib.upa_grad_scaler_update(sd.data_ptr(), ssd.data_ptr(), 2.0, 0.5, 4, st), "scaler")
        state = TR.scaler_ref(state, ss, 2.0, 0.5, 4)
        assert sd.cpu().tolist() == state, f"step {i} (sumsq {ss}): {sd.cpu().tolist()} != {state}"
    assert state[0] == 65536.0 * 2 / 8 * 2
    print(f"grad scaler: {len(seq)} steps exact")


@pytest.mark.parametrize("n", [1, 1000, 300001])
@KC.stop_after_fault
def test_ema_update(n):
    """upa_ema_update: e d + (1 - d) v, d from the argument and from device memory (the scalar then holding a wrong value); three
    float32 roundings and (1 - d): 4 u (|e d| + |(1 - d) v|)."""
    DEV, L, lib, st = KC.env()
    gen = torch.Generator().manual_seed(n)
    e, v = torch.rand(n, generator=gen) * 2 - 1, torch.rand(n, generator=gen) * 2 - 1
    report = []
    for use_dev in (False, True):
        d = 0.3
        ed, vd, dd = _dev(e), _dev(v), _dev(torch.tensor([d]))
        L.check(lib.upa_ema_update(ed.data_ptr(), vd.data_ptr(), n, 0.9 if use_dev else d, dd.data_ptr() if use_dev else None, st), "ema")
        d32 = TR.f32(d)
        ref = e.double() * d32 + (1 - d32) * v.double()
        KC.check_bound(ed.cpu().double(), ref, 4 * U24 * ((e.double() * d32).abs() + ((1 - d32) * v.double()).abs()) + 1e-300, f"ema dev{int(use_dev)}", report)
        assert torch.equal(vd.cpu(), v)
    KC.print_report(report, f"ema n{n}", "comparisons")


@KC.stop_after_fault
def test_cast_add_copy_views_and_layout_movers():
    """upa_cast_view (all four type pairs on slices; float32 -> bf16 must round to nearest even: compared with tensor.to(bfloat16) on
    values that include exact ties both ways), upa_add_view and upa_copy_view (exact on slices: the sums are chosen representable),
    upa_nchw_to_nhwc / upa_nhwc_to_nchw (a permutation, plus the same rounding into bf16)."""
    DEV, L, lib, st = KC.env()
    rows, c = 37, 24
    gen = torch.Generator().manual_seed(3)
    src32 = torch.rand(rows, c, generator=gen) * 4 - 2
    # exact ties: 1 + 2^-8 (down to even), 1 + 3 * 2^-8 (up to even), their negatives, and just off the tie
    ties = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23, 1 + 2.0 ** -8 - 2.0 ** -23,
                         3.0e38, 2.0 ** -120])
    src32[0, :8] = ties
    for sdt, ddt in ((F32, BF16), (BF16, F32), (F32, F32), (BF16, BF16)):
        src = TR.stored(src32, sdt)
        S = _In(src, sdt, 2 if sdt == BF16 else 4)
        outs = []
        for _ in range(2):
            o = [_Out(rows, c, ddt, 3 if ddt == BF16 else 6)]
            L.check(lib.upa_cast_view(S.ptr, L.dtype_code(sdt), S.ld, o[0].ptr, L.dtype_code(ddt), o[0].ld, rows, c, st), "cast")
            outs.append(o)
        for a, b in zip(*outs):
            assert KC.same_bits(a.buf, b.buf)
        got = outs[0][0].buf.cpu()[:rows, outs[0][0].E:outs[0][0].E + c]
        assert KC.same_bits(got, src.to(ddt)), f"cast {sdt} -> {ddt}"
        a = outs[0][0].buf.cpu().float()
        assert bool(torch.isnan(a[rows:]).all()) and bool(torch.isnan(a[:, :outs[0][0].E]).all()) and bool(torch.isnan(a[:, outs[0][0].E + c:]).all())
    for dtype in (F32, BF16):
        code = L.dtype_code(dtype)
        n, h, w = 2, 3, 5
        a = (torch.randint(-64, 65, (n * h * w, c), generator=gen) / 8).float()
        b = (torch.randint(-64, 65, (n * h * w, c), generator=gen) / 8).float()
        A, B = _In(a, dtype, 2), _In(b, dtype, 4)
        o, o2 = _Out(n * h * w, c, dtype, 3), _Out(n * h * w, c, dtype, 5)
        L.check(lib.upa_add_view(A.ptr, A.ld, B.ptr, B.ld, o.ptr, o.ld, n, h, w, c, code, st), "add")
        L.check(lib.upa_copy_view(A.ptr, n, h, w, c, A.ld, o2.ptr, o2.ld, code, st), "copy")
        assert torch.equal(o.payload("add_view"), (a + b).double()) and torch.equal(o2.payload("copy_view"), a.double())
        # layout movers: NCHW float32 -> NHWC view of dtype -> NCHW float32
        for cc in (3, 24):
            x = torch.rand(n, cc, h, w, generator=gen) * 2 - 1
            xd = _dev(x)
            E = 16 // _es(dtype)
            cpad = -(-cc // E) * E
            y = _Out(n * h * w, cpad, dtype, 3)
            L.check(lib.upa_nchw_to_nhwc(xd.data_ptr(), n, cc, h, w, y.ptr, y.ld, code, st), "nchw_to_nhwc")
            got = y.buf.cpu()[:n * h * w, y.E:y.E + cc]
            assert KC.same_bits(got, _rows(x).to(dtype)), f"nchw_to_nhwc {dtype} c{cc}"
            back = torch.full((n * cc * h * w + 8,), NAN, device=DEV)
            L.check(lib.upa_nhwc_to_nchw(y.ptr, n, h, w, cc, y.ld, back.data_ptr() + 16, code, st), "nhwc_to_nchw")
            bk = back.cpu()
            assert bool(torch.isnan(bk[:4]).all()) and bool(torch.isnan(bk[-4:]).all())
            assert torch.equal(bk[4:-4].reshape(n, cc, h, w), x.to(dtype).float()), f"nhwc_to_nchw {dtype} c{cc}"
    print("cast / add / copy / layout movers: exact")


# =====================================================================================================================
# g. refusals
# =====================================================================================================================
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@KC.stop_after_fault
def test_refusals_leave_every_output_untouched(dtype):
    """Every pitch argument of every entry that is not a multiple of 16 bytes, c not a multiple of E, c > 256 E, npix = 0, and
    upa_maxpool2d_bwd with k > h + 2 pad, pad > k / 2, k = 16 or a workspace one byte short, upa_cast_view with c = 0: UPA_EINVAL, and
    every output buffer is bit-identical to its pre-fill afterwards - nothing was launched."""
    DEV, L, lib, st = KC.env()
    code = L.dtype_code(dtype)
    E = 16 // _es(dtype)
    n, h, w, c = 2, 4, 6, 2 * E
    npix = n * h * w
    big = 4 * npix  # rows: room for every variation
    src = TR.stored(torch.rand(big, 4 * c, generator=torch.Generator().manual_seed(1)), dtype)
    A, B = _In(src, dtype, 2), _In(src, dtype, 4)
    o1, o2, oc = _Out(big, 4 * c, dtype, 3), _Out(big, 4 * c, dtype, 5), _Out(big, 4 * c, dtype, 4)
    v1, v2, v3, v4 = (_Vec(4 * c, torch.linspace(-1, 1, 4 * c)) for _ in range(4))
    f = _dev(torch.ones(300 * E))
    ws = _reduce_ws(300 * E)
    wsb = torch.full((big * 4 * c,), 0x5A, dtype=torch.uint8, device=DEV)
    outs = [o1, o2, oc, v1, v2, v3, v4]
    before = [t.buf.clone() for t in outs] + [ws.clone(), wsb.clone()]
    fp = f.data_ptr()

    def stats(**kw):
        a = dict(npix=npix, c=c, ld=A.ld); a.update(kw)
        return lib.upa_bn_stats(A.ptr, a["npix"], a["c"], a["ld"], ws.data_ptr(), code, st)

    def csum(**kw):
        a = dict(npix=npix, c=c, ld=A.ld); a.update(kw)
        return lib.upa_channel_sum(A.ptr, a["npix"], a["c"], a["ld"], v1.ptr, 0, ws.data_ptr(), code, st)

    def fwd(**kw):
        a = dict(npix=npix, c=c, ldz=A.ld, ldy=o1.ld, ldr=B.ld); a.update(kw)
        return lib.upa_bn_act_fwd(A.ptr, a["npix"], a["c"], a["ldz"], fp, fp, fp, fp, EPS, SILU, o1.ptr, a["ldy"], B.ptr, a["ldr"], code, st)

    def bwd(**kw):
        a = dict(npix=npix, c=c, ldz=A.ld, lddy=B.ld, lddz=o1.ld); a.update(kw)
        return lib.upa_bn_act_bwd(A.ptr, B.ptr, a["npix"], a["c"], a["ldz"], a["lddy"], fp, fp, fp, fp, EPS, SILU, o1.ptr, a["lddz"], v1.ptr, v2.ptr,
                                  0, ws.data_ptr(), code, st)

    def dil(**kw):
        a = dict(c=c, lds=A.ld, ldd=o1.ld, n=n); a.update(kw)
        return lib.upa_dilate2x(A.ptr, a["n"], h // 2, w // 2, a["c"], a["lds"], o1.ptr, h, w, a["ldd"], code, st)

    def ups(**kw):
        a = dict(c=c, lddy=A.ld, lddx=o1.ld, n=n); a.update(kw)
        return lib.upa_upsample2x_bwd(A.ptr, a["n"], h // 2, w // 2, a["c"], a["lddy"], o1.ptr, a["lddx"], 0, code, st)

    def itl(**kw):
        a = dict(c=c, ldt=A.ld, lddx=o1.ld, n=n); a.update(kw)
        return lib.upa_interleave2x(A.ptr, A.ptr, A.ptr, A.ptr, a["n"], h // 2 + 1, w // 2 + 1, a["c"], a["ldt"], o1.ptr, h, w, a["lddx"], 0, code, st)

    def pool(**kw):
        a = dict(c=c, ldx=A.ld, lddy=B.ld, lddx=o1.ld, k=3, s=1, p=1, n=n, nws=wsb.numel()); a.update(kw)
        return lib.upa_maxpool2d_bwd(A.ptr, B.ptr, a["n"], h, w, a["c"], a["ldx"], a["lddy"], a["k"], a["s"], a["p"], o1.ptr, a["lddx"], 0, code,
                                     wsb.data_ptr(), a["nws"], st)

    def cast(**kw):
        a = dict(c=2 * 8, lds=A.ld, ldd=oc.ld, npix=npix); a.update(kw)
        return lib.upa_cast_view(A.ptr, code, a["lds"], oc.ptr, code, a["ldd"], a["npix"], a["c"], st)

    bad = {
        "bn_stats ld": stats(ld=A.ld - 1), "bn_stats c % E": stats(c=c - 1), "bn_stats c > 256 E": stats(c=257 * E, ld=300 * E), "bn_stats npix 0": stats(npix=0),
        "channel_sum ld": csum(ld=A.ld + 1), "channel_sum c % E": csum(c=c + 1), "channel_sum c > 256 E": csum(c=257 * E, ld=300 * E), "channel_sum npix 0": csum(npix=0),
        "bn_act_fwd ldz": fwd(ldz=A.ld - 1), "bn_act_fwd ldy": fwd(ldy=o1.ld - 1), "bn_act_fwd ldr": fwd(ldr=B.ld - 1), "bn_act_fwd c % E": fwd(c=c - 1),
        "bn_act_fwd c > 256 E": fwd(c=257 * E), "bn_act_fwd npix 0": fwd(npix=0),
        "bn_act_bwd ldz": bwd(ldz=A.ld + 1), "bn_act_bwd lddy": bwd(lddy=B.ld - 1), "bn_act_bwd lddz": bwd(lddz=o1.ld + 1), "bn_act_bwd c % E": bwd(c=c + 1),
        "bn_act_bwd c > 256 E": bwd(c=257 * E), "bn_act_bwd npix 0": bwd(npix=0),
        "dilate2x lds": dil(lds=A.ld - 1), "dilate2x ldd": dil(ldd=o1.ld - 1), "dilate2x c % E": dil(c=c - 1), "dilate2x npix 0": dil(n=0),
        "upsample2x_bwd lddy": ups(lddy=A.ld - 1), "upsample2x_bwd lddx": ups(lddx=o1.ld - 1), "upsample2x_bwd c % E": ups(c=c - 1), "upsample2x_bwd npix 0": ups(n=0),
        "interleave2x ldt": itl(ldt=A.ld - 1), "interleave2x lddx": itl(lddx=o1.ld - 1), "interleave2x c % E": itl(c=c - 1), "interleave2x npix 0": itl(n=0),
        "maxpool2d_bwd ldx": pool(ldx=A.ld - 1), "maxpool2d_bwd lddy": pool(lddy=B.ld - 1), "maxpool2d_bwd lddx": pool(lddx=o1.ld - 1),
        "maxpool2d_bwd c % E": pool(c=c - 1), "maxpool2d_bwd npix 0": pool(n=0), "maxpool2d_bwd k > h + 2 pad": pool(k=7, p=1),
        "maxpool2d_bwd pad > k / 2": pool(k=3, p=2), "maxpool2d_bwd k 16": pool(k=16, p=8),
        "maxpool2d_bwd workspace one byte short": pool(nws=lib.upa_maxpool2d_bwd_workspace_bytes(n, h, w, c, 3, 1, 1) - 1),
        "cast_view c 0": cast(c=0), "cast_view c % 8": cast(c=12), "cast_view lds": cast(lds=A.ld - 4), "cast_view ldd": cast(ldd=oc.ld + 4), "cast_view npix 0": cast(npix=0),
    }
    wrong = {k: v for k, v in bad.items() if v != UPA_EINVAL}
    assert not wrong, f"not refused with UPA_EINVAL: {wrong}"
    torch.cuda.synchronize()
    for t, b in zip([t.buf for t in outs] + [ws, wsb], before):
        assert KC.same_bits(t, b), "a refused call wrote to one of its buffers"
    # ... and the unvaried calls are valid ones
    for name, rc in (("bn_stats", stats()), ("channel_sum", csum()), ("bn_act_fwd", fwd()), ("bn_act_bwd", bwd()), ("dilate2x", dil()),
                     ("upsample2x_bwd", ups()), ("interleave2x", itl()), ("maxpool2d_bwd", pool()), ("cast_view", cast())):
        assert rc == UPA_OK, name
    torch.cuda.synchronize()
    print(f"refusals {dtype}: {len(bad)} calls refused, outputs untouched")
