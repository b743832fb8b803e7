"""-m gpu: `upa_dwconv2d`, `upa_psa_attention` and `upa_conv_transpose2x2` called through the C ABI on raw buffers and compared, element
by element, with the float64 references and derived bounds of tests/yolo11_kernel_ref.py (pinned on the CPU by
tests/test_yolo11_kernel_ref.py).

Buffers, sentinels, the two bit-identical runs, the per-element bounds and the fault latch: the conventions of tests/kernel_check.py,
with the
output canary held to its very NaN bits.  Batch is 2 unless stated.

Which instantiation a parametrisation reaches (from the dispatch conditions; neither entry point has a variant query):
  upa_dwconv2d       vec = c, ldx, ldy multiples of V (f32 4, bf16 8) and x, y, weight, bias 16-byte aligned -> dwconv3_kernel<T, V, S>,
                     else <T, 1, S>.  Views start E = 16 bytes of channels into buffers c + 2 E / c + 3 E wide, so alignment follows c:
                       f32  c 4, 8, 12, 40 -> <float, 4, S>;  c 6 -> <float, 1, S>
                       bf16 c 8, 40 -> <bf16, 8, S>;  c 4, 6, 12 -> <bf16, 1, S>
                     c 8 at channel offset 1 (odd pitches) -> V = 1 in both types.  S = stride.
  upa_psa_attention  bf16 and ldqkv % 8 == 0 and qkv 16-byte aligned -> psa_attn_mfma_kernel; else psa_attn_kernel<T, 32, 64>:
                       route "f32"          ldqkv = 128 heads + 8, view at channel 4  -> psa_attn_kernel<float, 32, 64>
                       route "mfma"         bf16, ldqkv = 128 heads + 8, view at channel 8 (16 bytes) -> psa_attn_mfma_kernel
                       route "scalar_ld"    bf16, ldqkv = 128 heads + 3 -> psa_attn_kernel<bf16, 32, 64>
                       route "scalar_base"  bf16, ldqkv = 128 heads + 8, view at channel 1 (2 bytes) -> psa_attn_kernel<bf16, 32, 64>
                     ldy = 64 heads + 8 with the view at channel 4 on every route.
  upa_conv_transpose2x2  convt2x2_kernel<bf16> / <f32> by dtype alone.

Worst error / bound over all cases, CPU emulation of the kernel's arithmetic (tests/test_yolo11_kernel_ref.py) | measured on MI355X:
  dwconv3_kernel<float, 4 | 1>                  0.250 | 0.250      dwconv3_kernel<bf16, 8 | 1>             0.989 | 0.996 (1 x 1048876 map)
  convt2x2_kernel<f32>                          0.327 | 0.327      convt2x2_kernel<bf16>                   0.995 | 0.995
  psa_attn_kernel<float> (route f32)            0.171 | 0.171      psa_attn_kernel<bf16> (both scalar routes) 0.995 | 0.995
  psa_attn_mfma_kernel (route mfma)             0.988 | 0.988
The bf16 figures are the output rounding itself (half an ulp at the foot of a binade); the f32 ones agree with the emulation to the
digits shown, so the bounds are as tight as the derivation allows and every mutant of the CPU file leaves them."""

import pytest
import torch

from tests import yolo11_kernel_ref as Y
from tests.conv_ref import ACT_NONE, ACT_SILU
from tests import kernel_check as KC

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SPARE = 4
UPA_EINVAL, UPA_EUNSUPPORTED = -1, -2
NAN = float("nan")


def _es(dtype):
    return 2 if dtype == BF16 else 4


class _View:
    """`rows` x `c` values at channel `off` of a (rows + spare) x ld buffer of NaN."""

    def __init__(self, rows, c, ld, off, dtype, values=None):
        self.rows, self.c, self.ld, self.off, self.dtype = rows, c, ld, off, dtype
        self.buf = (KC.out_buf((rows,), ld, dtype, SPARE, dev="cpu").to(KC.env()[0]) if values is None else
                    KC.slice_buf(values, dtype, off, tail=ld - off - c))
        self.ptr = self.buf.data_ptr() + off * _es(dtype)

    def untouched(self):
        return bool((KC.bits(self.buf) == KC.bits(torch.full((1,), NAN, dtype=self.dtype))[0]).all())

    def payload(self, what):
        """Canary intact in every bit outside the slice, payload finite -> (rows, c) float64."""
        return KC.payload(self.buf, self.rows, self.c, what, offset=self.off, exact_fill=True).double()


def _rows(t_nchw):
    """NCHW -> (n h w, c)."""
    return t_nchw.permute(0, 2, 3, 1).reshape(-1, t_nchw.shape[1])


# =====================================================================================================================
# upa_dwconv2d
# =====================================================================================================================
def _dw_call(x, w9c, bias, stride, act, dtype, off=None, k=3, pad=1):
    DEV, L, lib, st = KC.env()
    n, c, h, w = x.shape
    E = 16 // _es(dtype)
    off = E if off is None else off
    oh, ow = Y.dw_out_hw(h, w, stride)
    xin = _View(n * h * w, c, c + 2 * E + (off - E if off != E else 0), off, dtype, _rows(x))
    yout = _View(n * oh * ow, c, c + 3 * E + (off - E if off != E else 0), off, dtype)
    wd, bd = w9c.to(DEV), bias.to(DEV)
    rc = lib.upa_dwconv2d(xin.ptr, n, h, w, c, xin.ld, wd.data_ptr(), bd.data_ptr(), yout.ptr, yout.ld, k, stride, pad, act, L.dtype_code(dtype), st)
    torch.cuda.synchronize()
    return rc, yout, (n, oh, ow, c)


def _dw_check(family, n, c, h, w, stride, act, dtype, seed, report, off=None):
    x, w9c, bias = Y.dw_family(family, n, c, h, w, dtype, seed)
    what = f"dwconv {'bf16' if dtype == BF16 else 'f32'} {family} n{n} c{c} {h}x{w} s{stride} act{act} off{off}"
    rc, yout, (n_, oh, ow, _) = _dw_call(x, w9c, bias, stride, act, dtype, off)
    assert rc == 0, what
    y = yout.payload(what)
    v, S, ref = Y.dw_ref(x, w9c, bias, stride, act)
    if family == "saturated" and v.numel() >= 400:
        assert float(v.max()) > 60 and float(v.min()) < -60, what
    KC.check_bound(y, _rows(ref), _rows(Y.dw_bound(v, S, ref, act, dtype)), what, report)


@pytest.mark.parametrize("act", [ACT_NONE, ACT_SILU], ids=["none", "silu"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_dwconv_every_instantiation(dtype, stride, act):
    """Three families x seven maps (1 x 1 to 5 x 4: every border combination, odd and even sizes for stride 2) x c 4 / 6 / 8 / 12 / 40,
    which reach V = 4 / 8 and V = 1 in both types (module docstring), and c = 8 views at channel offset 1, which must take V = 1."""
    report = []
    for fi, family in enumerate(Y.DW_FAMILIES):
        for (h, w) in Y.DW_MAPS:
            for c in Y.DW_CHANNELS:
                _dw_check(family, 2, c, h, w, stride, act, dtype, 10 * c + fi, report)
            _dw_check(family, 2, 8, h, w, stride, act, dtype, 90 + fi, report, off=1)
    KC.print_report(report, f"dwconv {dtype} s{stride} act{act}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_dwconv_row_loop_second_trip_crosses_the_image_boundary(dtype):
    """n = 2, h = 33000, w = 1, c = 8: 66000 output rows on a grid of 65535, so blocks 0 .. 464 take a second trip, which lands in image
    1 while their first was in image 0 (b = row / oh is recomputed per trip)."""
    report = []
    for family in ("uniform", "impulse"):
        _dw_check(family, 2, 8, 33000, 1, 1, ACT_SILU, dtype, 120, report)
    KC.print_report(report, f"dwconv rows {dtype}")


@pytest.mark.parametrize("stride,vectors", [(1, 1), (2, 1), (2, 2)], ids=["s1_1vec", "s2_1vec", "s2_2vec"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_dwconv_item_loop_second_trip(dtype, stride, vectors):
    """n = 1, h = 1, w = 4096 * 256 + 300: with one vector of channels and stride 1 a row has 1048876 items on a grid of 4096 x 256, so
    300 threads take a second trip.  At stride 2 one vector of channels halves the items (524438: one trip, the case as the issue
    lists it); two vectors bring them back to 1048876 and the second trip with them."""
    V = 16 // _es(dtype)
    w = 4096 * 256 + 300
    items = Y.dw_out_hw(1, w, stride)[1] * vectors
    assert (items > 4096 * 256) == (stride == 1 or vectors == 2)
    report = []
    _dw_check("uniform", 1, V * vectors, 1, w, stride, ACT_NONE, dtype, 130 + stride, report)
    KC.print_report(report, f"dwconv items {dtype} s{stride} x{vectors}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_dwconv_refusals_leave_the_output_untouched(dtype):
    DEV, L, lib, st = KC.env()
    x, w9c, bias = Y.dw_family("uniform", 2, 8, 4, 4, dtype, 140)
    rc, yout, _ = _dw_call(x, w9c, bias, 1, ACT_SILU, dtype, k=5, pad=2)
    assert rc == UPA_EUNSUPPORTED and yout.untouched()
    rc, yout, _ = _dw_call(x, w9c, bias, 3, ACT_SILU, dtype)
    assert rc == UPA_EUNSUPPORTED and yout.untouched()
    # ldx < c, and an output view that starts inside the input view
    E, es = 16 // _es(dtype), _es(dtype)
    xin = _View(32, 8, 8 + 2 * E, E, dtype, _rows(x))
    yout = _View(32, 8, 8 + 3 * E, E, dtype)
    wd, bd = w9c.to(DEV), bias.to(DEV)
    code = L.dtype_code(dtype)
    assert lib.upa_dwconv2d(xin.ptr, 2, 4, 4, 8, 7, wd.data_ptr(), bd.data_ptr(), yout.ptr, yout.ld, 3, 1, 1, ACT_SILU, code, st) == UPA_EINVAL
    before = KC.bits(xin.buf.cpu()).clone()
    assert lib.upa_dwconv2d(xin.ptr, 2, 4, 4, 8, xin.ld, wd.data_ptr(), bd.data_ptr(), xin.ptr + 3 * xin.ld * es, xin.ld, 3, 1, 1, ACT_SILU, code,
                            st) == UPA_EINVAL
    torch.cuda.synchronize()
    assert yout.untouched() and torch.equal(KC.bits(xin.buf.cpu()), before)
    assert lib.upa_dwconv2d(xin.ptr, 2, 4, 4, 8, xin.ld, wd.data_ptr(), bd.data_ptr(), yout.ptr, yout.ld, 3, 1, 1, ACT_SILU, code, st) == 0
    torch.cuda.synchronize()
    yout.payload("the unvaried call")


# =====================================================================================================================
# upa_psa_attention
# =====================================================================================================================
PSA_ROUTES = {  # dtype, bound, ldqkv - 128 heads, channel offset of the view
    "f32": (F32, "scalar", 8, 4),
    "mfma": (BF16, "mfma", 8, 8),
    "scalar_ld": (BF16, "scalar", 3, 0),
    "scalar_base": (BF16, "scalar", 8, 1),
}
_psa_cache = {}


def _psa_problem(family, h, w, heads, dtype):
    """Inputs, reference and both bounds, computed once and shared by the routes of one dtype (nothing modifies them)."""
    key = (family, h, w, heads, dtype)
    if key not in _psa_cache:
        qkv, pw, pb = Y.psa_family(family, 2, h, w, heads, dtype, 100 * heads + Y.PSA_FAMILIES.index(family))
        r = Y.psa_ref(qkv, h, w, heads, Y.SCALE, pw, pb)
        bounds = {kind: Y.psa_bound(kind, r, h * w, dtype).reshape(-1, heads * Y.HD) for kind in (("scalar", "mfma") if dtype == BF16 else ("scalar",))}
        _psa_cache[key] = (qkv, pw, pb, r["out"].reshape(-1, heads * Y.HD), bounds)
    return _psa_cache[key]


def _psa_call(qkv, pw, pb, h, w, heads, dtype, extra, off, key_dim=32, head_dim=64, ldqkv=None, code=None, y_in_x=False):
    DEV, L, lib, st = KC.env()
    n, C = qkv.shape[0], heads * Y.HD
    xin = _View(n * h * w, heads * Y.CH, heads * Y.CH + extra, off, dtype, qkv.reshape(n * h * w, heads * Y.CH))
    yout = _View(n * h * w, C, C + 8, 4, dtype)
    pwd, pbd = pw.to(DEV), pb.to(DEV)
    rc = lib.upa_psa_attention(xin.ptr, xin.ld if ldqkv is None else ldqkv, n, h, w, heads, key_dim, head_dim, float(Y.SCALE), pwd.data_ptr(),
                               pbd.data_ptr(), xin.ptr + 2 * xin.ld * _es(dtype) if y_in_x else yout.ptr, yout.ld,
                               L.dtype_code(dtype) if code is None else code, st)
    torch.cuda.synchronize()
    return rc, xin, yout


@pytest.mark.parametrize("heads", Y.PSA_HEADS)
@pytest.mark.parametrize("route", list(PSA_ROUTES))
@KC.stop_after_fault
def test_psa_every_route(route, heads):
    """Seven families x thirteen token counts around the 16-key partitions (15 / 16 / 17: partitions 1 - 3 empty or holding one key), the
    32-query tiles of the matrix-core kernel (31 / 32 / 33), the 64-key blocks (63 / 64 / 65, 127 / 129) and 200, on 1 x W and H x 1
    maps among them; heads 1 / 2 / 3.  The two bf16 scalar routes and the matrix-core route read the same values; each is held to its
    own bound."""
    dtype, kind, extra, off = PSA_ROUTES[route]
    report = []
    for (h, w) in Y.PSA_MAPS:
        for family in Y.PSA_FAMILIES:
            qkv, pw, pb, ref, bounds = _psa_problem(family, h, w, heads, dtype)
            what = f"psa {route} {family} {h}x{w} heads {heads}"
            rc, _, yout = _psa_call(qkv, pw, pb, h, w, heads, dtype, extra, off)
            assert rc == 0, what
            KC.check_bound(yout.payload(what), ref, bounds[kind], what, report)
    KC.print_report(report, f"psa {route} heads {heads}")


@KC.stop_after_fault
def test_psa_refusals_leave_the_output_untouched():
    qkv, pw, pb = Y.psa_family("uniform", 2, 4, 4, 1, F32, 1)
    for kw, want in ((dict(key_dim=16, head_dim=32), UPA_EUNSUPPORTED), (dict(ldqkv=127), UPA_EINVAL), (dict(code=99), UPA_EUNSUPPORTED),
                     (dict(y_in_x=True), UPA_EINVAL)):
        for dtype in (F32, BF16):
            q = qkv if dtype == F32 else Y.stored(qkv, BF16)
            rc, xin, yout = _psa_call(q, pw, pb, 4, 4, 1, dtype, 8, 8 if dtype == BF16 else 4, **kw)
            assert rc == want, (kw, dtype, rc)
            assert yout.untouched(), kw
            if "y_in_x" in kw:
                a = xin.buf.cpu()
                assert bool(torch.isnan(a[:, :xin.off].float()).all()) and torch.equal(a[:xin.rows, xin.off:xin.off + xin.c].float(), q.reshape(32, 128))


# =====================================================================================================================
# upa_conv_transpose2x2
# =====================================================================================================================
def _convt_call(x, wt, bias, dtype, cin=None, x_shift=0):
    DEV, L, lib, st = KC.env()
    n, cin_, h, w = x.shape
    cout = wt.shape[1]
    E, code = 16 // _es(dtype), L.dtype_code(dtype)
    wc = wt.contiguous().float()
    packed = torch.zeros(lib.upa_conv_transpose2x2_packed_weight_bytes(cin_, cout, code), dtype=torch.uint8)
    L.check(lib.upa_pack_conv_transpose2x2_weight(wc.data_ptr(), cin_, cout, code, packed.data_ptr()), "pack")
    assert torch.equal(packed.view(dtype).reshape(4 * cout, -1).float(), Y.convt_pack_ref(wt, dtype))
    xin = _View(n * h * w, cin_, cin_ + 2 * E, E, dtype, _rows(x))
    yout = _View(n * 4 * h * w, cout, cout + 3 * E, E, dtype)
    pd, bd = packed.to(DEV), bias.to(DEV)
    rc = lib.upa_conv_transpose2x2(xin.ptr + x_shift, n, h, w, cin_ if cin is None else cin, xin.ld, pd.data_ptr(), bd.data_ptr(), yout.ptr, cout,
                                   yout.ld, code, st)
    torch.cuda.synchronize()
    return rc, yout


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_conv_transpose2x2_every_tile_shape(dtype):
    """cin with partial MFMA depth steps (f32 depth 4: 4 / 12 / 40; bf16 depth 32: 8 / 40 / 72), 4 cout = 16 / 80 / 160 (f32) and
    32 / 96 / 160 (bf16) columns: partial 64-column blocks of 16 and 32, a second and a third block; 2 / 126 / 128 / 130 pixels: one
    partial 64-pixel block, two ending two pixels short, two full, and a third holding two pixels, with a block spanning both images."""
    cins, couts = Y.CONVT_CH[dtype]
    report = []
    for fi, family in enumerate(Y.CONVT_FAMILIES):
        for (h, w) in Y.CONVT_MAPS:
            for cin in cins:
                for cout in couts:
                    x, wt, bias = Y.convt_family(family, 2, cin, h, w, cout, dtype, cin + cout + fi)
                    what = f"convt {dtype} {family} {h}x{w} {cin}->{cout}"
                    rc, yout = _convt_call(x, wt, bias, dtype)
                    assert rc == 0, what
                    v, S, ref = Y.convt_ref(x, wt, bias)
                    KC.check_bound(yout.payload(what), _rows(ref), _rows(Y.convt_bound(v, S, ref, cin, dtype)), what, report)
    KC.print_report(report, f"convt {dtype}")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@KC.stop_after_fault
def test_conv_transpose2x2_refusals_leave_the_output_untouched(dtype):
    E = 16 // _es(dtype)
    x, wt, bias = Y.convt_family("uniform", 2, 2 * E, 3, 3, E, dtype, 150)
    rc, yout = _convt_call(x, wt, bias, dtype, cin=2 * E - 1)       # cin no multiple of the 16-byte group
    assert rc == UPA_EINVAL and yout.untouched()
    rc, yout = _convt_call(x, wt, bias, dtype, x_shift=_es(dtype))  # input base one element off its 16 bytes
    assert rc == UPA_EINVAL and yout.untouched()
    rc, yout = _convt_call(x, wt, bias, dtype)
    assert rc == 0
    yout.payload("the unvaried call")
