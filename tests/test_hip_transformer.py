"""-m gpu: every `upa_mhsa` instantiation and the RT-DETR row / box / sampling kernels of csrc/transformer.hip, each called
through the C ABI and compared with the float64 references of tests/transformer_ref.py.

Buffers, sentinels, the two bit-identical runs, the per-element bounds and the fault latch: the conventions of tests/kernel_check.py:
outputs have four
spare rows and, where the call takes a pitch, spare columns; input padding is 7.0.  Tolerances are derived in the docstrings."""

import math

import pytest
import torch

from oracle import modules as om
from tests import transformer_ref as TR
from tests import kernel_check as KC

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
SPARE = 4
PAD = 7.0


def _rnd(t, dtype):
    """The values a buffer of `dtype` really stores, as float32."""
    return t.to(dtype).float()


# =====================================================================================================================
# upa_mhsa
# =====================================================================================================================
def _mhsa_pitches(heads, D, dtype, mfma):
    """ldqkv: q | k | v column ranges, rounded up to 16 bytes, plus one 16-byte group of padding.  ldy: the same for one
    range.  ldr: its own pitch - a multiple of 4 for the matrix-core form, = 2 mod 4 otherwise (which keeps bf16 d = 32 on
    the vector kernel at any L: `upa_mhsa` takes the matrix-core form only when ldr % 4 == 0)."""
    E = 16 // torch.empty(0, dtype=dtype).element_size()
    hd = heads * D
    ldqkv = -(-3 * hd // E) * E + E
    ldy = -(-hd // E) * E + E
    ldr = ldy + 4 if mfma else hd + ((2 - hd) % 4 or 4)
    assert ldr != ldy and ldr > hd and (ldr % 4 == 0) == mfma
    return ldqkv, ldy, ldr


def _mhsa_call(q, k, v, res, scale, dtype, mfma, what):
    """q, k, v, res: (n, L, heads, D) CPU float32 holding values `dtype` stores exactly.  Returns y as (n, L, heads, D)."""
    DEV, L_, lib, st = KC.env()
    n, L, heads, D = q.shape
    hd, es = heads * D, torch.empty(0, dtype=dtype).element_size()
    ldqkv, ldy, ldr = _mhsa_pitches(heads, D, dtype, mfma)
    buf = torch.full((n * L, ldqkv), PAD, dtype=dtype)
    for i, t in enumerate((q, k, v)):
        buf[:, i * hd:(i + 1) * hd] = t.reshape(n * L, hd).to(dtype)
    buf = buf.to(DEV)
    rbuf = None
    if res is not None:
        rbuf = torch.full((n * L, ldr), PAD, dtype=dtype)
        rbuf[:, :hd] = res.reshape(n * L, hd).to(dtype)
        rbuf = rbuf.to(DEV)
    ys = [KC.out_buf((n * L,), ldy, dtype, SPARE, dev=DEV) for _ in range(2)]
    for y in ys:
        L_.check(lib.upa_mhsa(buf.data_ptr(), buf.data_ptr() + hd * es, buf.data_ptr() + 2 * hd * es, ldqkv, n, L, heads, D, float(scale),
                              rbuf.data_ptr() if rbuf is not None else None, ldr, y.data_ptr(), ldy, L_.dtype_code(dtype), st), what)
    torch.cuda.synchronize()
    return KC.payload_of_two(ys, n * L, hd, what).reshape(n, L, heads, D)


def _mhsa_families(n, L, heads, D, scale, dtype, g, with_res):
    """(name, q, k, v, residual) of the plain family and of the families that make one wrong key, one dropped rescale or one
    wrong (image, head) offset loud.  All values are rounded to `dtype` here, so the reference sees what the kernel reads."""
    def U(lo, hi):
        return torch.rand(n, L, heads, D, generator=g) * (hi - lo) + lo

    def R(t):
        return _rnd(t, dtype)
    res = R(U(-1, 1)) if with_res else None
    yield "uniform", R(U(-1, 1)), R(U(-1, 1)), R(U(-1, 1)), res
    # phantom key: every true score is about -30, so a key that does not exist (zero fill, the 7.0 padding, a row of the
    # next image) would carry nearly all of the softmax weight and pull the output away from 3
    c = math.sqrt(30.0 / (D * scale))
    yield "phantom", R(torch.full((n, L, heads, D), c)), R(-c * (1 + 0.1 * U(-1, 1))), R(3 + 0.25 * U(-1, 1)), res
    # late maximum: scores rise by >= 1 per key and by >= 40 over the row, so every block / partition rescales what it has
    step = max(1.0, 40.0 / max(L - 1, 1))
    kk = (torch.arange(L, dtype=torch.float32) * step / (D * scale)).view(1, L, 1, 1).expand(n, L, heads, D)
    ql = R(1 + 0.01 * U(-1, 1))
    yield "late", ql, R(kk), R(U(-1, 1)), res
    yield "late_mirrored", ql, R(kk.flip(1)), R(U(-1, 1)), res
    # v constant per (image, head), all different; constants and residuals are multiples of 1/4 below 8, so that constant +
    # residual is a bf16 number and the output rounding is the only error there is
    cst = (1 + 0.25 * torch.arange(n * heads, dtype=torch.float32)).view(n, 1, heads, 1).expand(n, L, heads, D)
    resq = (torch.randint(0, 9, (n, L, heads, D), generator=g).float() * 0.25) if with_res else None
    yield "const_v", R(U(-1, 1)), R(U(-1, 1)), cst.contiguous(), resq


def _mhsa_check(kind, n, L, heads, D, dtype, seed, report):
    """kind: "f32" | "bf16vec" | "mfma".  Bounds against attention_ref on the stored values:
      f32      4 * 2^-24 * (max|s| + sqrt(L)) * max|v| + 2^-23 |residual|: relative error 2^-24 (max|s| + sqrt L) of a softmax weight
               (score rounding, expf argument, the L-term denominator), the factor 4 for expf / fmaf ordering;
      bf16vec  the same accumulation in f32 and one rounding of the output: + 2^-8 |y_ref|;
      mfma     weights rounded to bf16 (2^-9 each, denominator in f32) before the second product: 2^-7 max|v| + 2^-8 |y_ref|;
               with v constant the rounded weights cancel against the exact ones up to 2^-9: only the output rounding."""
    g = torch.Generator().manual_seed(seed)
    for scale in (1.0, D ** -0.5):
        for with_res in (False, True):
            for name, q, k, v, res in _mhsa_families(n, L, heads, D, scale, dtype, g, with_res):
                what = f"mhsa {kind} {name} L={L} D={D} scale={scale:.3g} res={with_res}"
                y = _mhsa_call(q, k, v, res, scale, dtype, kind == "mfma", what).double()
                ref = TR.attention_ref(q, k, v, scale, res)
                s = TR.attention_scores(q, k, scale)
                if name == "phantom":
                    assert float(s.max()) <= -20.0 and float((ref - (0 if res is None else res.double())).min()) > 2.7
                if name.startswith("late") and L > 1:
                    assert float((s.max(-1).values - s.min(-1).values).min()) >= 30.0
                vmax = float(v.abs().max())
                f32b = 4 * U24 * (float(s.abs().max()) + math.sqrt(L)) * vmax + (0 if res is None else 2 * U24 * res.double().abs())
                if kind == "f32":
                    bound = f32b + torch.zeros_like(ref)
                elif kind == "bf16vec":
                    bound = f32b + 2.0 ** -8 * ref.abs()
                else:
                    bound = (0.0 if name == "const_v" else 2.0 ** -7 * vmax) + 2.0 ** -8 * ref.abs()
                # measured on MI355X (worst error / bound): f32 0.80 on the late-maximum families at D = 64, L = 130 (64-term score sums
                # of |s| ~ 130; a float32 CPU emulation of the four-partition online softmax gives the same 0.80), 0.32 on the uniform
                # family; bf16 vector 0.996 (the output rounding itself: half an ulp at the foot of a binade); matrix-core 0.40
                KC.check_bound(y, ref, bound, what, report)
                if name == "const_v" and res is None:  # a pix0 or h * D slip shows as another head's constant
                    assert float((y - v.double()).abs().max()) <= 2.0 ** -8 * float(v.max())


@pytest.mark.parametrize("L", [1, 5, 63, 64, 65, 130])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [4, 8, 16, 32, 64])
@KC.stop_after_fault
def test_mhsa_vector_every_head_dim(D, dtype, L):
    """mhsa_kernel<float | bf16, D, 4> for every D: n = 2, heads = 3, q / k / v three column ranges of one padded buffer, y and
    the residual on pitches of their own.  L = 1 / 5 leave key partitions without keys, 63 / 64 / 65 straddle a 64-query block,
    130 takes three.  The residual pitch is 2 mod 4, which keeps bf16 d = 32 off the matrix-core kernel at L >= 16 too."""
    report = []
    _mhsa_check("f32" if dtype == torch.float32 else "bf16vec", 2, L, 3, D, dtype, 1000 * D + L, report)
    KC.print_report(report, f"mhsa vector D={D} {dtype} L={L}")


def _mfma_max_keys():
    """launch_mhsa_mfma: Lp * 64 (K image) + 32 * (Lp / 2 + 4) * 4 (V^T image) <= 158 KiB with Lp = L rounded up to 32."""
    lp = (158 * 1024 - 32 * 4 * 4) // (64 + 64)
    return lp // 32 * 32


@pytest.mark.parametrize("n,heads", [(1, 1), (2, 4)], ids=["n1h1", "n2h4"])
@pytest.mark.parametrize("L", [16, 17, 31, 32, 33, 48, 143, 300])
@KC.stop_after_fault
def test_mhsa_mfma_tails_and_scale(L, n, heads):
    """mhsa_mfma_bf16_d32_kernel (bf16, d = 32, ldr % 4 == 0, L >= 16): the second 16-key tile of the last block empty (16, 48's
    second block), partial (17, 31, 33, 143, 300) or full (32); 9 (L = 143) and 19 (L = 300) query tiles that do not fill
    chunks x waves, so one wave's tile lies past L."""
    report = []
    _mhsa_check("mfma", n, L, heads, 32, torch.bfloat16, 7000 + L * 10 + heads, report)
    KC.print_report(report, f"mhsa mfma L={L} n={n} heads={heads}")


@KC.stop_after_fault
def test_mhsa_mfma_largest_key_count():
    """The largest L the matrix-core launch admits (1248 keys: 156.5 KiB of LDS), n = heads = 1; the vector kernel would refuse
    it (128 L + 34816 bytes > 158 KiB), so a pass is the matrix-core kernel's."""
    L = _mfma_max_keys()
    assert L == 1248 and 2 * L * 32 * 2 + 4 * 34 * 64 * 4 > 158 * 1024
    g = torch.Generator().manual_seed(11)
    report = []
    scale = 32 ** -0.5
    for name, q, k, v, res in _mhsa_families(1, L, 1, 32, scale, torch.bfloat16, g, True):
        what = f"mhsa mfma {name} L={L}"
        y = _mhsa_call(q, k, v, res, scale, torch.bfloat16, True, what).double()
        ref = TR.attention_ref(q, k, v, scale, res)
        bound = (0.0 if name == "const_v" else 2.0 ** -7 * float(v.abs().max())) + 2.0 ** -8 * ref.abs()
        KC.check_bound(y, ref, bound, what, report)
    KC.print_report(report, "mhsa mfma largest L")


@KC.stop_after_fault
def test_mhsa_refuses_what_does_not_fit():
    """One key past what LDS holds, a head dim without an instantiation, a pitch that is no multiple of 16 bytes: UpaError with
    the library's message, nothing launched, the output untouched."""
    DEV, L_, lib, st = KC.env()

    def attempt(dtype, L, D, ldqkv=None):
        heads, n = 1, 1
        es = torch.empty(0, dtype=dtype).element_size()
        ld, ldy, _ = _mhsa_pitches(heads, max(D, 16), dtype, True)
        ld = ld if ldqkv is None else ldqkv
        buf = torch.zeros(n * L + 1, max(ld, 3 * D) + 16, dtype=dtype, device=DEV)
        y = KC.out_buf((n * L,), ldy, dtype, SPARE, dev=DEV)
        try:
            L_.check(lib.upa_mhsa(buf.data_ptr(), buf.data_ptr() + D * es, buf.data_ptr() + 2 * D * es, ld, n, L, heads, D, 1.0,
                                  None, 0, y.data_ptr(), ldy, L_.dtype_code(dtype), st), "mhsa")
        finally:
            torch.cuda.synchronize()
            assert bool(torch.isnan(y.float()).all()), "a refused call wrote to its output"

    # f32, D = 64: 2 * L * 64 * 4 + 4 * 66 * 64 * 4 <= 158 KiB  <=>  L <= 184
    l64 = (158 * 1024 - 4 * 66 * 64 * 4) // (2 * 64 * 4)
    assert l64 == 184
    with pytest.raises(L_.UpaError, match=f"mhsa: {l64 + 1} keys x 64 dims do not fit LDS"):
        attempt(torch.float32, l64 + 1, 64)
    # bf16, D = 32: past the matrix-core limit (1248) and therefore past the vector kernel's (992) as well
    lm = _mfma_max_keys()
    assert lm + 1 > (158 * 1024 - 4 * 34 * 64 * 4) // (2 * 32 * 2)
    with pytest.raises(L_.UpaError, match=f"mhsa: {lm + 1} keys x 32 dims do not fit LDS"):
        attempt(torch.bfloat16, lm + 1, 32)
    with pytest.raises(L_.UpaError, match=r"mhsa: head dim 12 not supported \(4, 8, 16, 32, 64\)"):
        attempt(torch.float32, 20, 12)
    with pytest.raises(L_.UpaError, match="mhsa: strides must be multiples of 16 bytes"):
        attempt(torch.float32, 20, 16, ldqkv=50)
    with pytest.raises(L_.UpaError, match="mhsa: strides must be multiples of 16 bytes"):
        attempt(torch.bfloat16, 20, 32, ldqkv=100)


# =====================================================================================================================
# upa_layer_norm
# =====================================================================================================================
@pytest.mark.parametrize("M", [1, 3, 6, 301])
@pytest.mark.parametrize("C", [1, 8, 100, 256, 1000])
@KC.stop_after_fault
def test_layer_norm_rows(C, M):
    """layer_norm_kernel (one wave per row, four rows per workgroup) at C below / across / not a multiple of the 64 lanes and at
    M % 4 != 0, on zero-mean, mean-30 and mean-1000 rows (sigma about 1) and on rows of one repeated value (sigma = 0: the output
    is beta).  Per row: |err| <= 8 * 2^-24 * (max|x + r| / sqrt(var + eps) + max|y_ref|) * max|gamma| - one rounding of x + r, of
    the mean and of the difference each move the normalised value by 2^-24 max|x + r| / sigma, the scale and shift round at
    2^-24 |y|; F.layer_norm in float32 stays within 1.64 of that unit, the factor 8 covers this kernel's reduction tree."""
    DEV, L_, lib, st = KC.env()
    g = torch.Generator().manual_seed(31 * C + M)
    gamma = torch.rand(C, generator=g) * 1.5 + 0.25
    gamma[0] = -1.75
    beta = torch.randn(C, generator=g)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    report = []
    for family, mean in (("zero_mean", 0.0), ("mean30", 30.0), ("mean1000", 1000.0), ("all_equal", None)):
        if mean is None:
            x = (torch.rand(M, 1, generator=g) * 60 - 20).expand(M, C).contiguous()
        else:
            x = torch.randn(M, C, generator=g) + mean
        for with_res in (False, True):
            if with_res:
                r = torch.randn(M, 1, generator=g).expand(M, C).contiguous() if mean is None else torch.randn(M, C, generator=g) * 0.5
            else:
                r = None
            xd, rd = x.to(DEV), (r.to(DEV) if with_res else None)
            for eps in (1e-5, 1e-3):
                what = f"layer_norm {family} C={C} M={M} res={with_res} eps={eps}"
                ys = [KC.out_buf((M,), C, torch.float32, SPARE, dev=DEV) for _ in range(2)]
                for y in ys:
                    L_.check(lib.upa_layer_norm(xd.data_ptr(), rd.data_ptr() if with_res else None, M, C, gd.data_ptr(), bd.data_ptr(), eps,
                                                y.data_ptr(), st), what)
                torch.cuda.synchronize()
                y = KC.payload_of_two(ys, M, C, what).double()
                ref = TR.layer_norm_ref(x, r, gamma, beta, eps)
                z = x.double() + (r.double() if with_res else 0)
                var = z.var(-1, unbiased=False, keepdim=True)
                bound = 8 * U24 * (z.abs().amax(-1, keepdim=True) / torch.sqrt(var + eps) + ref.abs().amax(-1, keepdim=True)) * float(gamma.abs().max())
                # measured on MI355X: 0.73 of the bound on the all-equal rows at C = 1000, M = 301, eps = 1e-5 (the rounded mean of 1000
                # equal values times 1 / sqrt(eps); a float32 CPU emulation of the lane-strided sums and the xor butterfly gives the same
                # figure), 0.29 on the mean-1000 family
                KC.check_bound(y, ref, bound.expand_as(ref), what, report)
    KC.print_report(report, f"layer_norm C={C} M={M}")


# =====================================================================================================================
# upa_rows_add / upa_rows_scale / upa_rows_gather
# =====================================================================================================================
@pytest.mark.parametrize("M,C", [(1, 1), (7, 100), (300, 256), (8200, 256)], ids=["1x1", "7x100", "300x256", "8200x256"])
@KC.stop_after_fault
def test_row_utilities_exact(M, C):
    """rows_kernel in its three modes, bit for bit against torch on the CPU.  8200 x 256 elements are more than the 8192 x 256
    threads the grid is capped at: the grid-stride loop takes a second trip.  Gather: descending, the first and the last source
    row, repeats, and more output rows than source rows."""
    DEV, L_, lib, st = KC.env()
    g = torch.Generator().manual_seed(M + C)
    a, b = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g) * 3
    sc = torch.randn(M, generator=g)
    sc[0] = 0.0
    ms = min(M, 300)                                    # source rows of the gather
    m_out = M if M > 300 else 2 * M + 2                 # > ms
    idx = torch.cat([torch.arange(ms - 1, -1, -1), torch.tensor([0, ms - 1]), (torch.arange(max(m_out - ms - 2, 0)) * 7) % ms])[:m_out].to(torch.int32)
    assert idx.numel() == m_out and m_out > ms and int(idx.max()) == ms - 1 and int(idx.min()) == 0
    ad, bd, scd, idxd = a.to(DEV), b.to(DEV), sc.to(DEV), idx.to(DEV)
    src = a[:ms].contiguous()
    srcd = src.to(DEV)

    def run(fn, rows, *args):
        ys = [KC.out_buf((rows,), C, torch.float32, SPARE, dev=DEV) for _ in range(2)]
        for y in ys:
            L_.check(fn(*args, y.data_ptr(), rows, C, st), fn.__name__)
        torch.cuda.synchronize()
        return KC.payload_of_two(ys, rows, C, fn.__name__)

    assert torch.equal(KC.bits(run(lib.upa_rows_add, M, ad.data_ptr(), bd.data_ptr())), KC.bits(a + b))
    assert torch.equal(KC.bits(run(lib.upa_rows_scale, M, ad.data_ptr(), scd.data_ptr())), KC.bits(a * sc[:, None]))
    assert torch.equal(KC.bits(run(lib.upa_rows_gather, m_out, srcd.data_ptr(), idxd.data_ptr())), KC.bits(src[idx.long()]))


# =====================================================================================================================
# upa_box_refine / upa_box_add_anchors / upa_sigmoid / upa_rtdetr_output
# =====================================================================================================================
def _flat_call(fn, n_rows, cols, tail, what, *inputs):
    """fn(inputs..., y, *tail, stream) with the CPU tensors `inputs` uploaded and y a contiguous (n_rows, cols) output."""
    DEV, L_, lib, st = KC.env()
    dev = [t.to(DEV) for t in inputs]
    ys = [KC.out_buf((n_rows,), cols, torch.float32, SPARE, dev=DEV) for _ in range(2)]
    for y in ys:
        L_.check(fn(*[t.data_ptr() for t in dev], y.data_ptr(), *tail, st), what)
    torch.cuda.synchronize()
    return KC.payload_of_two(ys, n_rows, cols, what, finite=False)   # (the +inf anchors of invalid tokens are values here)


@KC.stop_after_fault
def test_box_arithmetic_edges():
    """box_kernel's three modes and rtdetr_output_kernel at what the decoder tests never feed them: references at and beyond the
    inverse_sigmoid clamps (0, 1, eps = 1e-5) crossed with deltas up to +-30, the +inf anchors of invalid tokens, sigmoid
    arguments up to +-1e4, and box counts that are no multiple of the 64 boxes of a workgroup.
    box_refine: |err| <= 4 * 2^-24 (outputs in [0, 1]) and exactly 0 / 1 where the float64 value rounds to them in float32.
    sigmoid / score columns: |err| <= 2 * 2^-24 (expf, the sum and the quotient round once each on a value <= 1).
    Measured on MI355X: box_refine 0.17 of its bound, sigmoid 0.16, score columns 0.74 (a sigmoid just under 1: one ulp there is 2^-24)."""
    DEV, L_, lib, st = KC.env()
    # ---- box_refine: 40 (reference, delta) pairs, tiled to 70 boxes = 280 values: two workgroups, the second partial
    n_boxes = 70
    ref = torch.tensor(TR.BOX_REFS, dtype=torch.float32).repeat_interleave(len(TR.BOX_DELTAS)).repeat(7).view(n_boxes, 4)
    dl = torch.tensor(TR.BOX_DELTAS, dtype=torch.float32).repeat(len(TR.BOX_REFS)).repeat(7).view(n_boxes, 4)
    y = _flat_call(lib.upa_box_refine, n_boxes, 4, (n_boxes,), "box_refine", dl, ref)
    assert not bool(torch.isnan(y).any())
    want = TR.box_refine_ref(dl, ref)
    err = (y.double() - want).abs()
    print(f"box_refine: worst error / bound = {float(err.max()) / (4 * U24):.3f}")
    assert float(err.max()) <= 4 * U24
    w32 = want.float()
    assert int((w32 == 1).sum()) >= 7 and torch.equal(y == 1, w32 == 1) and torch.equal(y == 0, w32 == 0)
    assert bool(((y >= 0) & (y <= 1)).all())

    # ---- box_add_anchors: the reference's anchors for a 2 x 64 and a 1 x 3 map (the 64-wide map's edge columns are invalid:
    # +inf rows), token indices out of order and repeated, 131 boxes
    anchors, valid = om.RTDETRDecoder._generate_anchors([[2, 64], [1, 3]])
    anchors, valid = anchors[0].contiguous(), valid[0, :, 0]
    T = anchors.shape[0]
    assert T == 131 and 0 < int((~valid).sum()) < T and bool(torch.isinf(anchors[~valid]).all())
    g = torch.Generator().manual_seed(17)
    tok = torch.cat([torch.arange(T - 1, -1, -1), torch.tensor([0, T - 1, 0, 5, 5])]).to(torch.int32)
    nb = tok.numel()
    assert nb % 64 != 0
    d = torch.randn(nb, 4, generator=g) * 3
    y = _flat_call(lib.upa_box_add_anchors, nb, 4, (nb,), "box_add_anchors", d, tok, anchors)
    want = TR.box_add_anchors_ref(d, tok, anchors)
    assert torch.equal(KC.bits(y), KC.bits(want))
    bad = ~valid[tok.long()]
    assert bool((y[bad] == float("inf")).all()) and bool(torch.isfinite(y[~bad]).all())
    s = _flat_call(lib.upa_sigmoid, nb, 4, (nb * 4,), "sigmoid(anchored boxes)", y.contiguous())
    assert not bool(torch.isnan(s).any()) and bool((s[bad] == 1.0).all())
    assert float((s.double() - torch.sigmoid(want.double())).abs().max()) <= 2 * U24

    # ---- sigmoid at the ends of expf's range
    mags = [0.0, 1e-8, 1.0, 20.0, 88.0, 104.0, 1e4]
    x = torch.tensor([m for m in mags] + [-m for m in mags], dtype=torch.float32)
    s = _flat_call(lib.upa_sigmoid, 1, x.numel(), (x.numel(),), "sigmoid", x)[0]
    want = torch.sigmoid(x.double())
    err = (s.double() - want).abs()
    print(f"sigmoid: worst error / bound = {float(err.max()) / (2 * U24):.3f}")
    assert not bool(torch.isnan(s).any()) and float(err.max()) <= 2 * U24
    assert s[0] == 0.5 and s[7] == 0.5 and bool((s[4:7] == 1).all()) and bool((s[12:] == 0).all())
    nrm = want >= 2.0 ** -126  # a relative gate where the result is a normal float32: 8 ulp
    assert bool((err[nrm] <= 8 * U24 * want[nrm]).all())

    # ---- rtdetr_output
    worst = 0.0
    for nc in (1, 3, 80):
        for M in (1, 5, 600):
            boxes = torch.rand(M, 4, generator=g)
            scores = torch.randn(M, nc, generator=g) * 6
            scores.view(-1)[0] = 104.0
            scores.view(-1)[-1] = -104.0
            y = _flat_call(lib.upa_rtdetr_output, M, 4 + nc, (M, nc), f"rtdetr_output nc={nc} M={M}", boxes, scores)
            assert not bool(torch.isnan(y).any())
            want = TR.rtdetr_output_ref(boxes, scores)
            assert torch.equal(KC.bits(y[:, :4]), KC.bits(want[:, :4].float()))
            e = float((y[:, 4:].double() - want[:, 4:]).abs().max())
            worst = max(worst, e)
            assert e <= 2 * U24, (nc, M, e)
    print(f"rtdetr_output: worst score error / bound = {worst / (2 * U24):.3f}")


# =====================================================================================================================
# upa_msdeform_attn_strided
# =====================================================================================================================
MAPS = [(5, 7), (4, 4), (2, 3), (1, 1)]
BORDER = (-1.0, -0.5, 0.0, "W-1", "W-0.5", "W")


def _msd_inputs(family, logit_family, shapes, bs, nq, heads, g):
    """offsets (bs*nq, heads*nl*4*2), logits (bs*nq, heads*nl*4), ref boxes (bs*nq, 4).
    Everything that positions a sample lies on a binary grid (centres on 1/64, sizes on 1/16, offsets on 1/8 or finer), so that
    loc = ref_xy + off / 4 * ref_wh / 2 and the pixel coordinate ((2 loc - 1 + 1) * W - 1) / 2 are exact in float32 for W <= 7:
    kernel and reference then sample the same point, and the tolerance has to cover the corner weights, the softmax and the
    sums only - not a rounded position times the slope of the value map, which it does not contain."""
    nl, NP = len(shapes), 4
    Q = bs * nq
    ref = torch.cat([torch.randint(8, 57, (Q, 2), generator=g).float() / 64, torch.randint(1, 11, (Q, 2), generator=g).float() / 16], 1)
    shape = (Q, heads, nl, NP, 2)
    if family == "inside":       # |displacement| <= 1 / 4 * 10/16 / 2 < 0.08 around centres in [0.125, 0.875]
        off = torch.randint(-8, 9, shape, generator=g).float() / 8
    elif family == "share_outside":
        off = torch.randint(-48, 49, shape, generator=g).float() / 8
    elif family == "wild":       # boxes twice the image: +-3e9 / 4 * 2 / 2 * W is past 2^31 for W >= 3; every corner is outside
        ref[:, 2:] = 2.0
        mag = torch.tensor([1e6, 3e9])[torch.randint(0, 2, shape, generator=g)]
        off = mag * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    else:                        # "border": unit boxes at the centre, loc = 0.5 + off / 8; pixel coordinates -1, -0.5, 0, W-1, W-0.5, W
        ref[:, :2], ref[:, 2:] = 0.5, 1.0
        off = torch.empty(shape)
        cnt = 0
        for l, (H, W) in enumerate(shapes):
            for a, size in ((0, W), (1, H)):
                tgt = torch.tensor([{"W-1": size - 1.0, "W-0.5": size - 0.5, "W": float(size)}.get(t, t) for t in BORDER])
                pick = tgt[torch.randint(0, 6, (Q, heads, NP), generator=g)]
                pick[cnt % Q, :, :] = tgt[torch.arange(heads * NP).view(heads, NP) % 6]  # every target at least once
                cnt += 1
                loc = torch.round((pick + 0.5) / size * 4096) / 4096   # exact for sizes 1, 2, 4; within size / 8192 of it otherwise
                off[:, :, l, :, a] = (loc - 0.5) * 8
    lg = torch.rand(Q, heads, nl * NP, generator=g) * 6 - 3
    if logit_family == "peaked":
        hot = (torch.arange(Q).view(Q, 1) + torch.arange(heads).view(1, heads)) % (nl * NP)
        lg.scatter_add_(2, hot.unsqueeze(-1), torch.full((Q, heads, 1), 40.0))
    return off.reshape(Q, -1).contiguous(), lg.reshape(Q, -1).contiguous(), ref.contiguous()


@pytest.mark.parametrize("n_levels", [1, 2, 3, 4])
@pytest.mark.parametrize("vdtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("d", [8, 32])
@KC.stop_after_fault
def test_msdeform_vs_f64_grid_sample(d, vdtype, n_levels):
    """msdeform_kernel<8 | 32, 4, float | bf16> against the oracle's grid_sample formulation in float64: 1 - 4 levels of odd maps,
    15 and 80 (b, q, head) items (a partial block either way), a value pitch wider than heads * d with 7.0 next to the data,
    samples inside, on the borders, partly outside and absurdly far outside (+-1e6, +-3e9: exactly 0 and nothing non-finite),
    flat and one-hot softmax weights.  f32 values: |err| <= 8 * 2^-24 * max|v| (positions are exact, see _msd_inputs: four corner
    products, the softmax quotient and <= 64 additions of terms whose weights sum to 1).  bf16 values: the reference gets the same
    bf16-rounded values, what differs is v_exp_f32 / v_rcp_f32 and the order of the sums: 2e-5 * max|v|.
    The +-3e9 offsets are what found the unclamped `(int)floorf(ix)` of the exact-f32 branch: the coordinate converts to INT_MAX,
    `x0 + 1` wraps, the compiled range test `x0 > -2 && x0 + 1 < W` holds for the wrapped value, and the corner load went to a wild
    address (an illegal memory access, not a wrong number); the branch now clamps the integer corner as the bf16 branch does."""
    DEV, L_, lib, st = KC.env()
    shapes = MAPS[:n_levels]
    T = sum(h * w for h, w in shapes)
    shp = torch.tensor([v for s_ in shapes for v in s_], dtype=torch.int32)
    g = torch.Generator().manual_seed(100 * d + 10 * n_levels + (vdtype == torch.bfloat16))
    report = []
    for bs, nq, heads in ((1, 5, 3), (2, 10, 4)):
        C = heads * d
        ldv = C + 8
        rows = _rnd(torch.rand(bs * T, C, generator=g) * 2 - 1, vdtype)
        vbuf = torch.full((bs * T, ldv), PAD, dtype=vdtype)
        vbuf[:, :C] = rows.to(vdtype)
        vd = vbuf.to(DEV)
        vmax = float(rows.abs().max())
        tol = (8 * U24 if vdtype == torch.float32 else 2e-5) * vmax
        for family in ("inside", "border", "share_outside", "wild"):
            for lf in ("uniform", "peaked"):
                what = f"msdeform d={d} {vdtype} levels={n_levels} items={bs * nq * heads} {family} {lf}"
                off, lg, ref = _msd_inputs(family, lf, shapes, bs, nq, heads, g)
                offd, lgd, refd = off.to(DEV), lg.to(DEV), ref.to(DEV)
                ys = [KC.out_buf((bs * nq,), C, torch.float32, SPARE, dev=DEV) for _ in range(2)]
                for y in ys:
                    L_.check(lib.upa_msdeform_attn_strided(vd.data_ptr(), L_.dtype_code(vdtype), ldv, shp.data_ptr(), n_levels, bs, heads, d,
                                                           offd.data_ptr(), lgd.data_ptr(), refd.data_ptr(), nq, 4, y.data_ptr(), st), what)
                torch.cuda.synchronize()
                y = KC.payload_of_two(ys, bs * nq, C, what).double()
                want = TR.msdeform_ref(rows, shapes, bs, heads, d, off, lg, ref)
                if family == "wild":
                    assert bool((want == 0).all()) and bool((y == 0).all()), f"{what}: a sample far outside the map contributed"
                    continue
                if family in ("inside", "border"):
                    assert float(want.abs().max()) > 0.05
                e = float((y - want).abs().max())
                report.append((e / tol, what))
                # measured on MI355X: f32 values 0.72 of the bound at worst (d = 32, three levels, 15 items), 0.31-0.41 elsewhere;
                # bf16 values 0.015
                assert e <= tol, f"{what}: error {e:.3g} > {tol:.3g}"
    KC.print_report(report, f"msdeform d={d} {vdtype} levels={n_levels}")
