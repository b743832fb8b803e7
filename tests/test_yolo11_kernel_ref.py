"""CPU: tests/yolo11_kernel_ref.py itself.  The three float64 references against nested loops and hand-worked values; float32
emulations of the arithmetic order of dwconv3_kernel, convt2x2_kernel, psa_attn_kernel and psa_attn_mfma_kernel, which must lie inside
the derived bounds on every family at every shape tests/test_hip_yolo11_kernels.py walks; the same emulations with one defect each,
which must leave the bound on the family built to catch it; the families' stated conditions; the host-side ConvTranspose packer.

Worst error / bound of the unmutated emulations (pytest -s prints them): dwconv f32 0.250, bf16 0.989; convt f32 0.327, bf16 0.995;
psa scalar f32 0.171, scalar bf16 0.995, mfma 0.988 (the bf16 figures are the output rounding itself: half an ulp at the foot of a
binade).  The emulations take exp / exp2 correctly rounded from float64 and sum each MFMA's products one by one in f32."""

import math

import pytest
import torch
import torch.nn.functional as F

from tests import yolo11_kernel_ref as Y
from tests.conv_ref import ACT_NONE, ACT_SILU, F64, stored

BF16, F32 = torch.bfloat16, torch.float32
NEG_INF = float("-inf")


def _fma(a, b, c):
    """fmaf on float32 tensors: the product of two floats is exact in float64, the sum is rounded once more only at a float32 tie."""
    return (a.double() * b.double() + c.double()).float()


def _exp(x):
    return torch.exp(x.double()).float()


def _exp2(x):
    return torch.exp2(x.double()).float()


def _worst(y, ref, bound):
    err = (y.double() - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return float(ratio.max())


# =====================================================================================================================
# emulations (mutant = None: what the kernel does)
# =====================================================================================================================
def emu_dw(x, w9c, bias, stride, act, out_dtype, mutant=None):
    """dwconv3_kernel: acc = 0, one fmaf per in-range tap in (ky, kx) order (a zero-padded tap leaves acc unchanged, as the skipped
    one does), acc + bias, SiLU as v / (1 + exp(-v)) in f32, one rounding into the output type."""
    n, c, h, w = x.shape
    oh, ow = Y.dw_out_hw(h, w, stride)
    xp = F.pad(x.float(), (1, 1, 1, 2))
    off = 1 if (mutant == "row_start" and stride == 2) else 0  # rows from oy * 2 instead of oy * 2 - 1
    acc = torch.zeros(n, c, oh, ow)
    for ky in range(3):
        for kx in range(3):
            sl = xp[:, :, ky + off:ky + off + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride]
            acc = _fma(sl, w9c[ky * 3 + kx].view(1, c, 1, 1), acc)
    if mutant == "drop_channel":  # the last channel's taps never accumulated
        acc[:, c - 1] = 0.0
    acc = acc + bias.view(1, c, 1, 1)
    if act == ACT_SILU:
        acc = acc / (1.0 + _exp(-acc))
    return stored(acc, out_dtype)


def emu_convt(x, w, bias, out_dtype, mutant=None):
    """convt2x2_kernel: per output element an f32 chain over the input channels in ascending order (16x16x4 f32 MFMA: fused rounding
    per step; 16x16x32 bf16 MFMA: exact products, summed here one by one), + bias, one rounding into the output type."""
    n, cin, h, wd = x.shape
    cout = w.shape[1]
    if mutant == "swap_taps":  # taps 1 and 2 exchanged: (i, j) = (0, 1) <-> (1, 0)
        w = w.transpose(2, 3)
    acc = torch.zeros(n, cout, h, 2, wd, 2)
    for ci in range(cin - 1 if mutant == "drop_channel" else cin):
        acc = _fma(x[:, ci].float()[:, None, :, None, :, None], w[ci].float()[None, :, None, :, None, :], acc)
    acc = acc + bias.view(1, cout, 1, 1, 1, 1)
    return stored(acc.reshape(n, cout, 2 * h, 2 * wd), out_dtype)


def _emu_scores(qr, k, Np, dims):
    """s[p, key] = fmaf chain over `dims` dims, keys padded with zeros to Np."""
    n, heads, N, _ = qr.shape
    kp = torch.zeros(n, heads, Np, Y.KD)
    kp[:, :, :N] = k
    s = torch.zeros(n, heads, N, Np)
    for i in range(dims):
        s = _fma(qr[..., i:i + 1], kp[..., i].unsqueeze(-2), s)
    return s


def _emu_pe(os_, qkv, h, w, heads, pw, pb, out_dtype, mutant):
    """psa_pe_epilogue: acc = pb, one fmaf per in-range tap in (dy, dx) order on v read from qkv, os + acc, one rounding."""
    n, N, C = qkv.shape[0], h * w, heads * Y.HD
    v = Y.psa_split(qkv.float(), heads)[2].permute(0, 2, 1, 3).reshape(n, N, C)
    p = torch.arange(N)
    py, px = p // w, p % w
    acc = pb.view(1, 1, C).expand(n, N, C).clone()
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            iy, ix = py + dy, px + dx
            src = iy * w + ix
            ok = (iy >= 0) & (iy < h) & (src >= 0) & (src < N)
            if mutant != "pe_no_border":
                ok = ok & (ix >= 0) & (ix < w)
            tap = (dx + 1) * 3 + dy + 1 if mutant == "pe_transposed" else (dy + 1) * 3 + dx + 1
            xv = v[:, src.clamp(0, N - 1)] * ok.view(1, N, 1).float()
            acc = _fma(pw[tap].view(1, 1, C), xv, acc)
    val = os_.permute(0, 2, 1, 3).reshape(n, N, C) + acc
    return stored(val.reshape(n, h, w, C), out_dtype)


def emu_psa_scalar(qkv, h, w, heads, scale, pw, pb, out_dtype, mutant=None):
    """psa_attn_kernel<T, 32, 64>: q * scale rounded, 32 fmaf per logit; per query four online-softmax states, partition `part`
    walking keys [16 part, 16 part + 16) of every 64-key block (jn keys of the last), each key mn = max(m, s), alpha = expf(m - mn),
    p = expf(s - mn), l = l * alpha + p (two roundings), o = fmaf(p, v, o * alpha); the merge in partition order with
    expf(m_part - max) (an empty partition has m = -inf, l = 0: factor 0); o * (1 / l); the pe epilogue."""
    n, N = qkv.shape[0], h * w
    q, k, v = (t.float() for t in Y.psa_split(qkv, heads))
    if mutant == "swap_qk":
        q, k = k, q
    if mutant == "neighbour_v":
        v = torch.roll(v, 1, dims=1)
    qr = q if mutant == "no_scale" else q * torch.tensor(scale, dtype=F32)
    Np = -(-N // 64) * 64
    s = _emu_scores(qr, k, Np, Y.KD - 1 if mutant == "drop_channel" else Y.KD)
    vp = torch.zeros(n, heads, Np, Y.HD)
    vp[:, :, :N] = v
    m = torch.full((n, heads, N, 4), NEG_INF)
    l = torch.zeros(n, heads, N, 4)
    o = torch.zeros(n, heads, N, 4, Y.HD)
    for k0 in range(0, N, 64):
        for jj in range(16):
            keys = k0 + 16 * torch.arange(4) + jj
            valid = torch.ones(4, dtype=torch.bool) if mutant == "unmasked" else keys < N
            if not bool(valid.any()):
                break
            sj, vj = s[..., keys], vp[:, :, keys].unsqueeze(2)
            mn = torch.maximum(m, sj)
            alpha = torch.ones_like(m) if mutant == "no_alpha" else _exp(m - mn)
            pj = _exp(sj - mn)
            l_new = l * alpha + pj
            o_new = _fma(pj.unsqueeze(-1), vj, o * alpha.unsqueeze(-1))
            m, l = torch.where(valid, mn, m), torch.where(valid, l_new, l)
            o = torch.where(valid.view(4, 1), o_new, o)
    # mutant: emptiness decided from the last block alone, so a partition with keys in earlier blocks is left out
    parts = [p for p in range(1, 4) if not (mutant == "merge_skip" and (N - 1) % 64 < 16 * p)]
    mm = m[..., 0]
    for p in parts:
        mm = torch.maximum(mm, m[..., p])
    a0 = _exp(m[..., 0] - mm)
    lt, ot = l[..., 0] * a0, o[..., 0, :] * a0.unsqueeze(-1)
    for p in parts:
        aq = _exp(m[..., p] - mm)
        lt = lt + l[..., p] * aq
        ot = _fma(o[..., p, :], aq.unsqueeze(-1), ot)
    os_ = ot * (1.0 / lt).unsqueeze(-1)
    return _emu_pe(os_, qkv, h, w, heads, pw, pb, out_dtype, mutant)


def emu_psa_mfma(qkv, h, w, heads, scale, pw, pb, out_dtype, mutant=None):
    """psa_attn_mfma_kernel: logit = f32 sum of 32 exact bf16 products, t = logit * c_log2 with c_log2 = scale * log2(e) in f32, padded
    keys -inf; per 64-key block one rescale alpha = exp2(m - mn), p = exp2(t - mn); the denominator sums the unrounded p (16 per lane,
    four lanes per query, added across lanes at the end), the numerator takes p rounded to bf16 (nearest even) in two 32-key MFMAs
    after o * alpha; o * (1 / l); the pe epilogue."""
    n, N = qkv.shape[0], h * w
    q, k, v = (t.float() for t in Y.psa_split(qkv, heads))
    nb = -(-N // 64)
    Np = nb * 64
    c_log2 = torch.tensor(scale, dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32)
    t = _emu_scores(q, k, Np, Y.KD) * c_log2
    if mutant != "unmasked":
        t[..., N:] = NEG_INF
    vp = torch.zeros(n, heads, Np, Y.HD)
    vp[:, :, :N] = v
    m = torch.full((n, heads, N), NEG_INF)
    l = torch.zeros(n, heads, N, 4)
    o = torch.zeros(n, heads, N, Y.HD)
    for b in range(nb):
        tb = t[..., b * 64:(b + 1) * 64]
        mn = torch.maximum(m, tb.max(-1).values)
        alpha = torch.ones_like(m) if mutant == "no_alpha" else _exp2(m - mn)
        p = _exp2(tb - mn.unsqueeze(-1))
        lane = p.reshape(n, heads, N, 4, 4, 4).permute(0, 1, 2, 4, 3, 5).reshape(n, heads, N, 4, 16)  # [g][tt * 4 + e]: key 16 tt + 4 g + e
        ps = torch.zeros(n, heads, N, 4)
        for e in range(16):
            ps = ps + lane[..., e]
        l = l * alpha.unsqueeze(-1) + ps
        m = mn
        pb16 = stored(p, BF16)
        o = o * alpha.unsqueeze(-1)
        for key in range(64):
            o = _fma(pb16[..., key:key + 1], vp[:, :, b * 64 + key].unsqueeze(2), o)
    lt = (l[..., 0] + l[..., 1]) + (l[..., 2] + l[..., 3])
    os_ = o * (1.0 / lt).unsqueeze(-1)
    return _emu_pe(os_, qkv, h, w, heads, pw, pb, out_dtype, mutant)


# =====================================================================================================================
# 1. the references against nested loops and hand-worked values
# =====================================================================================================================
def test_dw_ref_against_loops_and_by_hand():
    for stride in (1, 2):
        x, w9c, b = Y.dw_family("uniform", 2, 3, 4, 5, F32, 1)
        v, S, ref = Y.dw_ref(x, w9c, b, stride, ACT_SILU)
        oh, ow = Y.dw_out_hw(4, 5, stride)
        assert v.shape == (2, 3, oh, ow)
        for n in range(2):
            for c in range(3):
                for oy in range(oh):
                    for ox in range(ow):
                        acc, sab = float(b[c]), abs(float(b[c]))
                        for ky in range(3):
                            for kx in range(3):
                                iy, ix = oy * stride - 1 + ky, ox * stride - 1 + kx
                                if 0 <= iy < 4 and 0 <= ix < 5:
                                    t = float(x[n, c, iy, ix]) * float(w9c[ky * 3 + kx, c])
                                    acc, sab = acc + t, sab + abs(t)
                        assert abs(float(v[n, c, oy, ox]) - acc) < 1e-12 and abs(float(S[n, c, oy, ox]) - sab) < 1e-12
                        assert abs(float(ref[n, c, oy, ox]) - acc / (1 + math.exp(-acc))) < 1e-12
    # a unit impulse at the centre of a 3 x 3 map reads the weights back mirrored: out[oy, ox] = w[tap (2 - oy, 2 - ox)]
    x = torch.zeros(1, 1, 3, 3)
    x[0, 0, 1, 1] = 1.0
    w9c = torch.arange(1.0, 10.0).view(9, 1)
    v, _, _ = Y.dw_ref(x, w9c, torch.tensor([0.5]), 1, ACT_NONE)
    assert torch.equal(v[0, 0], torch.tensor([[9.5, 8.5, 7.5], [6.5, 5.5, 4.5], [3.5, 2.5, 1.5]], dtype=F64))
    v2, _, _ = Y.dw_ref(x, w9c, torch.tensor([0.5]), 2, ACT_NONE)  # outputs (0, 0), (0, 1), (1, 0), (1, 1) read rows / columns -1 .. 1 and 1 .. 3
    assert torch.equal(v2[0, 0], torch.tensor([[9.5, 7.5], [3.5, 1.5]], dtype=F64))


def test_convt_ref_against_loops_and_by_hand():
    x, w, b = Y.convt_family("uniform", 2, 3, 2, 3, 2, F32, 2)
    v, S, ref = Y.convt_ref(x, w, b)
    assert v.shape == (2, 2, 4, 6) and torch.equal(v, ref)
    for n in range(2):
        for co in range(2):
            for y in range(2):
                for xx in range(3):
                    for i in range(2):
                        for j in range(2):
                            acc = float(b[co]) + sum(float(x[n, ci, y, xx]) * float(w[ci, co, i, j]) for ci in range(3))
                            sab = abs(float(b[co])) + sum(abs(float(x[n, ci, y, xx]) * float(w[ci, co, i, j])) for ci in range(3))
                            assert abs(float(v[n, co, 2 * y + i, 2 * xx + j]) - acc) < 1e-12
                            assert abs(float(S[n, co, 2 * y + i, 2 * xx + j]) - sab) < 1e-12
    x = torch.zeros(1, 1, 2, 2)
    x[0, 0, 1, 0] = 2.0
    w = torch.tensor([1.0, 2.0, 3.0, 4.0]).view(1, 1, 2, 2)
    v, _, _ = Y.convt_ref(x, w, torch.tensor([0.25]))
    want = torch.full((4, 4), 0.25, dtype=F64)
    want[2:, :2] = torch.tensor([[2.25, 4.25], [6.25, 8.25]], dtype=F64)  # pixel (1, 0) -> rows 2 .. 3, columns 0 .. 1, tap 2 i + j
    assert torch.equal(v[0, 0], want)


def test_psa_ref_against_loops_and_by_hand():
    n, h, w, heads = 2, 2, 3, 2
    qkv, pw, pb = Y.psa_family("uniform", n, h, w, heads, F32, 3)
    r = Y.psa_ref(qkv, h, w, heads, Y.SCALE, pw, pb)
    sc, N = Y.f32_scale(Y.SCALE), h * w
    x = qkv.double().reshape(n, N, heads * Y.CH)
    for b in range(n):
        for hh in range(heads):
            c0 = hh * Y.CH
            for p in range(N):
                lg = [sc * sum(float(x[b, p, c0 + i]) * float(x[b, q_, c0 + 32 + i]) for i in range(32)) for q_ in range(N)]
                ab = [sc * sum(abs(float(x[b, p, c0 + i]) * float(x[b, q_, c0 + 32 + i])) for i in range(32)) for q_ in range(N)]
                mx = max(lg)
                ex = [math.exp(v_ - mx) for v_ in lg]
                den = sum(ex)
                py, px = p // w, p % w
                for j in (0, 17, 63):
                    c = hh * 64 + j
                    att = sum(ex[q_] / den * float(x[b, q_, c0 + 64 + j]) for q_ in range(N))
                    A = sum(ex[q_] / den * abs(float(x[b, q_, c0 + 64 + j])) for q_ in range(N))
                    pe, peS = float(pb[c]), abs(float(pb[c]))
                    for dy in (-1, 0, 1):
                        for dx in (-1, 0, 1):
                            iy, ix = py + dy, px + dx
                            if 0 <= iy < h and 0 <= ix < w:
                                t = float(pw[(dy + 1) * 3 + dx + 1, c]) * float(x[b, iy * w + ix, c0 + 64 + j])
                                pe, peS = pe + t, peS + abs(t)
                    assert abs(float(r["out"][b, py, px, c]) - (att + pe)) < 1e-12
                    assert abs(float(r["A"][b, py, px, c]) - A) < 1e-12 and abs(float(r["peS"][b, py, px, c]) - peS) < 1e-12
                    assert abs(float(r["Sqk"][b, py, px, c]) - max(ab)) < 1e-12
    # by hand, scale 1: one token -> out = v (1 + w[centre]) + b; two tokens with logits (0, x) for query 0 -> weights 1 / (1 + e^x), ...
    qkv = torch.zeros(1, 1, 1, Y.CH)
    qkv[..., 64:] = 2.0
    pw, pb = torch.zeros(9, 64), torch.full((64,), 0.5)
    pw[4] = 0.25
    assert torch.equal(Y.psa_ref(qkv, 1, 1, 1, 1.0, pw, pb)["out"], torch.full((1, 1, 1, 64), 3.0, dtype=F64))
    qkv = torch.zeros(1, 1, 2, Y.CH)
    qkv[0, 0, 0, 0], qkv[0, 0, 1, 32] = 1.0, 1.5   # q of token 0, k of token 1: logits of query 0 are (0, 1.5), of query 1 (0, 0)
    qkv[0, 0, 0, 64:], qkv[0, 0, 1, 64:] = 1.0, 5.0
    out = Y.psa_ref(qkv, 1, 2, 1, 1.0, torch.zeros(9, 64), torch.zeros(64))["out"]
    w1 = math.exp(1.5) / (1 + math.exp(1.5))
    assert abs(float(out[0, 0, 0, 7]) - (1 - w1 + 5 * w1)) < 1e-14 and abs(float(out[0, 0, 1, 7]) - 3.0) < 1e-14


def test_convt_packer_layout_zero_fill_and_rounding():
    """`upa_pack_conv_transpose2x2_weight` is host code: row q = tap * cout + co, kp = cin rounded up to the MFMA depth with zeros, bf16
    rounded to nearest even (ties included) - compared in every bit with convt_pack_ref on weights that are NOT bf16 numbers."""
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    for cin, cout in ((5, 3), (40, 6), (72, 24)):
        g = torch.Generator().manual_seed(cin)
        w = (torch.rand(cin, cout, 2, 2, generator=g) * 2 - 1).contiguous()
        w.view(-1)[:4] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20])  # ties and one just above
        for dtype, code, kb in ((F32, L.UPA_F32, 4), (BF16, L.UPA_BF16, 32)):
            kp, es = -(-cin // kb) * kb, 4 if dtype == F32 else 2
            nbytes = lib.upa_conv_transpose2x2_packed_weight_bytes(cin, cout, code)
            assert nbytes == 4 * cout * kp * es
            host = torch.full((nbytes,), 0xAB, dtype=torch.uint8)
            L.check(lib.upa_pack_conv_transpose2x2_weight(w.data_ptr(), cin, cout, code, host.data_ptr()))
            got = host.view(dtype).reshape(4 * cout, kp)
            want = Y.convt_pack_ref(w, dtype).to(dtype)
            assert torch.equal(got.view(torch.int32 if dtype == F32 else torch.int16), want.view(torch.int32 if dtype == F32 else torch.int16))
            assert bool((got[:, cin:] == 0).all())
            tap, co, ci = 2, cout - 1, cin - 1
            assert float(got[tap * cout + co, ci]) == float(stored(w, dtype)[ci, co, 1, 0])
    assert float(stored(torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8]), BF16)[0]) == 1.0  # the tie goes to the even neighbour


# =====================================================================================================================
# 2. the emulations lie inside the bounds at every shape of the GPU tests
# =====================================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_dw_emulation_inside_bound(dtype):
    worst = (0.0, "")
    for stride in (1, 2):
        for act in (ACT_NONE, ACT_SILU):
            for fi, family in enumerate(Y.DW_FAMILIES):
                for (h, w) in Y.DW_MAPS:
                    for c in Y.DW_CHANNELS:
                        x, w9c, b = Y.dw_family(family, 2, c, h, w, dtype, 10 * c + fi)
                        v, S, ref = Y.dw_ref(x, w9c, b, stride, act)
                        y = emu_dw(x, w9c, b, stride, act, dtype)
                        worst = max(worst, (_worst(y, ref, Y.dw_bound(v, S, ref, act, dtype)), f"{family} {h}x{w} c{c} s{stride} act{act}"))
    print(f"dwconv emulation {dtype}: worst error / bound = {worst[0]:.3f} ({worst[1]})")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_convt_emulation_inside_bound(dtype):
    worst = (0.0, "")
    cins, couts = Y.CONVT_CH[dtype]
    for fi, family in enumerate(Y.CONVT_FAMILIES):
        for (h, w) in Y.CONVT_MAPS:
            for cin in cins:
                for cout in couts:
                    x, wt, b = Y.convt_family(family, 2, cin, h, w, cout, dtype, cin + cout + fi)
                    v, S, ref = Y.convt_ref(x, wt, b)
                    y = emu_convt(x, wt, b, dtype)
                    worst = max(worst, (_worst(y, ref, Y.convt_bound(v, S, ref, cin, dtype)), f"{family} {h}x{w} {cin}->{cout}"))
    print(f"convt emulation {dtype}: worst error / bound = {worst[0]:.3f} ({worst[1]})")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("hw", Y.PSA_MAPS, ids=[f"{h}x{w}" for h, w in Y.PSA_MAPS])
def test_psa_emulations_inside_bound(hw):
    h, w = hw
    N = h * w
    worst = {"scalar f32": (0.0, ""), "scalar bf16": (0.0, ""), "mfma": (0.0, "")}
    for heads in Y.PSA_HEADS:
        for fi, family in enumerate(Y.PSA_FAMILIES):
            for dtype in (F32, BF16):
                qkv, pw, pb = Y.psa_family(family, 2, h, w, heads, dtype, 100 * heads + fi)
                r = Y.psa_ref(qkv, h, w, heads, Y.SCALE, pw, pb)
                name = "scalar f32" if dtype == F32 else "scalar bf16"
                y = emu_psa_scalar(qkv, h, w, heads, Y.SCALE, pw, pb, dtype)
                worst[name] = max(worst[name], (_worst(y, r["out"], Y.psa_bound("scalar", r, N, dtype)), f"{family} heads {heads}"))
                if dtype == BF16:
                    y = emu_psa_mfma(qkv, h, w, heads, Y.SCALE, pw, pb, dtype)
                    worst["mfma"] = max(worst["mfma"], (_worst(y, r["out"], Y.psa_bound("mfma", r, N, dtype)), f"{family} heads {heads}"))
    for name, (ratio, what) in worst.items():
        print(f"psa emulation {name} N={N}: worst error / bound = {ratio:.3f} ({what})")
        assert ratio <= 1.0, (name, ratio, what)


# =====================================================================================================================
# 3. every mutant leaves the bound on the family built to catch it
# =====================================================================================================================
def _psa_mutant_escapes(emu, kind, mutant, family, h, w, heads, dtype):
    qkv, pw, pb = Y.psa_family(family, 2, h, w, heads, dtype, 7)
    r = Y.psa_ref(qkv, h, w, heads, Y.SCALE, pw, pb)
    bound = Y.psa_bound(kind, r, h * w, dtype)
    good = _worst(emu(qkv, h, w, heads, Y.SCALE, pw, pb, dtype), r["out"], bound)
    bad = _worst(emu(qkv, h, w, heads, Y.SCALE, pw, pb, dtype, mutant), r["out"], bound)
    print(f"psa {kind} {dtype} mutant {mutant} on {family} {h}x{w} heads {heads}: {bad:.3g} (unmutated {good:.3f})")
    assert good <= 1.0
    return bad > 1.0


PSA_MUTANTS = [  # mutant, family, (h, w), heads
    ("swap_qk", "uniform", (3, 5), 1),
    ("no_scale", "uniform", (3, 5), 1),
    ("no_scale", "large", (4, 4), 1),
    ("unmasked", "negative", (1, 17), 1),
    ("unmasked", "negative", (5, 13), 2),
    ("no_alpha", "rising", (4, 8), 1),
    ("no_alpha", "rising", (5, 13), 1),
    ("merge_skip", "uniform", (5, 13), 1),
    ("merge_skip", "tail", (3, 43), 1),
    ("neighbour_v", "uniform", (3, 5), 2),
    ("neighbour_v", "impulse_v", (3, 5), 3),
    ("pe_transposed", "impulse_v", (3, 5), 1),
    ("pe_no_border", "impulse_v", (3, 5), 2),
    ("drop_channel", "uniform", (4, 4), 1),
]


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", PSA_MUTANTS, ids=[f"{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}-h{c[3]}" for c in PSA_MUTANTS])
def test_psa_scalar_mutants_leave_the_bound(case, dtype):
    mutant, family, (h, w), heads = case
    assert _psa_mutant_escapes(emu_psa_scalar, "scalar", mutant, family, h, w, heads, dtype)


MFMA_MUTANTS = [("unmasked", "negative", (1, 17), 1), ("unmasked", "negative", (5, 13), 2), ("no_alpha", "rising", (5, 13), 1),
                ("no_alpha", "rising", (3, 43), 2), ("pe_transposed", "impulse_v", (3, 5), 1), ("pe_no_border", "impulse_v", (3, 5), 2)]


@pytest.mark.parametrize("case", MFMA_MUTANTS, ids=[f"{c[0]}-{c[1]}-{c[2][0]}x{c[2][1]}-h{c[3]}" for c in MFMA_MUTANTS])
def test_psa_mfma_mutants_leave_the_bound(case):
    mutant, family, (h, w), heads = case
    assert _psa_mutant_escapes(emu_psa_mfma, "mfma", mutant, family, h, w, heads, BF16)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_dw_and_convt_mutants_leave_the_bound(dtype):
    for mutant, family, stride in (("row_start", "impulse", 2), ("row_start", "uniform", 2), ("drop_channel", "uniform", 1),
                                   ("drop_channel", "impulse", 2)):
        x, w9c, b = Y.dw_family(family, 2, 6, 5, 4, dtype, 5)
        v, S, ref = Y.dw_ref(x, w9c, b, stride, ACT_SILU)
        bound = Y.dw_bound(v, S, ref, ACT_SILU, dtype)
        assert _worst(emu_dw(x, w9c, b, stride, ACT_SILU, dtype), ref, bound) <= 1.0
        assert _worst(emu_dw(x, w9c, b, stride, ACT_SILU, dtype, mutant), ref, bound) > 1.0, (mutant, family)
    cin = Y.CONVT_CH[dtype][0][1]
    for mutant, family in (("swap_taps", "impulse"), ("swap_taps", "uniform"), ("drop_channel", "uniform"), ("drop_channel", "impulse")):
        x, wt, b = Y.convt_family(family, 2, cin, 7, 9, 8, dtype, 6)
        v, S, ref = Y.convt_ref(x, wt, b)
        bound = Y.convt_bound(v, S, ref, cin, dtype)
        assert _worst(emu_convt(x, wt, b, dtype), ref, bound) <= 1.0
        assert _worst(emu_convt(x, wt, b, dtype, mutant), ref, bound) > 1.0, (mutant, family)


# =====================================================================================================================
# 4. the families' stated conditions, on the reference alone
# =====================================================================================================================
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_psa_family_conditions(dtype):
    for (h, w) in Y.PSA_MAPS:
        N = h * w
        for heads in Y.PSA_HEADS:
            def ref(family):
                qkv, pw, pb = Y.psa_family(family, 2, h, w, heads, dtype, 100 * heads)
                assert torch.equal(stored(qkv, dtype), qkv), "values not representable"
                return Y.psa_ref(qkv, h, w, heads, Y.SCALE, pw, pb), qkv
            r, _ = ref("uniform")
            if N >= 64:
                med = float(r["attn"].max(-1).values.median())
                assert 5.0 / N < med < 0.5, (N, heads, med)
            if N >= 2:
                d = ref("rising")[0]["logits"].diff(dim=-1)
                assert float(d.min()) > 0.4, (N, float(d.min()))       # strictly increasing: every key raises the running maximum
                d = ref("falling")[0]["logits"].diff(dim=-1)
                assert float(d.max()) < -0.4
                lg = ref("large")[0]["logits"]
                assert float(lg.max(-1).values.min()) > 55 and float(lg.min(-1).values.max()) < -55
            r, _ = ref("negative")
            assert float(r["logits"].max()) < -10 and float(r["A"].min()) > 2.7  # v > 0: A is the attention part itself
            r, _ = ref("tail")
            if N >= 2:
                assert float(r["attn"][..., N - 1].min()) > 0.5
            r, qkv = ref("impulse_v")
            v = Y.psa_split(qkv, heads)[2]
            assert int((v.abs().sum(-1) > 0).sum()) == 2 * heads      # one pixel per (image, head)
            if N >= 16:
                assert float(r["attn"].max()) < 2.0 / N               # near-flat attention


def test_dw_vector_width_restates_the_dispatch():
    assert [Y.dw_vector_width(c, F32) for c in Y.DW_CHANNELS] == [4, 1, 4, 4, 4]
    assert [Y.dw_vector_width(c, BF16) for c in Y.DW_CHANNELS] == [1, 1, 8, 1, 8]
    assert Y.dw_vector_width(8, F32, 1) == 1 and Y.dw_vector_width(8, BF16, 1) == 1
