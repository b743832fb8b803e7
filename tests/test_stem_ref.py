"""Pins tests/stem_ref.py (the float64 reference of the first-layer kernels, csrc/stem.hip) on the CPU: against a loop-written convolution
and hand-worked border pixels of the k = 6, pad = 2, stride 2 stem, an f32 emulation of the kernels' arithmetic in four summation orders,
the uint8 table's distance from every bf16 rounding boundary, the conditions that make the GPU comparison worth its name on every fused
case, the case lists' own promises (every instantiation met, seams crossed, several tiles per workgroup where a case says so), and
negative controls that each fail the comparison they target."""

import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import block_ref as B
from tests import stem_ref as S
from tests.conv_ref import ACT_NONE, ACT_SILU, F64

BF16 = torch.bfloat16


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _loops(x, wt, bias, k, stride, pad, act):
    """The seven-loop convolution (n, co, oy, ox, ci, ky, kx) in Python floats."""
    n, cin, h, w = x.shape
    cout = wt.shape[0]
    oh, ow = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    out = torch.zeros(n, cout, oh, ow, dtype=F64)
    for i in range(n):
        for co in range(cout):
            for oy in range(oh):
                for ox in range(ow):
                    v = float(bias[co])
                    for ci in range(cin):
                        for ky in range(k):
                            for kx in range(k):
                                iy, ix = oy * stride + ky - pad, ox * stride + kx - pad
                                if 0 <= iy < h and 0 <= ix < w:
                                    v += float(x[i, ci, iy, ix]) * float(wt[co, ci, ky, kx])
                    out[i, co, oy, ox] = v / (1 + math.exp(-v)) if act == ACT_SILU else v
    return out


def test_single_stem_against_seven_loops():
    g = _g(1)
    for (cin, cout, k, s, pad, h, w, act) in ((3, 4, 6, 2, 2, 7, 9, ACT_SILU), (3, 4, 3, 2, 1, 5, 6, ACT_NONE), (1, 4, 5, 1, 2, 4, 5, ACT_SILU), (3, 4, 3, 1, 0, 5, 5, ACT_SILU)):
        x = torch.rand(2, cin, h, w, generator=g) * 2 - 1
        wt = torch.rand(cout, cin, k, k, generator=g) * 2 - 1
        bias = torch.rand(cout, generator=g) - 0.5
        for mfma in (False, True):
            ref, bound = S.stem_single(x, wt, bias, k, s, pad, act, torch.float32, mfma)
            xs, ws = (B.rn_bf16(x.double()), B.rn_bf16(wt.double())) if mfma else (x.double(), wt.double())
            want = _loops(xs, ws, bias, k, s, pad, act)
            assert ref.shape == want.shape
            assert float((ref - want).abs().max()) <= 1e-13
            assert bool((bound > 0).all()) and float(bound.max()) < 1e-3  # f32 rounding of K + 1 <= 109 terms: no term tied to the largest output
        if not (cin == 3 and k in (3, 6)):
            continue
        # the MFMA family's rounding of its operands is a real change of the problem, far outside the f32 bound of the unrounded one
        r0, b0 = S.stem_single(x, wt, bias, k, s, pad, act, torch.float32, False)
        r1, _ = S.stem_single(x, wt, bias, k, s, pad, act, torch.float32, True)
        assert bool(((r0 - r1).abs() > b0).any())


def test_hand_worked_border_pixels_of_the_k6_pad2_stride2_stem():
    ones = torch.ones(1, 1, 8, 8)
    ref, _ = S.stem_single(ones, torch.ones(1, 1, 6, 6), torch.zeros(1), 6, 2, 2, ACT_NONE, torch.float32, False)
    # output (oy, ox) covers input rows 2 oy - 2 .. 2 oy + 3: four of the six rows at either border, all six inside
    assert ref[0, 0].tolist() == [[16, 24, 24, 16], [24, 36, 36, 24], [24, 36, 36, 24], [16, 24, 24, 16]]
    ramp = torch.arange(64, dtype=torch.float32).view(1, 1, 8, 8)
    first = torch.zeros(1, 1, 6, 6)
    first[0, 0, 0, 0] = 1.0   # tap (0, 0) alone: out(oy, ox) = x[2 oy - 2, 2 ox - 2], zero in the first row and column (padding)
    ref, _ = S.stem_single(ramp, first, torch.zeros(1), 6, 2, 2, ACT_NONE, torch.float32, False)
    assert ref[0, 0].tolist() == [[0, 0, 0, 0], [0, 0, 2, 4], [0, 16, 18, 20], [0, 32, 34, 36]]
    last = torch.zeros(1, 1, 6, 6)
    last[0, 0, 5, 5] = 1.0    # tap (5, 5) alone: out(oy, ox) = x[2 oy + 3, 2 ox + 3], zero in the last row and column
    ref, _ = S.stem_single(ramp, last, torch.zeros(1), 6, 2, 2, ACT_NONE, torch.float32, False)
    assert ref[0, 0].tolist() == [[27, 29, 31, 0], [43, 45, 47, 0], [59, 61, 63, 0], [0, 0, 0, 0]]
    # the same through `stage` with its new pad argument (default k // 2 = 3 would give another map)
    t, e = B.stage(ramp, None, last, torch.zeros(1), 6, 2, ACT_NONE, pad=2)
    assert t[0, 0].tolist() == [[27, 29, 31, 0], [43, 45, 47, 0], [59, 61, 63, 0], [0, 0, 0, 0]] and float(e.max()) == 0.0
    assert tuple(B.stage(ramp, None, last, torch.zeros(1), 6, 2, ACT_NONE)[0].shape) == (1, 1, 5, 5)


def test_fused_pair_and_pool_against_loops():
    g = _g(2)
    x = B.family_input("positive", g, 2, 3, 8, 12)
    for k0, s0, p0 in ((3, 2, 1), (6, 2, 2), (3, 1, 1)):
        w0, b0 = B.family_conv("positive", g, 4, 3, k0)
        w1, b1 = B.family_conv("positive", g, 8, 4, 3)
        trace = []
        out, e = S.fused_pair(x, w0, b0, k0, s0, p0, w1, b1, trace=trace)
        t_want = B.rn_bf16(_loops(x.double(), w0.double(), b0, k0, s0, p0, ACT_SILU))
        t, et = trace[0]
        assert bool(((t - t_want).abs() <= et).all())
        o_want = B.rn_bf16(_loops(t, w1.double(), b1, 3, 2, 1, ACT_SILU))
        assert tuple(out.shape) == (2, 8, 8 // (2 * s0), 12 // (2 * s0))
        assert bool(((out - o_want).abs() <= e).all()) and bool((out[e == 0] == o_want[e == 0]).all())
    wt = torch.rand(4, 3, 3, 3, generator=g) * 2 - 1
    bias = torch.rand(4, generator=g) - 0.5
    xs = torch.rand(2, 3, 6, 8, generator=g) * 2 - 1
    for pad in (0, 1):
        p, ep = S.stem_pool(xs, wt, bias, pad)
        full = B.rn_bf16(_loops(B.rn_bf16(xs.double()), B.rn_bf16(wt.double()), bias, 3, 1, pad, ACT_SILU))
        want = torch.stack([full[:, :, i::2, j::2] for i in (0, 1) for j in (0, 1)]).amax(0)
        assert p.shape == want.shape and bool(((p - want).abs() <= ep).all())


# ---------------------------------------------------------------------------------------------------------------------
# f32 emulation of the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------
ORDERS = ("k32", "k16_lines", "chain", "perm")


def _order(name, cin, k, g):
    """Groups of K-indices (ci * k * k + tap, F.unfold's order); a group is summed on its own, then added to the accumulator (an MFMA k-step).
    k32: the (tap, ci) im2col row in 32-deep k-steps, bias first (stem_mfma_kernel, stage 3 of the fused kernels).  k16_lines: one patch line
    (ci, kh) per group (the 16-deep gather forms).  chain: the scalar kernel's (kh, kw, ci) chain from the bias.  perm: any order."""
    kk = k * k
    flat = [ci * kk + tap for tap in range(kk) for ci in range(cin)]
    if name == "k32":
        return [flat[i:i + 32] for i in range(0, len(flat), 32)], True
    if name == "k16_lines":
        return [[ci * kk + kh * k + kw for kw in range(k)] for ci in range(cin) for kh in range(k)], True
    if name == "chain":
        return [[i] for i in flat], True
    return [[int(i)] for i in torch.randperm(cin * kk, generator=g)], False


@pytest.mark.parametrize("form", ["k3s2c16", "k6s2c16", "k3s1c32", "pool_p1", "pool_p0", "single_f32", "single_bf16"])
def test_f32_emulation_in_four_orders_stays_inside_the_bound(form):
    g = _g(5)
    x = B.family_input("positive", g, 2, 3, 16, 24)
    if form.startswith("k"):
        k0, s0, c0 = int(form[1]), int(form[3]), int(form[5:])
        w0, b0 = B.family_conv("positive", g, c0, 3, k0)
        w1, b1 = B.family_conv("positive", g, 2 * c0, c0, 3)

        def run(fn):
            return S.fused_pair(x, w0, b0, k0, s0, 1 if k0 == 3 else 2, w1, b1, fn)
    elif form.startswith("pool"):
        wt, bias = B.family_conv("positive", g, 16, 3, 3)

        def run(fn):
            if fn is B.stage:
                return S.stem_pool(x, wt, bias, int(form[-1]))
            return F.max_pool2d(fn(x, None, wt, bias, 3, 1, ACT_SILU, pad=int(form[-1]))[0], 2, 2), None
    else:
        xs = B._bf(torch.rand(2, 3, 16, 24, generator=g) * 2 - 1)
        wt, bias = B._bf(torch.rand(16, 3, 6, 6, generator=g) * 2 - 1), torch.rand(16, generator=g) - 0.5
        odt = torch.float32 if form == "single_f32" else BF16

        def run(fn):
            if fn is B.stage:
                return S.stem_single(xs, wt, bias, 6, 2, 2, ACT_SILU, odt, True)
            return fn(xs, None, wt, bias, 6, 2, ACT_SILU, out_dtype=odt, pad=2)
    with torch.no_grad():
        ref, e = run(B.stage)
        pre = {o: [] for o in ORDERS}
        outs = {o: run(B.emu_stage(_order, o, pre[o]))[0] for o in ORDERS}
    for o, y in outs.items():
        d = (y - ref).abs()
        assert bool((d <= e).all()), (form, o, float((d - e).max()))
        if form[0] in "kp":
            assert bool((d[e == 0] == 0).all()), (form, o)
    differ = sum(int(not torch.equal(pre[a][0], pre[b][0])) for a in ORDERS for b in ORDERS if a < b)
    assert differ >= 2, "the summation orders gave the same f32 bits: the emulation proves nothing"


# ---------------------------------------------------------------------------------------------------------------------
# the uint8 table
# ---------------------------------------------------------------------------------------------------------------------
def test_u8_table_is_far_from_every_bf16_rounding_boundary():
    """The staged bf16 of float32(b) / 255 must not depend on the last bit of the device's division: every entry lies at least 64 f32 ulps
    from the midpoint of two bf16 numbers (the low 16 bits of its f32 pattern, as a distance from 0x8000).  The minimum is 129, at b = 1."""
    tab = (np.arange(256, dtype=np.float32) / np.float32(255))
    assert tab[0] == 0.0 and tab[255] == 1.0 and tab[51] == np.float32(0.2)
    low = (tab.view(np.uint32) & 0xFFFF).astype(np.int64)
    dist = np.abs(low - 0x8000)[1:]
    print("u8 table: minimum distance", int(dist.min()), "f32 ulps at b =", int(dist.argmin()) + 1)
    assert int(dist.min()) >= 64
    assert (int(dist.min()), int(dist.argmin()) + 1) == (129, 1)
    # hence the same bf16 for the neighbouring f32 numbers on either side, and the table of the reference is what any such division stages
    t64 = torch.from_numpy(tab.astype(np.float64))
    for step in (-1, 1):
        nb = torch.from_numpy((tab.view(np.int32) + step).view(np.float32)[1:].astype(np.float64))
        assert torch.equal(B.rn_bf16(nb), B.rn_bf16(t64[1:]))
    assert torch.equal(S.u8_table(), t64)
    fr = torch.tensor([[[[0, 51, 255]]]], dtype=torch.uint8)     # B = 0, G = 51, R = 255 -> channels (R, G, B)
    assert S.u8_to_nchw(fr, False).flatten().tolist() == [1.0, float(np.float32(0.2)), 0.0]
    assert S.u8_to_nchw(fr, True).flatten().tolist() == [1.0, float(torch.tensor(0.2).to(BF16)), 0.0]


# ---------------------------------------------------------------------------------------------------------------------
# conditions on the GPU cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(S.FUSED_CASES)), ids=[c["id"] for c in S.FUSED_CASES])
def test_fused_cases_are_decidable_on_positive(ci):
    """Computed by the reference alone: at least 90 % of a fused case's outputs on `positive` have bound 0 (the kernel must give the
    reference's bits there) and no bound exceeds one bf16 ulp.  block_ref's scales (inputs in [0, 1.5], weights in [0, 3 / K]) give 0.985
    to 0.993 on 3 -> 16 -> 32 and 3 -> 32 -> 64; no scale had to be changed."""
    case = S.FUSED_CASES[ci]
    if "positive" not in case["families"]:
        pytest.fail("every fused case runs on `positive`")
    _, (out, e) = S.fused_case_reference(ci, "positive")
    share = float((e == 0).double().mean())
    assert share >= 0.9, share
    assert bool((e <= B.ulp_bf16(out)).all()), float((e / B.ulp_bf16(out)).max())
    assert float(out.min()) >= 0.0 and 0.1 < float(out.max()) < 64.0
    assert tuple(out.shape) == (case["n"], 2 * case["c0"], case["oh"], case["ow"])


def test_case_lists_keep_their_promises():
    every = S.SINGLE_CASES + S.POOL_CASES + S.FUSED_CASES
    met = {S.instantiation(c["expect"]) for c in every}
    assert met == set(S.INSTANTIATIONS), (set(S.INSTANTIATIONS) - met, met - set(S.INSTANTIATIONS))
    assert len(S.INSTANTIATIONS) == len(set(S.INSTANTIATIONS)) == 4 + 18 + 9 + 5
    assert len({c["id"] for c in every}) == len(every)
    for c in every:
        assert c["n"] >= 2, c["id"]
        if c["walk"]:
            assert c["expect"]["wgs"] < c["tiles"], c["id"]   # a workgroup walks several tiles
        else:
            gy = -(-c["cout"] // 16) if c["expect"]["family"] == S.SCALAR else 1   # the scalar kernel: one workgroup per tile and 16 channels
            assert c["expect"]["wgs"] == c["tiles"] * gy, c["id"]
    for c in S.SINGLE_CASES + S.POOL_CASES:
        e = c["expect"]
        tw = 64 if e["family"] != S.SCALAR or c["ow"] >= 64 else (32 if c["ow"] >= 32 else 16)
        th = 8 if e["family"] != S.SCALAR else 256 // tw
        assert c["ow"] > tw and c["oh"] > th and (c["ow"] % tw or c["oh"] % th), c["id"]   # two tiles each way, a partial one
    for c in S.FUSED_CASES:
        assert c["ow"] > 16 and c["oh"] > 8 and c["ow"] % 16 and c["oh"] % 8, c["id"]
    # stem_wgs 2 | 3 on 8 tiles of two images: 4 tiles per workgroup, or 3 | 3 | 2 - an even and an odd walk across the image boundary
    assert {c["opts"].get("stem_wgs", 0) for c in S.SINGLE_CASES if c["expect"]["family"] != S.SCALAR} >= {0, 2, 3, 8}
    assert {c["opts"].get("stemf_wgs", 0) for c in S.FUSED_CASES} >= {0, 2, 3, 4, 8}
    stag = {(c["expect"]["family"], c["expect"]["staging"]) for c in S.SINGLE_CASES}
    assert stag >= {(f, s) for f in (S.MFMA, S.MFMA_G16) for s in (S.DMA, S.VGPR, S.U8)} | {(S.SCALAR, S.VGPR), (S.SCALAR, S.U8)}
    # the interior tile of the larger fused shapes: the 17 x 33 stem tile of output tile (1, 1) inside the stem map
    for c in S.FUSED_CASES:
        if c["opts"].get("stemf_wgs") in (4, 8):
            assert 15 + 17 <= c["h"] // c["s0"] and 31 + 33 <= c["w"] // c["s0"], c["id"]


def test_impulse_family_lights_both_sides_of_every_tile_seam():
    case = S.FUSED_CASES[0]
    x = S.fused_data(case, "impulse")["x"]
    lit = [set(map(tuple, (x[i].abs().sum(0) > 0).nonzero().tolist())) for i in range(case["n"])]
    assert all(lit) and not (lit[0] & lit[1]) and not (lit[1] & lit[2]) and not (lit[0] & lit[2])
    every = set().union(*lit)
    assert case["seams_x"] == (64,) and case["seams_y"] == (32,)
    assert any(c == 63 for _, c in every) and any(c == 64 for _, c in every) and any(r == 31 for r, _ in every) and any(r == 32 for r, _ in every)


# ---------------------------------------------------------------------------------------------------------------------
# negative controls: each must exceed the bound or break bit-equality
# ---------------------------------------------------------------------------------------------------------------------
def _fails(got, ref, e):
    d = (got - ref).abs()
    return int(((d > e) | ((e == 0) & (d != 0))).sum())


def test_negative_control_one_tap_transposed():
    case = next(c for c in S.SINGLE_CASES if c["expect"]["family"] == S.MFMA and c["fmt"] == "bf16")
    d, (ref, bound) = S.single_case_reference("single", S.SINGLE_CASES.index(case))
    w = d["w"].clone()
    w[:, :, 0, 1], w[:, :, 1, 0] = d["w"][:, :, 1, 0], d["w"][:, :, 0, 1]
    bad, _ = S.single_reference(case, dict(d, w=w))
    assert _fails(bad, ref, bound) > ref.numel() // 2
    assert _fails(S.single_reference(case, d)[0], ref, bound) == 0


def test_negative_control_padding_value_not_zero():
    """The stem pixels outside the stem map hold SiLU(b0) (what the MFMA of an all-zero patch gives) instead of ZERO: only the border outputs
    of the second conv see it, as whole taps - on `impulse` and on `positive`."""
    ci = 0
    case = S.FUSED_CASES[ci]
    for fam in ("positive", "impulse"):
        d, (ref, e) = S.fused_case_reference(ci, fam)

        def wrong(x, e_in, w, bias, k, stride, act, **kw):
            if e_in is None:   # the stem stage: remember its bias
                wrong.b0 = bias.double()
                return B.stage(x, e_in, w, bias, k, stride, act, **kw)
            fill = (wrong.b0 / (1 + torch.exp(-wrong.b0))).view(1, -1, 1, 1)
            xp = B.rn_bf16(fill).expand(x.shape[0], -1, x.shape[2] + 2, x.shape[3] + 2).clone()
            xp[:, :, 1:-1, 1:-1] = x
            return B.stage(xp, F.pad(e_in, (1, 1, 1, 1)), w, bias, k, stride, act, pad=0)
        bad, _ = S.fused_reference(case, d, fam, stage_fn=wrong)
        assert bad.shape == ref.shape
        out = ((bad - ref).abs() > e) | ((e == 0) & (bad != ref))
        assert int(out.sum()) >= 8 and not bool(out[:, :, 1:, 1:].any()) and bool(out[:, :, 0].any()) and bool(out[:, :, :, 0].any()), fam


def test_negative_control_next_image_leaks_into_the_bottom_padding():
    case = next(c for c in S.SINGLE_CASES if c["expect"]["family"] == S.MFMA and c["fmt"] == "f32" and c["pad"] > 0 and (c["h"] + 2 * c["pad"] - c["k"]) % c["s"] == 0)
    d, (ref, bound) = S.single_case_reference("single", S.SINGLE_CASES.index(case))
    p, k, s = case["pad"], case["k"], case["s"]
    x = B.rn_bf16(d["x"].double())
    xp = F.pad(x, (p, p, p, p))
    xp[:-1, :, -p:, p:-p] = x[1:, :, :p, :]   # image i's bottom padding rows read image i + 1's first rows (the next rows in memory)
    bad, _ = S.stem_single(xp, d["w"], d["b"], k, s, 0, case["act"], BF16, True)
    assert bad.shape == ref.shape
    out = (bad - ref).abs() > bound
    # (the case's last output row reaches the bottom padding) only that row, and not the last image's, moves - by whole taps
    assert bool(out[:-1, :, -1].any()) and not bool(out[-1].any()) and not bool(out[:, :, :-1].any())


def test_negative_control_bgr_not_reversed():
    case = next(c for c in S.SINGLE_CASES if c["fmt"] == "u8")
    d, (ref, bound) = S.single_case_reference("single", S.SINGLE_CASES.index(case))
    mfma = case["expect"]["family"] != S.SCALAR
    bad, _ = S.stem_single(S.u8_to_nchw(d["x"], mfma, reverse=False), d["w"], d["b"], case["k"], case["s"], case["pad"], case["act"], BF16, mfma)
    assert _fails(bad, ref, bound) > ref.numel() // 2


def test_negative_control_pool_taken_before_the_activation_of_a_negative_pair():
    """The pool belongs behind SiLU and its bf16 rounding.  Taken on the f32 values behind SiLU but before the ROUNDING it gives the same bits -
    round-to-nearest is monotone, which is what the G16 pool form relies on, and what the first assertion states.  Taken before the
    ACTIVATION it does not: below its minimum at v = -1.278 SiLU falls as v rises, so of a pair of pre-activations there the larger one has the
    smaller activation, and the pooled value is wrong by far more than a bf16 ulp.  (The issue's wording, "before the bf16 rounding of a
    negative pair", names a control that cannot fail; this is the one that can.)"""
    v = torch.tensor([[[[-2.0, -6.0], [-3.0, -4.0]]]], dtype=F64)
    x = torch.zeros(1, 3, 2, 2, dtype=F64)
    x[0, 0] = v[0, 0]
    w = torch.zeros(1, 3, 3, 3)
    w[0, 0, 1, 1] = 1.0
    ref, e = S.stem_pool(x, w, torch.zeros(1), 1)
    act = v / (1 + torch.exp(-v))
    assert float(ref) == float(B.rn_bf16(act).max()) == float(B.rn_bf16(act.max().view(1))) and float(e) == 0.0   # -6 / (1 + e^6): the pair's largest
    before = B.rn_bf16((v.max() / (1 + torch.exp(-v.max()))).view(1))   # SiLU(-2) = -0.238: the smallest
    assert float(before) < float(ref) and abs(float(before) - float(ref)) > 16 * float(B.ulp_bf16(ref))
    # ... and on a whole case: wherever the four pre-activations of a window are negative enough, with the case's own bound
    case = next(c for c in S.POOL_CASES if c["fmt"] == "bf16")
    d, (pref, pe) = S.single_case_reference("pool", S.POOL_CASES.index(case))
    xs, ws = B.rn_bf16(d["x"].double()), B.rn_bf16(d["w"].double())
    pre = F.conv2d(xs, ws, d["b"].double(), stride=1, padding=case["pad"])
    vmax = F.max_pool2d(pre, 2, 2)
    bad = B.rn_bf16(vmax / (1 + torch.exp(-vmax)))
    assert _fails(bad, pref, pe) >= 8
