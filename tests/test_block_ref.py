"""Pins tests/block_ref.py (the float64 chain reference of the whole-block kernels and its decided rounding points) on the CPU: `stage`
against a loop-written convolution and hand-worked pixels, the bf16 store's bound against brute force, an f32 emulation of the kernels'
arithmetic in four summation orders on every chain, the conditions that make the GPU comparison worth its name on every GPU case, and two
negative controls that show the `impulse` inputs sit where a wrong halo column or a wrong padding value bites."""

import math

import pytest
import torch
import torch.nn.functional as F

from tests import block_ref as B
from tests.conv_ref import ACT_NONE, ACT_SILU, F64, U24

BF16 = torch.bfloat16


def _g(seed):
    return torch.Generator().manual_seed(seed)


def test_rn_bf16_is_round_to_nearest_even():
    a = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, -1.0 - 2.0 ** -8, 0.0, 255.5, 3.0e38], dtype=F64)
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -1.0, 0.0, 256.0, 3.0e38], dtype=F64)
    want[-1] = torch.tensor(3.0e38).to(BF16).double()
    assert torch.equal(B.rn_bf16(a), want)
    r = torch.rand(20000, generator=_g(1), dtype=F64) * 8 - 4
    r32 = r.float().double()  # where float32 represents the value, torch's own float32 -> bf16 rounding is the same single rounding
    assert torch.equal(B.rn_bf16(r32), r32.float().to(BF16).double())
    assert torch.equal(B.ulp_bf16(torch.tensor([1.0, 1.5, 2.0, 0.75], dtype=F64)), torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8], dtype=F64))


def test_stage_against_loops_and_hand_worked_pixels():
    g = _g(2)
    n, cin, cout, h, w = 2, 3, 4, 4, 5
    x = B.family_input("positive", g, n, cin, h, w)
    res = B.family_input("positive", g, n, cout, h, w)
    for k, stride in ((3, 1), (1, 1), (3, 2)):
        wt, bias = B.family_conv("positive", g, cout, cin, k)
        oh, ow = (h + stride - 1) // stride, (w + stride - 1) // stride
        r = res[:, :, :oh, :ow] if stride == 1 else None
        t, e = B.stage(x, None, wt, bias, k, stride, ACT_SILU, residual=r)
        assert tuple(t.shape) == (n, cout, oh, ow)
        p = k // 2
        for i in range(n):
            for co in range(cout):
                for oy in range(oh):
                    for ox in range(ow):
                        v = float(bias[co])
                        for ci in range(cin):
                            for ky in range(k):
                                for kx in range(k):
                                    iy, ix = oy * stride + ky - p, ox * stride + kx - p
                                    if 0 <= iy < h and 0 <= ix < w:
                                        v += float(x[i, ci, iy, ix]) * float(wt[co, ci, ky, kx])
                        a = v / (1 + math.exp(-v)) + (float(r[i, co, oy, ox]) if r is not None else 0.0)
                        want = float(B.rn_bf16(torch.tensor([a], dtype=F64)))
                        # the loop's own float64 order may sit on the other side of a tie only where the bound says so
                        assert abs(float(t[i, co, oy, ox]) - want) <= float(e[i, co, oy, ox]) + 0.0, (k, stride, i, co, oy, ox)
    # hand-worked: one input channel, one filter of ones, no bias, no activation: the corner sums 4 pixels, the centre 9
    x1 = torch.ones(1, 1, 3, 3)
    t, e = B.stage(x1, None, torch.ones(1, 1, 3, 3), torch.zeros(1), 3, 1, ACT_NONE)
    assert t[0, 0].tolist() == [[4, 6, 4], [6, 9, 6], [4, 6, 4]] and float(e.max()) == 0.0
    # 255 + 1: the float64 value 256 is a bf16 number, its neighbourhood of width (K + 1) 2^-24 S holds no boundary: decided
    t, e = B.stage(torch.full((1, 1, 1, 1), 255.0), None, torch.ones(1, 1, 1, 1), torch.ones(1), 1, 1, ACT_NONE)
    assert float(t) == 256.0 and float(e) == 0.0
    # 256 + 1 = 257 is a tie between 256 and 258: either may come out of the kernel, the bound is the whole ulp
    t, e = B.stage(torch.full((1, 1, 1, 1), 256.0), None, torch.ones(1, 1, 1, 1), torch.ones(1), 1, 1, ACT_NONE)
    assert float(t) == 256.0 and float(e) == 2.0
    # an input bound passes through |w| and, with a residual, adds e_res: f32 store keeps it as a number
    t, e = B.stage(torch.ones(1, 1, 1, 1), torch.full((1, 1, 1, 1), 0.5), torch.full((1, 1, 1, 1), 2.0), torch.zeros(1), 1, 1, ACT_NONE,
                   residual=torch.ones(1, 1, 1, 1), e_res=torch.full((1, 1, 1, 1), 0.25), out_dtype=torch.float32)
    assert float(t) == 3.0 and abs(float(e) - (1.0 + 0.25 + 1.01 * 2 * U24 * 2 + 2.0 ** -23 * 3 + 2.0 ** -23 * 3)) < 1e-12


def test_store_bound_against_brute_force():
    g = _g(3)
    a = (torch.rand(200, generator=g, dtype=F64) * 4 + 0.01) * torch.where(torch.rand(200, generator=g) < 0.2, -1.0, 1.0)
    e_pre = a.abs() * 2.0 ** -(6 + 8 * torch.rand(200, generator=g, dtype=F64))   # from several ulps down to far below one
    t, e_out = B.store_bf16(a, e_pre)
    u = torch.rand(200, 1000, generator=g, dtype=F64) * 2 - 1
    u[:, 0], u[:, 1] = -1.0, 1.0
    pts = B.rn_bf16(a[:, None] + u * e_pre[:, None])
    assert bool(((pts - t[:, None]).abs() <= e_out[:, None]).all())
    dec = e_out == 0
    assert bool((pts[dec] == t[dec][:, None]).all())
    assert 20 < int(dec.sum()) < 180, int(dec.sum())  # both kinds are present


# ---------------------------------------------------------------------------------------------------------------------
# f32 emulation of the kernels' arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def _order(name, cin, k, g):
    """Groups of K-indices (ci * k * k + tap, F.unfold's order): a group is summed on its own from zero, then added to the accumulator
    (an MFMA k-step); groups of one make a plain sequential sum.  Returns (groups, bias_first)."""
    kk = k * k
    if name in ("ch16", "ch32"):
        ch = 16 if name == "ch16" else 32
        return [[ci * kk + tap for ci in range(c0, min(c0 + ch, cin))] for tap in range(kk) for c0 in range(0, cin, ch)], name == "ch16"
    if name == "taps_outer":
        return [[ci * kk + tap] for tap in range(kk) for ci in range(cin)], False
    assert name == "perm"
    return [[int(i)] for i in torch.randperm(cin * kk, generator=g)], True


ORDERS = ("ch16", "ch32", "taps_outer", "perm")


def _small_chains():
    """Every chain of block_ref on a small instance: name -> (run(stage_fn) -> list of (value, bound or None))."""
    g = _g(5)
    x32 = B.family_input("positive", g, 2, 32, 5, 7)
    w_c2f = B.c2f_weights("positive", g, 32, 16, 32, 2)
    w_c2f1 = B.c2f_weights("positive", g, 32, 16, 32, 1)
    x16 = B.family_input("positive", g, 2, 16, 5, 6)
    w_down = B.c2f_weights("positive", g, 16, 8, 16, 1, down=24)
    w_pair = (B.family_conv("positive", g, 16, 16, 3), B.family_conv("positive", g, 16, 16, 3))
    fc = B.family_conv
    w_det = {"box": [fc("positive", g, 16, 16, 3), fc("positive", g, 16, 16, 3), fc("positive", g, 64, 16, 1, signed_tail=True)],
             "cls": [fc("positive", g, 24, 16, 3), fc("positive", g, 24, 24, 3), fc("positive", g, 20, 24, 1, signed_tail=True)]}

    def det(fn):
        bl, be, cl, ce, _ = B.detect_level(x16, w_det, fn)
        return [(bl, be), (cl, ce)]
    return {"c2f": lambda fn: [B.c2f(x32, w_c2f, 2, True, fn)], "c2f_noshortcut": lambda fn: [B.c2f(x32, w_c2f, 2, False, fn)],
            "c2f_down": lambda fn: [B.c2f_down(x16, w_down, fn)], "pair": lambda fn: [B.bottleneck_pair(x16.double(), None, w_pair, True, fn)],
            "pair_cv2": lambda fn: [B.c2f(x32, w_c2f1, 1, True, fn, skip_cv1=True)], "detect": det}


@pytest.mark.parametrize("chain", ["c2f", "c2f_noshortcut", "c2f_down", "pair", "pair_cv2", "detect"])
def test_f32_emulation_in_four_orders_stays_inside_the_bound(chain):
    run = _small_chains()[chain]
    with torch.no_grad():
        ref = run(B.stage)
        pre = {o: [] for o in ORDERS}
        outs = {o: run(B.emu_stage(_order, o, pre[o])) for o in ORDERS}
    for o, got in outs.items():
        for (t, e), (y, _) in zip(ref, got):
            d = (y - t).abs()
            assert bool((d <= e).all()), (chain, o, float((d - e).max()))
            assert bool((d[e == 0] == 0).all()), (chain, o)
    # the orders must really be different sums: their f32 values before the first store already differ (the stored bf16 bits of so small
    # an instance rarely do: an f32 rounding error reaches a bf16 boundary for about one element in 2^14)
    differ = sum(int(not torch.equal(pre[a][0], pre[b][0])) for a in ORDERS for b in ORDERS if a < b)
    assert differ >= 2, "the summation orders gave the same f32 bits: the emulation proves nothing"


# ---------------------------------------------------------------------------------------------------------------------
# conditions on every GPU case
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ci", range(len(B.CASES)), ids=[c["id"] for c in B.CASES])
def test_conditions_hold_on_every_gpu_case(ci):
    """Checked on the reference alone, `positive` family: at least 50 % of the block outputs (Detect: of the logits' inputs t2) have bound 0
    and no bf16 output has a bound above one ulp.  Caps with room (the decided share runs from 75 to 100 %), not measurements; where a case
    missed them the family's scale was changed (block_ref.family_conv, wscale), not the caps."""
    case = B.CASES[ci]
    d, ref = B.reference(ci, "positive")
    if case["form"] == "detect":
        e = torch.cat([q.flatten() for q in ref[4]])
        assert float((e == 0).float().mean()) >= 0.5
        assert bool(torch.isfinite(ref[1]).all()) and bool(torch.isfinite(ref[3]).all())
        sc = torch.sigmoid(ref[2])
        assert float(sc.min()) < 0.5 < float(sc.max())  # the signed tails put scores on both sides of 1 / 2
        return
    out, e = ref
    assert float((e == 0).float().mean()) >= 0.5, float((e == 0).float().mean())
    assert bool((e <= B.ulp_bf16(out)).all()), float((e / B.ulp_bf16(out)).max())
    assert float(out.min()) >= 0.0 and 0.1 < float(out.max()) < 64.0  # non-negative and O(1)


def test_impulse_family_lights_the_seams_and_differs_per_image():
    case = next(c for c in B.CASES if c["kernel"] == "c2f32 stream2" and c["w"] == 41)
    x = B.case_data(case, "impulse")["x"]
    lit = [set(map(tuple, (x[i].abs().sum(0) > 0).nonzero().tolist())) for i in range(case["n"])]
    assert all(lit) and not (lit[0] & lit[1]) and not (lit[1] & lit[2]) and not (lit[0] & lit[2])
    every = set().union(*lit)
    h, w = case["h"], case["w"]
    assert {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)} <= every
    for s in case["seams_x"]:
        assert any(c == s - 1 for _, c in every) and any(c == s for _, c in every)
    for s in case["seams_y"]:
        assert any(r == s - 1 for r, _ in every) and any(r == s for r, _ in every)


# ---------------------------------------------------------------------------------------------------------------------
# negative controls
# ---------------------------------------------------------------------------------------------------------------------
def _wrong_stage(kind, seam):
    """`stage` with one deliberately wrong thing in every 3x3 stage.  halo: output column seam - 1 reads its right-hand neighbour from
    column seam - 2 (the halo column taken from the wrong side of the seam).  padding: the pixels outside the image hold SiLU(bias of the
    producing stage) instead of 0."""
    state = {"bias": None}

    def run(x, e_in, w, bias, k, stride, act, residual=None, e_res=None, out_dtype=BF16):
        t, e = B.stage(x, e_in, w, bias, k, stride, act, residual, e_res, out_dtype)
        if k == 3 and kind == "halo":
            x2 = x.clone()
            x2[..., seam] = x[..., seam - 2]
            t2, _ = B.stage(x2, e_in, w, bias, k, stride, act, residual, e_res, out_dtype)
            t = t.clone()
            t[..., seam - 1] = t2[..., seam - 1]
        if k == 3 and kind == "padding" and state["bias"] is not None:
            pb = state["bias"][-x.shape[1]:].double()
            fill = (pb / (1 + torch.exp(-pb))).view(1, -1, 1, 1)
            xp = fill.expand(x.shape[0], -1, x.shape[2] + 2, x.shape[3] + 2).clone()
            xp[:, :, 1:-1, 1:-1] = x
            rp = None if residual is None else F.pad(residual, (1, 1, 1, 1))
            t = B.stage(xp, None, w, bias, k, stride, act, rp, None, out_dtype)[0][:, :, 1:-1, 1:-1]
        state["bias"] = bias
        return t, e
    return run


@pytest.mark.parametrize("kind", ["halo", "padding"])
def test_negative_control_falls_outside_the_bound_on_impulse(kind):
    g = _g(9)
    n, h, w, seam = 2, 6, 9, 4
    x = B.family_input("impulse", g, n, 16, h, w, seams_x=(seam,), seams_y=(4,))
    wts = B.c2f_weights("impulse", g, 16, 8, 16, 1)
    with torch.no_grad():
        ref, e = B.c2f(x, wts, 1, True)
        bad, _ = B.c2f(x, wts, 1, True, _wrong_stage(kind, seam))
        same, _ = B.c2f(x, wts, 1, True, _wrong_stage("none", seam))
    assert torch.equal(same, ref)
    out = (bad - ref).abs() > e
    assert int(out.sum()) >= 8, int(out.sum())  # whole taps: not one marginal element
    if kind == "halo":
        assert bool(out[..., seam - 2:seam + 1].any()) and not bool(out[..., seam + 2:].any())
    else:
        inner = out[:, :, 2:-2, 2:-2]
        assert not bool(inner.any()) and bool(out[:, :, 0].any()) and bool(out[:, :, :, 0].any())
