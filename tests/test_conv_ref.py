"""CPU: pins tests/conv_ref.py - the float64 reference and the per-element bound that tests/test_hip_conv_views.py holds every conv2d
dispatch path to - before any GPU is involved: against a seven-loop convolution written here, against hand-worked pixels, and against
a float32 emulation of the kernels' arithmetic, which must sit inside the bound and fall out of it when one input channel of one tap
is dropped."""

import math

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as CR

F64 = torch.float64


def _direct(x, w, bias, k, stride, pad):
    """y[n, co, oy, ox] = bias[co] + sum_{ci, kh, kw} x[n, ci, oy s + kh - p, ox s + kw - p] w[co, ci, kh, kw], zero outside the image."""
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    oh, ow = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    y = torch.zeros(n, cout, oh, ow, dtype=F64)
    for b in range(n):
        for co in range(cout):
            for oy in range(oh):
                for ox in range(ow):
                    acc = float(bias[co]) if bias is not None else 0.0
                    for ci in range(cin):
                        for kh in range(k):
                            for kw in range(k):
                                iy, ix = oy * stride + kh - pad, ox * stride + kw - pad
                                if 0 <= iy < h and 0 <= ix < wd:
                                    acc += float(x[b, ci, iy, ix]) * float(w[co, ci, kh, kw])
                    y[b, co, oy, ox] = acc
    return y


@pytest.mark.parametrize("k,stride,pad", [(1, 1, 0), (2, 1, 1), (3, 1, 1), (3, 2, 1), (4, 2, 1), (3, 1, 0), (3, 1, 2), (5, 1, 2), (7, 2, 3)],
                         ids=lambda v: str(v))
def test_conv_ref_matches_seven_loops(k, stride, pad):
    """v and S of conv_ref against the loops above on a 2 x 3 x 7 x 6 input (odd sizes, both borders inside every kernel's reach),
    cout 2; float64 on both sides, so only the summation order differs: 1e-13 of S."""
    g = torch.Generator().manual_seed(100 * k + 10 * stride + pad)
    x = torch.rand(2, 3, 7, 6, generator=g) * 2 - 1
    w = torch.rand(2, 3, k, k, generator=g) * 2 - 1
    b = torch.rand(2, generator=g) * 2 - 1
    res = torch.rand(2, 2, (7 + 2 * pad - k) // stride + 1, (6 + 2 * pad - k) // stride + 1, generator=g)
    v, S, ref = CR.conv_ref(x, w, b, res, k, stride, pad, CR.ACT_SILU)
    vd = _direct(x, w, b, k, stride, pad)
    Sd = _direct(x.abs(), w.abs(), b.abs(), k, stride, pad)
    assert v.dtype == F64 and S.dtype == F64 and ref.dtype == F64
    assert v.shape == vd.shape
    assert bool(((v - vd).abs() <= 1e-13 * Sd).all())
    assert bool(((S - Sd).abs() <= 1e-13 * Sd).all())
    assert bool((S >= v.abs() - 1e-13 * Sd).all())
    silu = vd / (1 + torch.exp(-vd))
    assert bool(((ref - (silu + res.double())).abs() <= 1e-13 * (1 + Sd)).all())
    v0, S0, ref0 = CR.conv_ref(x, w, None, None, k, stride, pad, CR.ACT_RELU)
    assert bool(((v0 - _direct(x, w, None, k, stride, pad)).abs() <= 1e-13 * Sd).all())
    assert bool(((S0 - (Sd - b.abs().double().view(1, 2, 1, 1))).abs() <= 1e-13 * Sd).all())
    assert torch.equal(ref0, v0.clamp_min(0))


def test_conv_ref_hand_worked_pixels():
    """One 1x1 pixel and one 3x3 corner pixel worked by hand.
    1x1: x = (2, -3), w = (0.5, 0.25), bias 1 -> v = 1 - 0.75 + 1 = 1.25, S = 1 + 0.75 + 1 = 2.75; ReLU + residual 0.5 -> 1.75.
    3x3, pad 1, 2 x 2 image x = [[1, 2], [3, 4]], w[kh][kw] = kh * 3 + kw + 1, bias -100: the top-left output sees x[0][0] under the centre tap
    (5), x[0][1] under tap (1, 2) = 6, x[1][0] under (2, 1) = 8, x[1][1] under (2, 2) = 9: v = 5 + 12 + 24 + 36 - 100 = -23, S = 177;
    SiLU(-23) = -23 / (1 + e^23)."""
    x = torch.tensor([2.0, -3.0]).view(1, 2, 1, 1)
    w = torch.tensor([0.5, 0.25]).view(1, 2, 1, 1)
    v, S, ref = CR.conv_ref(x, w, torch.tensor([1.0]), torch.tensor([0.5]).view(1, 1, 1, 1), 1, 1, 0, CR.ACT_RELU)
    assert float(v) == 1.25 and float(S) == 2.75 and float(ref) == 1.75
    x = torch.tensor([[1.0, 2.0], [3.0, 4.0]]).view(1, 1, 2, 2)
    w = (torch.arange(9, dtype=torch.float32) + 1).view(1, 1, 3, 3)
    v, S, ref = CR.conv_ref(x, w, torch.tensor([-100.0]), None, 3, 1, 1, CR.ACT_SILU)
    assert float(v[0, 0, 0, 0]) == -23.0 and float(S[0, 0, 0, 0]) == 177.0
    assert float(ref[0, 0, 0, 0]) == pytest.approx(-23.0 / (1.0 + math.exp(23.0)), rel=1e-15)
    # bottom-right output: x[1][1] under the centre, x[1][0] under (1, 0) = 4, x[0][1] under (0, 1) = 2, x[0][0] under (0, 0) = 1
    assert float(v[0, 0, 1, 1]) == 4 * 5 + 3 * 4 + 2 * 2 + 1 * 1 - 100
    # the far SiLU tail: exp overflows, the quotient is -0 and not NaN
    t = CR.act_ref(torch.tensor([-800.0, 800.0], dtype=F64), CR.ACT_SILU)
    assert float(t[0]) == 0.0 and math.copysign(1.0, float(t[0])) == -1.0 and float(t[1]) == 800.0


def _emulate(x, w, bias, res, k, stride, pad, act, dtype, drop=None):
    """The kernels' arithmetic on the CPU: an f32 convolution of the stored operands (exact products, f32 sums), optionally without
    input channel drop[0] under tap drop[1:], the activation and residual add in f32, one rounding into `dtype`."""
    v = F.conv2d(x, w, bias, stride=stride, padding=pad)
    if drop is not None:
        ci, kh, kw = drop
        w1 = torch.zeros_like(w)
        w1[:, ci, kh, kw] = w[:, ci, kh, kw]
        v = v - F.conv2d(x, w1, None, stride=stride, padding=pad)
    if act == CR.ACT_SILU:
        v = v / (1 + torch.exp(-v))
    elif act == CR.ACT_RELU:
        v = v.clamp_min(0)
    if res is not None:
        v = v + res
    return v.to(dtype).double()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("family", ["uniform", "saturated", "impulse", "impulse2"])
@pytest.mark.parametrize("k,stride,pad,act,with_res", [(1, 1, 0, CR.ACT_SILU, False), (3, 1, 1, CR.ACT_SILU, True), (3, 2, 1, CR.ACT_RELU, False),
                                                      (5, 1, 2, CR.ACT_NONE, True)], ids=lambda v: str(v))
def test_bound_holds_the_f32_emulation_and_rejects_a_dropped_tap(k, stride, pad, act, with_res, family, dtype):
    """The bound is neither empty nor loose: an f32 torch.conv2d of the stored operands, rounded into the storage type, lies inside it
    in every element; the same result with ONE input channel of ONE tap left out (the last channel under the last tap: what a wrong
    partial k-tile or a wrong halo mask loses) has elements outside it.  2 x 24 x 9 x 11 -> 24 channels (K = 24 .. 600)."""
    n, cin, h, wd, cout = 2, 24, 9, 11, 24
    oh, ow = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    x, w, bias, res = CR.conv_family(family, n, cin, h, wd, cout, k, dtype, 4242 + k, True, with_res, (oh, ow))
    v, S, ref = CR.conv_ref(x, w, bias, res, k, stride, pad, act)
    bound = CR.conv_bound(v, S, ref, cin * k * k, act, dtype)
    assert bool((bound > 0).all())
    if family == "saturated":
        assert float(v.max()) > 90 and float(v.min()) < -90
    y = _emulate(x, w, bias, res, k, stride, pad, act, dtype)
    err = (y - ref).abs()
    assert bool((err <= bound).all()), f"worst error / bound = {float((err / bound).max()):.3f}"
    drop = (cin - 1, k - 1, k - 1)
    if family.startswith("impulse"):  # a tap under which image 0's impulse (positive: ReLU keeps it) is sampled at this stride
        py, px = CR.impulse_positions(h, wd)[2 if family == "impulse2" else 0]
        drop = (cin - 1, (py + pad) % stride, (px + pad) % stride)
    yd = _emulate(x, w, bias, res, k, stride, pad, act, dtype, drop=drop)
    errd = (yd - ref).abs()
    assert int((errd > bound).sum()) >= 1, "a dropped (channel, tap) stays inside the bound"
    if not family.startswith("impulse"):
        # ... and not by a hair: the worst element misses by more than three times the bound
        assert float((errd / bound).max()) > 3.0
