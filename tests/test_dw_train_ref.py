"""tests/dw_train_ref.py pinned on the CPU: it IS float64 autograd of Sequential(Conv2d(groups=C, bias=False), BatchNorm2d, SiLU | Identity)
in train mode (1e-12, running statistics included); a float32 restatement in three summation orders stays inside its bounds; and each of
five wrong computations falls outside them - taps not flipped in dx, the biased variance written to running_var, the halo pixel dropped at
a tile seam, mean(g xhat) omitted from dz, dz rounded to bf16 before the weight gradient (the bound of a dz kept in float32 has no such
term)."""

import pytest
import torch

from tests import dw_train_ref as DR
from tests import psa_train_ref as PR
from tests import train_ref as TR

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
EPS, MOM = 1e-3, 0.03
T_ = 16  # the fused kernels' tile width: the seam of the halo control
SHAPE = (2, 9, T_ + 5, 8)


def _inputs(shape=SHAPE, seed=0):
    g = torch.Generator().manual_seed(seed)
    n, h, w, c = shape
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64)  # noqa: E731
    x, dy, wt = 2 * r(*shape) - 1, 2 * r(*shape) - 1, 2 * r(c, 1, 3, 3) - 1
    return x.float(), dy.float(), wt.float(), (0.5 + r(c)).float(), (r(c) - 0.5).float(), (r(c) - 0.5).float(), (0.5 + r(c)).float()


def _outside(got, ref, bound):
    return bool(((got.to(F64) - ref).abs() > bound).any())


def _inside(got, ref, bound, what):
    e = (got.to(F64) - ref).abs()
    assert bool((e <= bound).all()), (what, float((e / bound).max()))
    return float((e / bound).max())


@pytest.mark.parametrize("act", [TR.ACT_SILU, TR.ACT_NONE], ids=["silu", "none"])
def test_reference_is_float64_autograd(act):
    x, dy, wt, gamma, beta, rm, rv = (t.double() for t in _inputs())
    n, h, w, c = x.shape
    conv = torch.nn.Conv2d(c, c, 3, 1, 1, groups=c, bias=False).double()
    bn = torch.nn.BatchNorm2d(c, eps=TR.f32(EPS), momentum=TR.f32(MOM)).double()  # (the C ABI takes both as `float`)
    with torch.no_grad():
        conv.weight.copy_(wt), bn.weight.copy_(gamma), bn.bias.copy_(beta), bn.running_mean.copy_(rm), bn.running_var.copy_(rv)
    net = torch.nn.Sequential(conv, bn, torch.nn.SiLU() if act == TR.ACT_SILU else torch.nn.Identity()).train()
    xi = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = net(xi)
    y.backward(dy.permute(0, 3, 1, 2))
    f = DR.forward_ref(x, wt, gamma, beta, EPS, act, rm, rv, MOM, dtype=F64)
    b = DR.backward_ref(x, f["z_stored"], dy, wt, f["mean_stored"], f["var_stored"], gamma, beta, EPS, act, out_dtype=F64)
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1)  # noqa: E731
    pairs = [(f["y"], nhwc(y)), (f["running_mean"], bn.running_mean), (f["running_var"], bn.running_var), (b["dx"], nhwc(xi.grad)),
             (b["dw"], conv.weight.grad), (b["dgamma"], bn.weight.grad), (b["dbeta"], bn.bias.grad)]
    for i, (a, r) in enumerate(pairs):
        assert float((a - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max())), i


@pytest.mark.parametrize("act", [TR.ACT_SILU, TR.ACT_NONE], ids=["silu", "none"])
@pytest.mark.parametrize("order", ["natural", "reversed", "partitioned"])
def test_float32_orders_stay_inside_the_bounds(order, act):
    x, dy, wt, gamma, beta, rm, rv = _inputs(seed=1)
    e = DR.train_f32(x, dy, wt, gamma, beta, EPS, act, order)
    f = DR.forward_ref(x, wt, gamma, beta, EPS, act, rm, rv, MOM, dtype=F32, z=e["z"], mean=e["mean"], var=e["var"])
    b = DR.backward_ref(x, e["z"], dy, wt, e["mean"], e["var"], gamma, beta, EPS, act)
    worst = [_inside(e[k], f[k], f["b_" + k], k) for k in ("z", "mean", "var", "y")]
    worst += [_inside(e[k], b[k], b["b_" + k], k) for k in ("dz", "dgamma", "dbeta", "dx", "dw")]
    print(f"{order} act {act}: worst error / bound {max(worst):.3f}")


def test_negative_controls_fall_outside_the_bounds():
    x, dy, wt, gamma, beta, rm, rv = _inputs(seed=2)
    n, h, w, c = x.shape
    act = TR.ACT_SILU
    f = DR.forward_ref(x, wt, gamma, beta, EPS, act, rm, rv, MOM, dtype=F32)
    z, mean, var = f["z_stored"], f["mean_stored"], f["var_stored"]
    b = DR.backward_ref(x, z, dy, wt, mean, var, gamma, beta, EPS, act)
    assert not _outside(b["dx"], b["dx"], b["b_dx"])
    # 1. taps not flipped in dx
    wrong = DR.backward_ref(x, z, dy, wt, mean, var, gamma, beta, EPS, act, unflipped=True)
    assert _outside(wrong["dx"], b["dx"], b["b_dx"]) and not _outside(wrong["dw"], b["dw"], b["b_dw"])
    # 2. the biased variance written to running_var
    m = TR.f32(MOM)
    assert _outside((1.0 - m) * rv.double() + m * f["var"], f["running_var"], f["b_running_var"])
    # 3. the halo pixel dropped at a tile seam: the tile left of column T_ reads dz[:, :, T_] as zero
    dz = b["dz"]
    lost = torch.zeros_like(dz)
    lost[:, :, T_] = dz[:, :, T_]
    miss = PR.dw_bwd_ref(x, lost, wt)[0]
    dx_seam = b["dx"].clone()
    dx_seam[:, :, T_ - 1] -= miss[:, :, T_ - 1]
    assert _outside(dx_seam, b["dx"], b["b_dx"])
    x_lost = x.double().clone()  # ... and the weight gradient's x halo: the tile right of the seam reads x[:, :, T_ - 1] as zero
    dw_seam = b["dw"].clone()
    for kh in range(3):
        dw_seam[:, 0, kh, 0] -= (dz[:, :, T_] * PR._shift(x_lost, kh - 1, -1)[:, :, T_]).sum(dim=(0, 1))
    assert _outside(dw_seam, b["dw"], b["b_dw"])
    # 4. mean(g xhat) omitted from dz
    wrong = DR.backward_ref(x, z, dy, wt, mean, var, gamma, beta, EPS, act, drop_xhat_mean=True)
    assert _outside(wrong["dz"], b["dz"], b["b_dz"]) and _outside(wrong["dx"], b["dx"], b["b_dx"]) and _outside(wrong["dw"], b["dw"], b["b_dw"])
    # 5. dz rounded to bf16 before the weight gradient: outside the bound of a float32 dz, inside the one that carries the store
    dw_r = PR.dw_bwd_ref(x, dz.to(BF16), wt)[2]
    assert _outside(dw_r, b["dw"], b["b_dw"])
    stored = DR.backward_ref(x, z, dy, wt, mean, var, gamma, beta, EPS, act, dz_dtype=BF16)
    assert not _outside(dw_r, stored["dw"], stored["b_dw"])


def test_bounds_scale_with_the_operands_only():
    """Scaling dy by 2^k scales every backward reference and bound by 2^k: no literal sits in a bound."""
    x, dy, wt, gamma, beta, rm, rv = _inputs(seed=3)
    f = DR.forward_ref(x, wt, gamma, beta, EPS, TR.ACT_SILU, dtype=F32)
    a = DR.backward_ref(x, f["z_stored"], dy, wt, f["mean_stored"], f["var_stored"], gamma, beta, EPS, TR.ACT_SILU)
    s = DR.backward_ref(x, f["z_stored"], dy * 1024.0, wt, f["mean_stored"], f["var_stored"], gamma, beta, EPS, TR.ACT_SILU)
    for k in ("dx", "dw", "b_dx", "b_dw", "b_dz"):
        assert torch.allclose(s[k], 1024.0 * a[k], rtol=1e-9, atol=1e-280), k
